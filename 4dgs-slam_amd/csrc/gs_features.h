// gs_features.h -- the kernels of include/feature_matching.h: FAST-9 corners with rotated BRIEF descriptors in a fixed slot layout
// (gsr_feat_extract), the mutual ratio-tested Hamming match of two such sets (gsr_feat_match) and three-point RANSAC with a point-to-point
// refinement and a gate on the back-projected matches (gsr_feat_pose), or the same from the 3D points of A and the pixels of B alone
// (gsr_feat_pose_pnp). gfx950 / wave64; every LDS size is a compile-time constant; no atomics anywhere: every result is formed thread ->
// wave -> block in one fixed order.
//
// Extract, per call:  feat_score_kernel        a 16 x 16 tile per block with a halo of 3 of luma bytes in LDS: luma, the corner score c(p)
//                                              and the 5 x 5 sum of every pixel
//                     feat_select_kernel       one block per cell: c of the cell and a ring of one pixel in LDS, suppression, then per_cell
//                                              rounds of a block-wide maximum of the key score << 24 | (area - 1 - local index)
//                     feat_describe_kernel     one wave per slot: the moments of the disc summed by lanes, the bin, 4 bits per lane and a
//                                              ballot per pair of words
// Match, per call:    feat_nearest_kernel      one wave per slot, lanes striding over the other set: best key d << 16 | index and second d
//                                              (run both ways), feat_mutual_kernel: thread per slot of A
// Pose, per call:     feat_pairs_kernel        (one block) the list of pairs with two valid depths, compacted in ascending a by ballots
//                     feat_hypotheses_kernel   one wave per hypothesis: the pose of three pairs, the inliers by ballot + popcount
//                     feat_finish_kernel       (one block) winner, Gauss-Newton in double, recount, gate
//                     each of the three is a template over PNP: <false> is gsr_feat_pose; <true>, gsr_feat_pose_pnp, reads no depth of B,
//                     keeps B's bearings where <false> keeps B's points, finds the three ranges along them by Newton in double
//                     (feat_ranges) before the same triads, tests the reprojection alone and refines the reprojection error
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "gs_reloc.h"                          // reloc_quant: q(v) of relocalisation.h

namespace gsr {

constexpr int FEAT_BLOCK = 256;
constexpr int FEAT_WAVES = FEAT_BLOCK / 64;
constexpr int FEAT_TILE = 16, FEAT_HALO = 3, FEAT_SPAN = FEAT_TILE + 2 * FEAT_HALO;
constexpr int FEAT_BORDER = 18;                // 16 (the clamp of the pattern) + 2 (the 5 x 5 sum); the disc's 15 lies inside
constexpr int FEAT_MIN_CELL = 8, FEAT_MAX_CELL = 64, FEAT_MAX_PER_CELL = 8, FEAT_MAX_SLOTS = 4096;
constexpr int FEAT_RING = FEAT_MAX_CELL + 2;
constexpr int FEAT_WORDS = 8, FEAT_BINS = 32, FEAT_PAIRS = 256, FEAT_RADIUS = 15, FEAT_CLAMP = 16;
constexpr int FEAT_NONE = 257;                 // the distance of "no match"; FEAT_NONE << 16 | 0xFFFF is the key of "none"
constexpr unsigned FEAT_NO_KEY = (unsigned)FEAT_NONE << 16 | 0xFFFFu;
constexpr int FEAT_MAX_HYPOTHESES = 1024;
constexpr int FEAT_MAX_REFINE = 16;
constexpr int FEAT_SUMS = 27;                  // 21 of H (upper triangle, row-major) and 6 of g
constexpr int FEAT_STATS = 8;
constexpr int FEAT_NEWTON = 8;                 // the steps of feat_ranges

__device__ __forceinline__ int feat_block_sum(int v, int* part)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();                                                   // part may still be read from an earlier call
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    int s = 0;
#pragma unroll
    for (int w = 0; w < FEAT_WAVES; ++w) s += part[w];
    return s;
}

__device__ __forceinline__ unsigned feat_block_max(unsigned v, unsigned* part)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, (unsigned)__shfl_xor(v, o, 64));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    unsigned m = part[0];
#pragma unroll
    for (int w = 1; w < FEAT_WAVES; ++w) m = max(m, part[w]);
    return m;
}

// ---- extract -------------------------------------------------------------------------------------------------------------------------
// grid: (ceil(W / 16), ceil(H / 16)); thread (lx, ly) of a block owns one pixel
__global__ void __launch_bounds__(FEAT_BLOCK) feat_score_kernel(int W, int H, const float* __restrict__ image, const unsigned char* __restrict__ mask,
                                                                int threshold, unsigned char* __restrict__ luma, unsigned char* __restrict__ corner,
                                                                unsigned short* __restrict__ box)
{
    __shared__ unsigned char tile[FEAT_SPAN][FEAT_SPAN + 2];
    const int x0 = (int)blockIdx.x * FEAT_TILE - FEAT_HALO, y0 = (int)blockIdx.y * FEAT_TILE - FEAT_HALO;
    const size_t n = (size_t)W * H;
    for (int k = threadIdx.x; k < FEAT_SPAN * FEAT_SPAN; k += FEAT_BLOCK) {
        const int ty = k / FEAT_SPAN, tx = k % FEAT_SPAN, x = x0 + tx, y = y0 + ty;
        int L = 0;
        if (x >= 0 && x < W && y >= 0 && y < H) {
            const size_t p = (size_t)y * W + x;
            L = (77 * reloc_quant(image[p]) + 150 * reloc_quant(image[n + p]) + 29 * reloc_quant(image[2 * n + p]) + 128) >> 8;
        }
        tile[ty][tx] = (unsigned char)L;
    }
    __syncthreads();
    const int lx = threadIdx.x & (FEAT_TILE - 1), ly = threadIdx.x / FEAT_TILE;
    const int x = (int)blockIdx.x * FEAT_TILE + lx, y = (int)blockIdx.y * FEAT_TILE + ly;
    if (x >= W || y >= H) return;
    const int cx = lx + FEAT_HALO, cy = ly + FEAT_HALO;
    const size_t p = (size_t)y * W + x;
    const int centre = tile[cy][cx];
    int S = 0;
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy)
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) S += tile[cy + dy][cx + dx];
    luma[p] = (unsigned char)centre;
    box[p] = (unsigned short)S;                                        // at most 25 * 255
    int c = 0;
    const bool interior = x >= FEAT_BORDER && x < W - FEAT_BORDER && y >= FEAT_BORDER && y < H - FEAT_BORDER;
    if (interior && (!mask || mask[p])) {
        constexpr int OX[16] = {0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1};
        constexpr int OY[16] = {-3, -3, -2, -1, 0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3};
        int d[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) d[k] = (int)tile[cy + OY[k]][cx + OX[k]] - centre;
        int bright = -255, dark = -255;
#pragma unroll
        for (int s = 0; s < 16; ++s) {
            int lo = d[s], hi = -d[s];
#pragma unroll
            for (int j = 1; j < 9; ++j) {
                lo = min(lo, d[(s + j) & 15]);
                hi = min(hi, -d[(s + j) & 15]);
            }
            bright = max(bright, lo);
            dark = max(dark, hi);
        }
        const int score = max(max(bright, dark), 0);
        if (score > threshold) c = score;
    }
    corner[p] = (unsigned char)c;
}

// grid: one block per cell. keypoints: (x, y, score, 0) per slot, (-1, -1, 0, 0) for an empty one; feat_describe_kernel adds the bin.
__global__ void __launch_bounds__(FEAT_BLOCK) feat_select_kernel(int W, int H, int cell, int per_cell, int cells_x,
                                                                 const unsigned char* __restrict__ corner, int* __restrict__ keypoints)
{
    __shared__ unsigned char ring[FEAT_RING * FEAT_RING];
    __shared__ unsigned keys[FEAT_MAX_CELL * FEAT_MAX_CELL];
    __shared__ unsigned part[FEAT_WAVES];
    const int ci = (int)blockIdx.x % cells_x, cj = (int)blockIdx.x / cells_x;
    const int x0 = ci * cell, y0 = cj * cell, span = cell + 2, area = cell * cell;
    for (int k = threadIdx.x; k < span * span; k += FEAT_BLOCK) {
        const int x = x0 - 1 + k % span, y = y0 - 1 + k / span;
        ring[k] = (x >= 0 && x < W && y >= 0 && y < H) ? corner[(size_t)y * W + x] : (unsigned char)0;
    }
    __syncthreads();
    for (int k = threadIdx.x; k < area; k += FEAT_BLOCK) {
        const int at = (k / cell + 1) * span + k % cell + 1;
        const unsigned c = ring[at];
        bool kept = c > 0u;
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) {
                if (dx == 0 && dy == 0) continue;
                const unsigned nc = ring[at + dy * span + dx];
                const bool earlier = dy < 0 || (dy == 0 && dx < 0);    // the neighbour's index y W + x is the smaller one
                if (nc > c || (nc == c && earlier)) kept = false;
            }
        keys[k] = kept ? (c << 24 | (unsigned)(area - 1 - k)) : 0u;    // area <= 4096: 12 bits; distinct among the kept
    }
    unsigned last = 0xFFFFFFFFu;
    for (int r = 0; r < per_cell; ++r) {
        unsigned m = 0u;
        for (int k = threadIdx.x; k < area; k += FEAT_BLOCK) {
            const unsigned key = keys[k];
            if (key < last && key > m) m = key;
        }
        m = feat_block_max(m, part);                                   // a thread reads only the keys it wrote itself: no barrier before
        if (threadIdx.x == 0) {
            int* out = keypoints + ((size_t)blockIdx.x * per_cell + r) * 4;
            const int k = area - 1 - (int)(m & 0xFFFFFFu);
            out[0] = m ? x0 + k % cell : -1;
            out[1] = m ? y0 + k / cell : -1;
            out[2] = (int)(m >> 24);
            out[3] = 0;
        }
        last = m;                                                      // 0 once the cell is exhausted: every later round gives 0 too
    }
}

// grid: ceil(slots / 4) blocks of four waves, one wave per slot
__global__ void __launch_bounds__(FEAT_BLOCK) feat_describe_kernel(int W, int slots, const unsigned char* __restrict__ luma,
                                                                   const unsigned short* __restrict__ box, const int* __restrict__ directions,
                                                                   const signed char* __restrict__ pattern, int* __restrict__ keypoints,
                                                                   unsigned* __restrict__ descriptors)
{
    const int slot = (int)blockIdx.x * FEAT_WAVES + (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (slot >= slots) return;                                         // the whole wave
    const int x = keypoints[4 * slot], y = keypoints[4 * slot + 1];
    if (x < 0) {
        if (lane < FEAT_WORDS) descriptors[(size_t)slot * FEAT_WORDS + lane] = 0u;
        return;
    }
    // x, y came from feat_select_kernel: at least FEAT_BORDER from every edge, so every read below is inside the image
    constexpr int SIDE = 2 * FEAT_RADIUS + 1;
    int m10 = 0, m01 = 0;                                              // at most 709 * 15 * 255 in size
    for (int k = lane; k < SIDE * SIDE; k += 64) {
        const int dy = k / SIDE - FEAT_RADIUS, dx = k % SIDE - FEAT_RADIUS;
        if (dx * dx + dy * dy > FEAT_RADIUS * FEAT_RADIUS) continue;
        const int L = luma[(size_t)(y + dy) * W + (x + dx)];
        m10 += dx * L;
        m01 += dy * L;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        m10 += __shfl_xor(m10, o, 64);
        m01 += __shfl_xor(m01, o, 64);
    }
    int bin = 0;
    long long top = 0;
    for (int k = 0; k < FEAT_BINS; ++k) {
        const long long v = (long long)directions[2 * k] * m10 + (long long)directions[2 * k + 1] * m01;
        if (k == 0 || v > top) {
            top = v;
            bin = k;
        }
    }
    if (lane == 0) keypoints[4 * slot + 3] = bin;
    const signed char* pairs = pattern + (size_t)bin * FEAT_PAIRS * 4;
#pragma unroll
    for (int j = 0; j < FEAT_PAIRS / 64; ++j) {
        const signed char* q = pairs + (size_t)(64 * j + lane) * 4;
        const int ax = min(max((int)q[0], -FEAT_CLAMP), FEAT_CLAMP), ay = min(max((int)q[1], -FEAT_CLAMP), FEAT_CLAMP);
        const int bx = min(max((int)q[2], -FEAT_CLAMP), FEAT_CLAMP), by = min(max((int)q[3], -FEAT_CLAMP), FEAT_CLAMP);
        const int Sa = box[(size_t)(y + ay) * W + (x + ax)], Sb = box[(size_t)(y + by) * W + (x + bx)];
        const unsigned long long bits = __ballot(Sa < Sb);
        if (lane == 0) {
            descriptors[(size_t)slot * FEAT_WORDS + 2 * j] = (unsigned)bits;
            descriptors[(size_t)slot * FEAT_WORDS + 2 * j + 1] = (unsigned)(bits >> 32);
        }
    }
}

// ---- match ---------------------------------------------------------------------------------------------------------------------------
// grid: ceil(slots_a / 4) blocks, one wave per slot a. best[a] = d << 16 | b of the smallest (d, b), second[a] = the smallest d of the others
__global__ void __launch_bounds__(FEAT_BLOCK) feat_nearest_kernel(int slots_a, const int* __restrict__ kp_a, const unsigned* __restrict__ desc_a,
                                                                  int slots_b, const int* __restrict__ kp_b, const unsigned* __restrict__ desc_b,
                                                                  unsigned* __restrict__ best, int* __restrict__ second)
{
    const int a = (int)blockIdx.x * FEAT_WAVES + (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (a >= slots_a) return;
    unsigned key = FEAT_NO_KEY;
    int sec = FEAT_NONE;
    if (kp_a[4 * a] >= 0) {
        unsigned da[FEAT_WORDS];
#pragma unroll
        for (int w = 0; w < FEAT_WORDS; ++w) da[w] = desc_a[(size_t)a * FEAT_WORDS + w];
        for (int b = lane; b < slots_b; b += 64) {
            if (kp_b[4 * b] < 0) continue;
            int d = 0;
#pragma unroll
            for (int w = 0; w < FEAT_WORDS; ++w) d += __popc(da[w] ^ desc_b[(size_t)b * FEAT_WORDS + w]);
            const unsigned k = (unsigned)d << 16 | (unsigned)b;
            if (k < key) {
                sec = min(sec, (int)(key >> 16));
                key = k;
            } else {
                sec = min(sec, d);
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned other = (unsigned)__shfl_xor(key, o, 64);
        const int other_sec = __shfl_xor(sec, o, 64);
        const unsigned lo = min(key, other), hi = max(key, other);
        sec = min(min(sec, other_sec), (int)(hi >> 16));               // the loser of the two bests is a second
        key = lo;
    }
    if (lane == 0) {
        best[a] = key;
        second[a] = sec;
    }
}

// thread per slot a
__global__ void __launch_bounds__(FEAT_BLOCK) feat_mutual_kernel(int slots_a, int slots_b, const unsigned* __restrict__ best_ab,
                                                                 const int* __restrict__ second_ab, const unsigned* __restrict__ best_ba,
                                                                 int max_distance, int ratio_eighths, int* __restrict__ matches)
{
    const int a = (int)blockIdx.x * FEAT_BLOCK + (int)threadIdx.x;
    if (a >= slots_a) return;
    const unsigned key = best_ab[a];
    const int d = (int)(key >> 16), b = (int)(key & 0xFFFFu);
    bool ok = key != FEAT_NO_KEY && b < slots_b && d <= max_distance && 8 * d <= ratio_eighths * second_ab[a];
    if (ok) ok = (int)(best_ba[b] & 0xFFFFu) == a;
    matches[2 * a] = ok ? b : -1;
    matches[2 * a + 1] = d;
}

// ---- pose ----------------------------------------------------------------------------------------------------------------------------
struct FeatPoseWs { float* PA; float* PB; float* UV; int* head; int* hyp; size_t bytes; };    // head: M
struct FeatRt { float R[9]; float t[3]; };

__device__ __forceinline__ unsigned feat_lowbias32(unsigned x)
{
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}

// the triad of the header: e[0..2] = e1, e[3..5] = e2, e[6..8] = e3; false where n3 >= min_area fails (a NaN fails it)
__device__ __forceinline__ bool feat_triad(const float* p1, const float* p2, const float* p3, float min_area, float* e)
{
#pragma clang fp contract(off)
    const float dx = p2[0] - p1[0], dy = p2[1] - p1[1], dz = p2[2] - p1[2];
    const float n1 = sqrtf(dx * dx + dy * dy + dz * dz);
    e[0] = dx / n1, e[1] = dy / n1, e[2] = dz / n1;
    const float gx = p3[0] - p1[0], gy = p3[1] - p1[1], gz = p3[2] - p1[2];
    const float cx = e[1] * gz - e[2] * gy, cy = e[2] * gx - e[0] * gz, cz = e[0] * gy - e[1] * gx;
    const float n3 = sqrtf(cx * cx + cy * cy + cz * cz);
    if (!(n3 >= min_area)) return false;
    e[6] = cx / n3, e[7] = cy / n3, e[8] = cz / n3;
    e[3] = e[7] * e[2] - e[8] * e[1], e[4] = e[8] * e[0] - e[6] * e[2], e[5] = e[6] * e[1] - e[7] * e[0];
    return true;
}

// the three indices of hypothesis h; false with M < 3 or two equal indices
__device__ __forceinline__ bool feat_draw(unsigned seed, int h, int M, unsigned* i)
{
    if (M < 3) return false;
    const unsigned base = seed * 0x9E3779B9u + 3u * (unsigned)h;
    i[0] = feat_lowbias32(base) % (unsigned)M, i[1] = feat_lowbias32(base + 1u) % (unsigned)M, i[2] = feat_lowbias32(base + 2u) % (unsigned)M;
    return !(i[0] == i[1] || i[0] == i[2] || i[1] == i[2]);
}

// R, t that take the triple a to the triple b; false where either triad is void
__device__ __forceinline__ bool feat_motion(const float* a1, const float* a2, const float* a3, const float* b1, const float* b2, const float* b3,
                                            float min_area, FeatRt& rt)
{
#pragma clang fp contract(off)
    float ea[9], eb[9];
    const bool ok_a = feat_triad(a1, a2, a3, min_area, ea), ok_b = feat_triad(b1, b2, b3, min_area, eb);
    if (!ok_a || !ok_b) return false;
    float ma[3], mb[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        ma[i] = (a1[i] + a2[i] + a3[i]) / 3.0f;
        mb[i] = (b1[i] + b2[i] + b3[i]) / 3.0f;
    }
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) rt.R[3 * i + j] = eb[i] * ea[j] + eb[3 + i] * ea[3 + j] + eb[6 + i] * ea[6 + j];
#pragma unroll
    for (int i = 0; i < 3; ++i) rt.t[i] = mb[i] - (rt.R[3 * i] * ma[0] + rt.R[3 * i + 1] * ma[1] + rt.R[3 * i + 2] * ma[2]);
    return true;
}

// the ranges of the header (gsr_feat_pose_pnp): the points pb[3 k + i] = (float)(l_k f_k) of B on the bearings u1, u2, u3 whose mutual
// distances are those of p1, p2, p3; float64, every operation rounded by itself, in the order written here and in tests/pnp_reference.py.
// false for a void hypothesis
__device__ inline bool feat_ranges(const float* p1, const float* p2, const float* p3, const float* u1, const float* u2, const float* u3, float* pb)
{
#pragma clang fp contract(off)
    const float* P[3] = {p1, p2, p3};
    const float* U[3] = {u1, u2, u3};
    double f[3][3], l[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double ux = (double)U[k][0], uy = (double)U[k][1], uz = (double)U[k][2];
        const double n = sqrt(ux * ux + uy * uy + uz * uz);
        f[k][0] = ux / n, f[k][1] = uy / n, f[k][2] = uz / n;
        const double px = (double)P[k][0], py = (double)P[k][1], pz = (double)P[k][2];
        l[k] = sqrt(px * px + py * py + pz * pz);
    }
    double c[3], d[3];                                                 // of the pairs (1, 2), (1, 3), (2, 3)
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int i = k == 2 ? 1 : 0, j = k == 0 ? 1 : 2;
        c[k] = f[i][0] * f[j][0] + f[i][1] * f[j][1] + f[i][2] * f[j][2];
        const double dx = (double)P[i][0] - (double)P[j][0], dy = (double)P[i][1] - (double)P[j][1], dz = (double)P[i][2] - (double)P[j][2];
        d[k] = dx * dx + dy * dy + dz * dz;
    }
    double l1 = l[0], l2 = l[1], l3 = l[2];
    for (int it = 0; it < FEAT_NEWTON; ++it) {
        const double F1 = l1 * l1 + l2 * l2 - 2.0 * l1 * l2 * c[0] - d[0];
        const double F2 = l1 * l1 + l3 * l3 - 2.0 * l1 * l3 * c[1] - d[1];
        const double F3 = l2 * l2 + l3 * l3 - 2.0 * l2 * l3 * c[2] - d[2];
        const double ja = 2.0 * l1 - 2.0 * l2 * c[0], jb = 2.0 * l2 - 2.0 * l1 * c[0];      // the Jacobian [ja jb 0; jc 0 jd; 0 je jg]
        const double jc = 2.0 * l1 - 2.0 * l3 * c[1], jd = 2.0 * l3 - 2.0 * l1 * c[1];
        const double je = 2.0 * l2 - 2.0 * l3 * c[2], jg = 2.0 * l3 - 2.0 * l2 * c[2];
        const double det = -ja * jd * je - jb * jc * jg;
        if (det == 0.0 || !isfinite(det)) return false;
        const double w = F2 * jg - jd * F3;
        const double n1 = -F1 * jd * je - jb * w, n2 = ja * w - F1 * jc * jg, n3 = -ja * F2 * je - jb * jc * F3 + F1 * jc * je;
        l1 = l1 - n1 / det, l2 = l2 - n2 / det, l3 = l3 - n3 / det;
    }
    const double F1 = l1 * l1 + l2 * l2 - 2.0 * l1 * l2 * c[0] - d[0];
    const double F2 = l1 * l1 + l3 * l3 - 2.0 * l1 * l3 * c[1] - d[1];
    const double F3 = l2 * l2 + l3 * l3 - 2.0 * l2 * l3 * c[2] - d[2];
    if (!(isfinite(l1) && l1 > 0.0 && isfinite(l2) && l2 > 0.0 && isfinite(l3) && l3 > 0.0)) return false;
    if (!(fabs(F1) <= 1e-9 * d[0] && fabs(F2) <= 1e-9 * d[1] && fabs(F3) <= 1e-9 * d[2])) return false;
    l[0] = l1, l[1] = l2, l[2] = l3;
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int i = 0; i < 3; ++i) pb[3 * k + i] = (float)(l[k] * f[k][i]);
    return true;
}

// R, t of hypothesis h; false for a void one. PNP: PB holds the bearings of B, and the points of B's triple come from feat_ranges
template <bool PNP>
__device__ __forceinline__ bool feat_hypothesis(unsigned seed, int h, int M, const float* __restrict__ PA, const float* __restrict__ PB,
                                                float min_area, FeatRt& rt)
{
    unsigned i[3];
    if (!feat_draw(seed, h, M, i)) return false;
    const float *a1 = PA + 3 * (size_t)i[0], *a2 = PA + 3 * (size_t)i[1], *a3 = PA + 3 * (size_t)i[2];
    const float *b1 = PB + 3 * (size_t)i[0], *b2 = PB + 3 * (size_t)i[1], *b3 = PB + 3 * (size_t)i[2];
    if constexpr (PNP) {
        float pb[9];
        return feat_ranges(a1, a2, a3, b1, b2, b3, pb) && feat_motion(a1, a2, a3, pb, pb + 3, pb + 6, min_area, rt);
    } else {
        return feat_motion(a1, a2, a3, b1, b2, b3, min_area, rt);
    }
}

// Q = R P + t and the squared reprojection error e2 against uv = (x_b, y_b); K = (fx, fy, cx, cy) of frame B; false where Q_z > 0 fails
__device__ __forceinline__ bool feat_project(const FeatRt& rt, const float* P, const float* uv, const float* K, float& Qz, float& e2)
{
#pragma clang fp contract(off)
    const float Qx = rt.R[0] * P[0] + rt.R[1] * P[1] + rt.R[2] * P[2] + rt.t[0];
    const float Qy = rt.R[3] * P[0] + rt.R[4] * P[1] + rt.R[5] * P[2] + rt.t[1];
    Qz = rt.R[6] * P[0] + rt.R[7] * P[1] + rt.R[8] * P[2] + rt.t[2];
    if (!(Qz > 0.f)) return false;
    const float ex = K[0] * (Qx / Qz) + K[2] - uv[0], ey = K[1] * (Qy / Qz) + K[3] - uv[1];
    e2 = ex * ex + ey * ey;
    return true;
}

// the inlier test of the header for pair m; a NaN anywhere fails it. PNP: the reprojection alone, nothing of PB is read
template <bool PNP>
__device__ __forceinline__ bool feat_inlier(const FeatRt& rt, const FeatPoseWs& ws, int m, const float* K, float tau_px, float tau_depth)
{
#pragma clang fp contract(off)
    float Qz, e2;
    if (!feat_project(rt, ws.PA + 3 * (size_t)m, ws.UV + 2 * (size_t)m, K, Qz, e2)) return false;
    const float bar2 = tau_px * tau_px;
    if constexpr (PNP) {
        return e2 <= bar2;
    } else {
        const float zb = ws.PB[3 * (size_t)m + 2];
        const float gap = fabsf(Qz - zb), bar = tau_depth * zb;
        return e2 <= bar2 && gap <= bar;
    }
}

// one block. stats[0..2] = valid keypoints of A, of B, M. PNP: depth_b is never read (NULL), and PB holds the bearing ((x_b - cx_b) / fx_b,
// (y_b - cy_b) / fy_b, 1) of B's keypoint
template <bool PNP>
__global__ void __launch_bounds__(FEAT_BLOCK) feat_pairs_kernel(int W, int H, int slots_a, const int* __restrict__ kp_a, const float* __restrict__ depth_a,
                                                                int slots_b, const int* __restrict__ kp_b, const float* __restrict__ depth_b,
                                                                const int* __restrict__ matches, const float* __restrict__ K_a,
                                                                const float* __restrict__ K_b, FeatPoseWs ws, int* __restrict__ stats)
{
#pragma clang fp contract(off)
    __shared__ int part[FEAT_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int base = 0;
    for (int start = 0; start < slots_a; start += FEAT_BLOCK) {
        const int a = start + tid;
        bool ok = false;
        float pa[3], pb[3], uv[2];
        if (a < slots_a) {
            const int b = matches[2 * a], xa = kp_a[4 * a], ya = kp_a[4 * a + 1];
            if (b >= 0 && b < slots_b && xa >= 0 && xa < W && ya >= 0 && ya < H) {
                const int xb = kp_b[4 * b], yb = kp_b[4 * b + 1];
                if (xb >= 0 && xb < W && yb >= 0 && yb < H) {
                    const float za = depth_a[(size_t)ya * W + xa];
                    float zb = 1.f;
                    if constexpr (!PNP) zb = depth_b[(size_t)yb * W + xb];
                    if (isfinite(za) && za > 0.f && isfinite(zb) && zb > 0.f) {
                        ok = true;
                        pa[0] = ((float)xa - K_a[2]) * za / K_a[0], pa[1] = ((float)ya - K_a[3]) * za / K_a[1], pa[2] = za;
                        if constexpr (PNP) pb[0] = ((float)xb - K_b[2]) / K_b[0], pb[1] = ((float)yb - K_b[3]) / K_b[1], pb[2] = 1.f;
                        else pb[0] = ((float)xb - K_b[2]) * zb / K_b[0], pb[1] = ((float)yb - K_b[3]) * zb / K_b[1], pb[2] = zb;
                        uv[0] = (float)xb, uv[1] = (float)yb;
                    }
                }
            }
        }
        const unsigned long long bits = __ballot(ok);
        __syncthreads();                                               // part of the chunk before has been read
        if (lane == 0) part[wave] = __popcll(bits);
        __syncthreads();
        int at = base + __popcll(bits & ((1ull << lane) - 1ull));
        for (int w = 0; w < FEAT_WAVES; ++w) {
            if (w < wave) at += part[w];
            base += part[w];
        }
        if (ok) {                                                      // at < slots_a: one entry per slot at most
#pragma unroll
            for (int i = 0; i < 3; ++i) ws.PA[3 * (size_t)at + i] = pa[i], ws.PB[3 * (size_t)at + i] = pb[i];
            ws.UV[2 * (size_t)at] = uv[0], ws.UV[2 * (size_t)at + 1] = uv[1];
        }
    }
    int na = 0, nb = 0;
    for (int a = tid; a < slots_a; a += FEAT_BLOCK) na += kp_a[4 * a] >= 0;
    for (int b = tid; b < slots_b; b += FEAT_BLOCK) nb += kp_b[4 * b] >= 0;
    na = feat_block_sum(na, part);
    nb = feat_block_sum(nb, part);
    if (tid == 0) {
        ws.head[0] = base;
        stats[0] = na, stats[1] = nb, stats[2] = base;
    }
}

// grid: ceil(hypotheses / 4) blocks, one wave per hypothesis; PNP: every lane runs the wave-uniform Newton of feat_ranges itself
template <bool PNP>
__global__ void __launch_bounds__(FEAT_BLOCK) feat_hypotheses_kernel(int hypotheses, unsigned seed, float min_area, float tau_px, float tau_depth,
                                                                     const float* __restrict__ K_b, FeatPoseWs ws, int* __restrict__ counts)
{
    const int h = (int)blockIdx.x * FEAT_WAVES + (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (h >= hypotheses) return;
    const int M = ws.head[0];
    const float K[4] = {K_b[0], K_b[1], K_b[2], K_b[3]};
    FeatRt rt;
    int count = 0;
    if (feat_hypothesis<PNP>(seed, h, M, ws.PA, ws.PB, min_area, rt)) {
        for (int m0 = 0; m0 < M; m0 += 64) {
            const int m = m0 + lane;
            const bool in = m < M && feat_inlier<PNP>(rt, ws, m, K, tau_px, tau_depth);
            count += __popcll(__ballot(in));
        }
    }
    if (lane == 0) {
        ws.hyp[h] = count;
        if (counts) counts[h] = count;
    }
}

// H xi = -g by Cholesky, H the upper triangle row-major; false where H is not positive definite or xi is not finite
__device__ inline bool feat_solve6(const double* s, double* xi)
{
    double A[6][6], L[6][6] = {};
    int k = 0;
    for (int i = 0; i < 6; ++i)
        for (int j = i; j < 6; ++j) A[i][j] = A[j][i] = s[k++];
    for (int i = 0; i < 6; ++i)
        for (int j = 0; j <= i; ++j) {
            double v = A[i][j];
            for (int q = 0; q < j; ++q) v -= L[i][q] * L[j][q];
            if (i == j) {
                if (!(v > 0.0) || !isfinite(v)) return false;
                L[i][i] = sqrt(v);
            } else {
                L[i][j] = v / L[j][j];
            }
        }
    double y[6];
    for (int i = 0; i < 6; ++i) {
        double v = -s[21 + i];
        for (int q = 0; q < i; ++q) v -= L[i][q] * y[q];
        y[i] = v / L[i][i];
    }
    for (int i = 5; i >= 0; --i) {
        double v = y[i];
        for (int q = i + 1; q < 6; ++q) v -= L[q][i] * xi[q];
        xi[i] = v / L[i][i];
    }
    for (int i = 0; i < 6; ++i)
        if (!isfinite(xi[i])) return false;
    return true;
}

// pose <- exp(xi) pose; pose = R row-major [0..8], t [9..11]; xi = [rho | theta]. With a = |theta|: A = sin a / a, B = (1 - cos a) / a^2,
// C = (a - sin a) / a^3 (1, 1/2, 1/6 below 1e-6); exp = [I + A W + B W^2 | (I + B W + C W^2) rho], W = [theta]x
__device__ inline void feat_exp_apply(const double* xi, double* pose)
{
    const double wx = xi[3], wy = xi[4], wz = xi[5];
    const double a2 = wx * wx + wy * wy + wz * wz, a = sqrt(a2);
    double A = 1.0, B = 0.5, C = 1.0 / 6.0;
    if (a >= 1e-6) {
        A = sin(a) / a;
        B = (1.0 - cos(a)) / a2;
        C = (a - sin(a)) / (a2 * a);
    }
    const double Wm[9] = {0.0, -wz, wy, wz, 0.0, -wx, -wy, wx, 0.0};
    double W2[9], dR[9], V[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) W2[3 * i + j] = Wm[3 * i] * Wm[j] + Wm[3 * i + 1] * Wm[3 + j] + Wm[3 * i + 2] * Wm[6 + j];
    for (int k = 0; k < 9; ++k) {
        const double I = (k % 4 == 0) ? 1.0 : 0.0;
        dR[k] = I + A * Wm[k] + B * W2[k];
        V[k] = I + B * Wm[k] + C * W2[k];
    }
    double R[9], t[3];
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) R[3 * i + j] = dR[3 * i] * pose[j] + dR[3 * i + 1] * pose[3 + j] + dR[3 * i + 2] * pose[6 + j];
        t[i] = dR[3 * i] * pose[9] + dR[3 * i + 1] * pose[10] + dR[3 * i + 2] * pose[11] + (V[3 * i] * xi[0] + V[3 * i + 1] * xi[1] + V[3 * i + 2] * xi[2]);
    }
    for (int k = 0; k < 9; ++k) pose[k] = R[k];
    for (int i = 0; i < 3; ++i) pose[9 + i] = t[i];
}

// acc += the 27 sums of ROWS rows of J and their residuals r
template <int ROWS>
__device__ __forceinline__ void feat_add_rows(double* acc, const double (*J)[6], const double* r)
{
#pragma unroll
    for (int row = 0; row < ROWS; ++row) {
        int k = 0;
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
            for (int j = i; j < 6; ++j) acc[k++] += J[row][i] * J[row][j];
#pragma unroll
        for (int i = 0; i < 6; ++i) acc[21 + i] += J[row][i] * r[row];
    }
}

// one block. PNP: the residual is the reprojection error in pixels (two rows per pair), J = d(proj)/dq [I | -[q]x]
template <bool PNP>
__global__ void __launch_bounds__(FEAT_BLOCK) feat_finish_kernel(int hypotheses, unsigned seed, float min_area, float tau_px, float tau_depth,
                                                                 int refine_iters, int min_matches, int min_inliers, float min_share,
                                                                 float max_translation, float max_rotation, const float* __restrict__ K_b,
                                                                 FeatPoseWs ws, float* __restrict__ T, int* __restrict__ stats)
{
    __shared__ unsigned char flag[FEAT_MAX_SLOTS];
    __shared__ double sums[FEAT_WAVES][FEAT_SUMS];
    __shared__ double pose[12];
    __shared__ float pose32[12];
    __shared__ unsigned upart[FEAT_WAVES];
    __shared__ int ipart[FEAT_WAVES];
    __shared__ int stop;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int M = ws.head[0];
    const float K[4] = {K_b[0], K_b[1], K_b[2], K_b[3]};
    unsigned key = 0u;
    for (int h = tid; h < hypotheses; h += FEAT_BLOCK) key = max(key, (unsigned)ws.hyp[h] << 10 | (unsigned)(FEAT_MAX_HYPOTHESES - 1 - h));
    key = feat_block_max(key, upart);                                  // a count is at most 4096: count << 10 fits; lowest h on a tie
    const int winner = FEAT_MAX_HYPOTHESES - 1 - (int)(key & 1023u), best = (int)(key >> 10);
    FeatRt rt;
    const bool have = best >= 3 && feat_hypothesis<PNP>(seed, winner, M, ws.PA, ws.PB, min_area, rt);
    int final_inliers = 0;
    if (have) {                                                        // uniform over the block
        for (int m = tid; m < M; m += FEAT_BLOCK) flag[m] = feat_inlier<PNP>(rt, ws, m, K, tau_px, tau_depth) ? 1 : 0;
        if (tid == 0) {
            for (int k = 0; k < 9; ++k) pose[k] = (double)rt.R[k];
            for (int i = 0; i < 3; ++i) pose[9 + i] = (double)rt.t[i];
            stop = 0;
        }
        __syncthreads();
        for (int it = 0; it < refine_iters; ++it) {
            double acc[FEAT_SUMS];
#pragma unroll
            for (int k = 0; k < FEAT_SUMS; ++k) acc[k] = 0.0;
            for (int m = tid; m < M; m += FEAT_BLOCK) {
                if (!flag[m]) continue;
                const float* P = ws.PA + 3 * (size_t)m;
                double q[3];
#pragma unroll
                for (int i = 0; i < 3; ++i)
                    q[i] = pose[3 * i] * (double)P[0] + pose[3 * i + 1] * (double)P[1] + pose[3 * i + 2] * (double)P[2] + pose[9 + i];
                if constexpr (PNP) {
                    const float* uv = ws.UV + 2 * (size_t)m;
                    const double fx = (double)K[0], fy = (double)K[1];
                    const double r[2] = {fx * q[0] / q[2] + (double)K[2] - (double)uv[0], fy * q[1] / q[2] + (double)K[3] - (double)uv[1]};
                    const double ax = fx / q[2], ay = fy / q[2], bx = -fx * q[0] / (q[2] * q[2]), by = -fy * q[1] / (q[2] * q[2]);
                    const double J[2][6] = {{ax, 0.0, bx, bx * q[1], ax * q[2] - bx * q[0], -ax * q[1]},
                                            {0.0, ay, by, by * q[1] - ay * q[2], -by * q[0], ay * q[0]}};
                    feat_add_rows<2>(acc, J, r);
                } else {
                    const float* Pb = ws.PB + 3 * (size_t)m;
                    const double r[3] = {q[0] - (double)Pb[0], q[1] - (double)Pb[1], q[2] - (double)Pb[2]};
                    const double J[3][6] = {{1.0, 0.0, 0.0, 0.0, q[2], -q[1]}, {0.0, 1.0, 0.0, -q[2], 0.0, q[0]}, {0.0, 0.0, 1.0, q[1], -q[0], 0.0}};
                    feat_add_rows<3>(acc, J, r);
                }
            }
#pragma unroll
            for (int k = 0; k < FEAT_SUMS; ++k) {
                double v = acc[k];
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
                if (lane == 0) sums[wave][k] = v;
            }
            __syncthreads();
            if (tid == 0) {
                double s[FEAT_SUMS], xi[6];
                for (int k = 0; k < FEAT_SUMS; ++k) {
                    double v = sums[0][k];
                    for (int w = 1; w < FEAT_WAVES; ++w) v += sums[w][k];
                    s[k] = v;
                }
                if (feat_solve6(s, xi)) feat_exp_apply(xi, pose);
                else stop = 1;
            }
            __syncthreads();
            if (stop) break;
        }
        if (tid < 12) pose32[tid] = (float)pose[tid];
        __syncthreads();
        FeatRt fin;
#pragma unroll
        for (int k = 0; k < 9; ++k) fin.R[k] = pose32[k];
#pragma unroll
        for (int i = 0; i < 3; ++i) fin.t[i] = pose32[9 + i];
        int n = 0;
        for (int m = tid; m < M; m += FEAT_BLOCK) n += feat_inlier<PNP>(fin, ws, m, K, tau_px, tau_depth) ? 1 : 0;
        final_inliers = feat_block_sum(n, ipart);
    }
    if (tid != 0) return;
    bool accepted = false;
    if (have) {
        double R[9], t[3];
        bool finite = true;
        for (int k = 0; k < 9; ++k) R[k] = (double)pose32[k], finite = finite && isfinite(pose32[k]);
        for (int i = 0; i < 3; ++i) t[i] = (double)pose32[9 + i], finite = finite && isfinite(pose32[9 + i]);
        const double norm_t = sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]);
        const double ax = R[7] - R[5], ay = R[2] - R[6], az = R[3] - R[1];
        const double angle = atan2(0.5 * sqrt(ax * ax + ay * ay + az * az), 0.5 * (R[0] + R[4] + R[8] - 1.0));
        accepted = finite && M >= min_matches && final_inliers >= min_inliers && (double)final_inliers >= (double)min_share * (double)M &&
                   norm_t <= (double)max_translation && angle <= (double)max_rotation;
    }
    for (int k = 0; k < 16; ++k) T[k] = (k % 5 == 0) ? 1.f : 0.f;
    if (accepted) {
        for (int i = 0; i < 3; ++i) {
            for (int j = 0; j < 3; ++j) T[4 * i + j] = pose32[3 * i + j];
            T[4 * i + 3] = pose32[9 + i];
        }
    }
    stats[3] = winner, stats[4] = best, stats[5] = final_inliers, stats[6] = accepted ? 1 : 0, stats[7] = 0;
}

}  // namespace gsr
