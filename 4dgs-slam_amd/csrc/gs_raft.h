// gs_raft.h -- the RAFT-specific hot path of the optical-flow estimator (include/optical_flow.h): the all-pairs correlation volume in
// both directions and its 4-level pyramid, the 9x9 window lookup of CorrBlock.__call__ (grid_sample, align_corners=True, zeros), and
// the convex upsampling of RAFT.upsample_flow with the unpad crop and the NDC scaling in its epilogue. gfx950 / wave64.
//
// corr: C[p1, p2] = <f1[:, p1], f2[:, p2]> / sqrt(D) on v_mfma_f32_16x16x4_f32 (f32 in, f32 accumulate: exact f32 products, the sum
// of each element always reduced over k in the same order). A block owns a 64 x 64 tile of C and writes it to the 1->2 volume and,
// transposed, to the 2->1 volume, so the two are bitwise transposes of each other and a single-direction call writes the same bits.
// pool: one launch per pyramid level (both directions in one grid), avg_pool2d(2, 2) of the previous level with floor sizes.
#pragma once
#include <hip/hip_runtime.h>

namespace gsr {

constexpr int RAFT_LEVELS = 4;
constexpr int RAFT_RADIUS = 4;
constexpr int RAFT_WIN = 2 * RAFT_RADIUS + 1;                        // 9
constexpr int RAFT_CORR_CH = RAFT_LEVELS * RAFT_WIN * RAFT_WIN;     // 324
constexpr int RAFT_MASK_CH = 9 * 64;                                 // 576

constexpr int CORR_TILE = 64;        // a block's tile of C: 64 p1 x 64 p2, four waves of 32 x 32 (2 x 2 MFMA 16 x 16 blocks each)
constexpr int CORR_KC = 16;          // k rows staged in LDS per step
constexpr int CORR_LDS_STRIDE = CORR_TILE + 16;   // +16 floats: the four k rows one MFMA operand read touches land on disjoint banks
constexpr int CORR_BLOCK = 256;

typedef float corr_f32x4 __attribute__((ext_vector_type(4)));

// f1, f2: [D, N] (the fmaps [D, h, w] with N = h * w). c12: [N, N] row p1; c21: [N, N] row p2 (NULL: one direction only).
__global__ void __launch_bounds__(CORR_BLOCK) raft_corr_kernel(int D, int N, const float* __restrict__ f1, const float* __restrict__ f2,
                                                               float* __restrict__ c12, float* __restrict__ c21)
{
    __shared__ float sA[CORR_KC * CORR_LDS_STRIDE];
    __shared__ float sB[CORR_KC * CORR_LDS_STRIDE];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int i0 = blockIdx.y * CORR_TILE, j0 = blockIdx.x * CORR_TILE;
    const int wr = (wave >> 1) * 32, wc = (wave & 1) * 32;
    corr_f32x4 acc[2][2];
    for (int a = 0; a < 2; ++a)
        for (int b = 0; b < 2; ++b) acc[a][b] = corr_f32x4{0.f, 0.f, 0.f, 0.f};
    // staging: thread t loads k row t / 16 of the chunk, columns 4 (t % 16) .. +3 of both tiles (zero outside [0, N) and [0, D))
    const int lk = t >> 4, lc = (t & 15) * 4;
    for (int k0 = 0; k0 < D; k0 += CORR_KC) {
        const int k = k0 + lk;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int i = i0 + lc + q, j = j0 + lc + q;
            sA[lk * CORR_LDS_STRIDE + lc + q] = (k < D && i < N) ? f1[(size_t)k * N + i] : 0.f;
            sB[lk * CORR_LDS_STRIDE + lc + q] = (k < D && j < N) ? f2[(size_t)k * N + j] : 0.f;
        }
        __syncthreads();
        // 16x16x4 operand map: lane l holds A[row l & 15][k l >> 4] and B[k l >> 4][col l & 15]
#pragma unroll
        for (int s = 0; s < CORR_KC / 4; ++s) {
            const int kr = (4 * s + (lane >> 4)) * CORR_LDS_STRIDE;
            float a[2], b[2];
#pragma unroll
            for (int m = 0; m < 2; ++m) {
                a[m] = sA[kr + wr + 16 * m + (lane & 15)];
                b[m] = sB[kr + wc + 16 * m + (lane & 15)];
            }
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int n = 0; n < 2; ++n) acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[m], b[n], acc[m][n], 0, 0, 0);
        }
        __syncthreads();
    }
    // C/D map: col = lane & 15, row = 4 (lane >> 4) + r
    const float rs = sqrtf((float)D);
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n) {
            const int j = j0 + wc + 16 * n + (lane & 15);
            const int ib = i0 + wr + 16 * m + 4 * (lane >> 4);
            if (j >= N) continue;
            float v[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = __fdiv_rn(acc[m][n][r], rs);
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (ib + r < N) c12[(size_t)(ib + r) * N + j] = v[r];
            if (c21) {
                float* row = c21 + (size_t)j * N;
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (ib + r < N) row[ib + r] = v[r];
            }
        }
}

// one pyramid level of both directions: dst[d][n] = avg_pool2d(src[d][n], 2, 2) for n < rows; src [rows, hp, wp], dst [rows, hp/2, wp/2]
// (torch's order: ((a + b) + c) + d over the window row by row, then / 4)
__global__ void __launch_bounds__(256) raft_pool_kernel(int rows, int hp, int wp, const float* __restrict__ s0, float* __restrict__ d0,
                                                        const float* __restrict__ s1, float* __restrict__ d1)
{
    const int hc = hp >> 1, wc = wp >> 1;
    const size_t per = (size_t)hc * wc;
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= per * rows) return;
    const float* src = blockIdx.y ? s1 : s0;
    float* dst = blockIdx.y ? d1 : d0;
    const size_t n = idx / per;
    const int cell = (int)(idx - n * per);
    const int y = cell / wc, x = cell - y * wc;
    const float* p = src + n * hp * wp + (size_t)(2 * y) * wp + 2 * x;
    float s = __fadd_rn(p[0], p[1]);
    s = __fadd_rn(s, p[wp]);
    s = __fadd_rn(s, p[wp + 1]);
    dst[idx] = __fdiv_rn(s, 4.f);
}

constexpr int RAFT_MAX_BATCH = 2;     // a lookup serves at most the two directions of one pair
struct RaftPyramids {                  // passed by value: no pointer table in device memory
    const float* level[RAFT_MAX_BATCH][RAFT_LEVELS];
};

// CorrBlock.__call__ + bilinear_sampler: out[b][l*81 + a*9 + c][p] = sample of level l of batch b's volume (row p, [hl, wl]) at
// x = coords[b][0][p] / 2^l + (a - 4), y = coords[b][1][p] / 2^l + (c - 4): the offset of the FIRST window axis goes to x (torch.meshgrid(dy,
// dx) stacked as (x, y)). The coordinate takes bilinear_sampler's round trip through [-1, 1] in torch's GPU arithmetic: x * 2 times the
// float reciprocal of (W - 1), minus 1 (one fma, as the compiled elementwise kernel contracts it); then grid_sample's ((g + 1) / 2) * (W - 1).
// Taps outside the level are 0; the four taps are accumulated into 0 with fma in grid_sample's order (nw, ne, sw, se).
__global__ void __launch_bounds__(256) raft_lookup_kernel(int h, int w, const RaftPyramids pyr, const float* __restrict__ coords,
                                                          float* __restrict__ out)
{
    const int N = h * w;
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= N) return;
    const int l = blockIdx.y, b = blockIdx.z;
    int hl = h, wl = w;
    for (int q = 0; q < l; ++q) { hl >>= 1; wl >>= 1; }
    const float* vol = pyr.level[b][l] + (size_t)p * hl * wl;
    const float* cb = coords + (size_t)b * 2 * N;
    const float inv_l = 1.f / (float)(1 << l);               // exact: the division by 2^l
    const float cx = __fmul_rn(cb[p], inv_l), cy = __fmul_rn(cb[N + p], inv_l);
    const float rx = __fdiv_rn(1.f, (float)(wl - 1)), ry = __fdiv_rn(1.f, (float)(hl - 1));
    const float sx = (float)(wl - 1), sy = (float)(hl - 1);
    float* o = out + ((size_t)b * RAFT_CORR_CH + (size_t)l * RAFT_WIN * RAFT_WIN) * N + p;
    float iys[RAFT_WIN];
#pragma unroll
    for (int c = 0; c < RAFT_WIN; ++c) {
        const float y = __fadd_rn(cy, (float)(c - RAFT_RADIUS));
        const float g = fmaf(__fmul_rn(2.f, y), ry, -1.f);
        iys[c] = __fmul_rn(__fmul_rn(__fadd_rn(g, 1.f), 0.5f), sy);
    }
    for (int a = 0; a < RAFT_WIN; ++a) {
        const float x = __fadd_rn(cx, (float)(a - RAFT_RADIUS));
        const float gx = fmaf(__fmul_rn(2.f, x), rx, -1.f);
        const float ix = __fmul_rn(__fmul_rn(__fadd_rn(gx, 1.f), 0.5f), sx);
        const bool xin = ix > -2.f && ix < (float)wl + 1.f;       // otherwise (NaN included) every tap is outside
        const float fx = floorf(xin ? ix : 0.f);
        const int x0 = (int)fx;
#pragma unroll
        for (int c = 0; c < RAFT_WIN; ++c) {
            const float iy = iys[c];
            float v = 0.f;
            if (xin && iy > -2.f && iy < (float)hl + 1.f) {
                const float fy = floorf(iy);
                const int y0 = (int)fy;
                const float e = __fadd_rn(fx, 1.f), s = __fadd_rn(fy, 1.f);
                const float nw = __fmul_rn(__fsub_rn(e, ix), __fsub_rn(s, iy));
                const float ne = __fmul_rn(__fsub_rn(ix, fx), __fsub_rn(s, iy));
                const float sw = __fmul_rn(__fsub_rn(e, ix), __fsub_rn(iy, fy));
                const float se = __fmul_rn(__fsub_rn(ix, fx), __fsub_rn(iy, fy));
                const bool x0in = x0 >= 0 && x0 < wl, x1in = x0 + 1 >= 0 && x0 + 1 < wl;
                const bool y0in = y0 >= 0 && y0 < hl, y1in = y0 + 1 >= 0 && y0 + 1 < hl;
                if (y0in && x0in) v = fmaf(vol[y0 * wl + x0], nw, v);
                if (y0in && x1in) v = fmaf(vol[y0 * wl + x0 + 1], ne, v);
                if (y1in && x0in) v = fmaf(vol[(y0 + 1) * wl + x0], sw, v);
                if (y1in && x1in) v = fmaf(vol[(y0 + 1) * wl + x0 + 1], se, v);
            }
            o[(size_t)(a * RAFT_WIN + c) * N] = v;
        }
    }
}

// RAFT.upsample_flow + InputPadder.unpad + camera_utils' NDC scaling, one thread per output pixel (X, Y) of batch b:
//   padded pixel (Xp, Yp) = (X + pad_left, Y + pad_top); cell (x, y) = (Xp / 8, Yp / 8); sub-pixel (dx, dy) = (Xp % 8, Yp % 8)
//   m_k = mask[b][k * 64 + dy * 8 + dx][y][x], k = 3 ky + kx;  w = softmax_k(m)
//   up_c = sum_k w_k * 8 flow[b][c][y + ky - 1][x + kx - 1]   (0 outside the low-res grid: unfold's zero padding)
//   out[b][Y][X][c] = ndc ? up_c / (out_w, out_h)[c] * 2 : up_c
__global__ void __launch_bounds__(256) raft_upsample_kernel(int h, int w, const float* __restrict__ flow, const float* __restrict__ mask,
                                                            int pad_left, int pad_top, int out_w, int out_h, int ndc, float* __restrict__ out)
{
    const int X = blockIdx.x * 256 + threadIdx.x, Y = blockIdx.y, b = blockIdx.z;
    if (X >= out_w) return;
    const int N = h * w;
    const int Xp = X + pad_left, Yp = Y + pad_top;
    const int x = Xp >> 3, y = Yp >> 3, dx = Xp & 7, dy = Yp & 7;
    const float* mb = mask + (size_t)b * RAFT_MASK_CH * N + (size_t)(dy * 8 + dx) * N + (size_t)y * w + x;
    float m[9];
    float mx = -INFINITY;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        m[k] = mb[(size_t)k * 64 * N];
        mx = fmaxf(mx, m[k]);
    }
    float sum = 0.f;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        m[k] = expf(__fsub_rn(m[k], mx));
        sum = __fadd_rn(sum, m[k]);
    }
    const float* fb = flow + (size_t)b * 2 * N;
    float up[2] = {0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const int yy = y + k / 3 - 1, xx = x + k % 3 - 1;
        const float wk = __fdiv_rn(m[k], sum);
        if (yy >= 0 && yy < h && xx >= 0 && xx < w) {
            up[0] = __fadd_rn(up[0], __fmul_rn(wk, __fmul_rn(8.f, fb[yy * w + xx])));
            up[1] = __fadd_rn(up[1], __fmul_rn(wk, __fmul_rn(8.f, fb[N + yy * w + xx])));
        }
    }
    if (ndc) {
        up[0] = __fmul_rn(__fdiv_rn(up[0], (float)out_w), 2.f);
        up[1] = __fmul_rn(__fdiv_rn(up[1], (float)out_h), 2.f);
    }
    reinterpret_cast<float2*>(out)[((size_t)b * out_h + Y) * out_w + X] = make_float2(up[0], up[1]);
}

}  // namespace gsr
