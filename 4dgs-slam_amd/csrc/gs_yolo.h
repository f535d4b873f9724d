// gs_yolo.h -- post-processing of a YOLO segmentation head (include/segmentation.h): ultralytics' Detect/Segment inference decode,
// non_max_suppression and process_mask (non-retina, logit form), restated as five launches that never leave the device. gfx950 / wave64.
//
//   decode   one thread per anchor: class sigmoid max / argmax, the class-set filter, DFL (softmax over 16 bins, expectation), the
//            anchor-centre box times the level stride, xywh -> xyxy. Writes a per-anchor record (score -1: not a candidate).
//   sort     one block: the candidates compacted in anchor order (wave64 ballots + a prefix over the block's waves, no atomics), then a
//            bitonic sort in LDS on the 64-bit key (score bits, ~anchor): score descending, anchor ascending. The boxes are written in
//            that order, offset by class * 7680 (ultralytics' max_wh) as torchvision.ops.nms sees them.
//   iou      64 x 64 tiles of the suppression bitmask: bit j of row i is set when j > i and IoU(i, j) > iou (torchvision's arithmetic).
//   select   one wave: the greedy pass over the sorted candidates, the removed set spread over the lanes (4 words each); every kept
//            box suppresses, and a kept box is emitted while its class has fewer than max_det detections.
//   masks    one block per 32 x 32 output tile: the proto tile (10 x 10 proto pixels around it) staged in LDS; per detection whose
//            crop box meets the tile, its cropped logits at proto resolution, then bilinear (align_corners=False) to the output
//            pixels, > 0, ORed; finally motion &= ~yolo.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gsr {

constexpr int YOLO_MAX_LEVELS = 4;
constexpr int YOLO_REG_MAX = 16;
constexpr int YOLO_BOX_CH = 4 * YOLO_REG_MAX;          // 64 DFL logits per anchor
constexpr int YOLO_MAX_ANCHORS = 8192;                 // the sort's LDS capacity (64 KiB of keys); 640 x 480 has 6300 anchors
constexpr int YOLO_WORDS = YOLO_MAX_ANCHORS / 64;      // 128 bitmask words per row at most: 2 per lane in the select wave
constexpr int YOLO_MAX_CLASSES = 256;
constexpr int YOLO_MAX_NM = 64;
constexpr int YOLO_DET_HEAD = 7;                        // x1 y1 x2 y2 score class anchor, then nm coefficients
constexpr float YOLO_CLASS_OFFSET = 7680.f;            // ultralytics ops.non_max_suppression max_wh
constexpr int YOLO_SORT_BLOCK = 1024;
constexpr int YOLO_TILE = 32;                           // output tile side of the mask kernel
constexpr int YOLO_PT = YOLO_TILE / 4 + 2;              // proto tile side: 8 cells + one on each side for the bilinear taps

struct YoloLevels {                                     // passed by value: no pointer table in device memory
    const float* head[YOLO_MAX_LEVELS];                 // [64 + nc, h, w]: Detect's cat(cv2, cv3) of the level
    const float* coef[YOLO_MAX_LEVELS];                 // [nm, h, w]: Segment's cv4 of the level
    int h[YOLO_MAX_LEVELS], w[YOLO_MAX_LEVELS], first[YOLO_MAX_LEVELS + 1];
    float stride[YOLO_MAX_LEVELS];
    int levels;
};

struct YoloClassSet {
    uint32_t bits[YOLO_MAX_CLASSES / 32];
};

__device__ __forceinline__ int yolo_level_of(const YoloLevels& L, int a)
{
    int l = 0;
    while (l + 1 < L.levels && a >= L.first[l + 1]) ++l;
    return l;
}

// torch's sigmoid: 1 / (1 + exp(-x)) in float
__device__ __forceinline__ float yolo_sigmoid(float x) { return __fdiv_rn(1.f, __fadd_rn(1.f, expf(-x))); }

__global__ void __launch_bounds__(256) yolo_decode_kernel(const YoloLevels L, int A, int nc, const YoloClassSet cs, float conf,
                                                          float* __restrict__ score, int* __restrict__ cls, float4* __restrict__ box)
{
    const int a = blockIdx.x * 256 + threadIdx.x;
    if (a >= A) return;
    const int l = yolo_level_of(L, a);
    const int w = L.w[l], hw = L.h[l] * w, p = a - L.first[l];
    const float* hd = L.head[l] + p;
    // cls.amax(1) > conf, then (conf, j) = cls.max(1): the first class of the largest sigmoid
    float best = -1.f;
    int j = 0;
    for (int c = 0; c < nc; ++c) {
        const float s = yolo_sigmoid(hd[(size_t)(YOLO_BOX_CH + c) * hw]);
        if (s > best) { best = s; j = c; }
    }
    if (!(best > conf) || !((cs.bits[j >> 5] >> (j & 31)) & 1u)) {
        score[a] = -1.f;
        return;
    }
    float d[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {                      // DFL: x.view(4, 16, a).softmax over the 16 bins, then . arange(16)
        float v[YOLO_REG_MAX], m = -INFINITY;
#pragma unroll
        for (int b = 0; b < YOLO_REG_MAX; ++b) {
            v[b] = hd[(size_t)(k * YOLO_REG_MAX + b) * hw];
            m = fmaxf(m, v[b]);
        }
        float sum = 0.f;
#pragma unroll
        for (int b = 0; b < YOLO_REG_MAX; ++b) {
            v[b] = expf(__fsub_rn(v[b], m));
            sum = __fadd_rn(sum, v[b]);
        }
        float e = 0.f;
#pragma unroll
        for (int b = 1; b < YOLO_REG_MAX; ++b) e = fmaf(__fdiv_rn(v[b], sum), (float)b, e);
        d[k] = e;
    }
    // make_anchors (cell centre + 0.5), dist2bbox(xywh=True) * stride, then non_max_suppression's xywh2xyxy
    const int y = p / w, x = p - y * w;
    const float ax = (float)x + 0.5f, ay = (float)y + 0.5f, st = L.stride[l];
    const float x1 = __fsub_rn(ax, d[0]), y1 = __fsub_rn(ay, d[1]), x2 = __fadd_rn(ax, d[2]), y2 = __fadd_rn(ay, d[3]);
    const float cx = __fmul_rn(__fdiv_rn(__fadd_rn(x1, x2), 2.f), st), cy = __fmul_rn(__fdiv_rn(__fadd_rn(y1, y2), 2.f), st);
    const float bw = __fmul_rn(__fsub_rn(x2, x1), st), bh = __fmul_rn(__fsub_rn(y2, y1), st);
    const float dw = __fdiv_rn(bw, 2.f), dh = __fdiv_rn(bh, 2.f);
    score[a] = best;
    cls[a] = j;
    box[a] = make_float4(__fsub_rn(cx, dw), __fsub_rn(cy, dh), __fadd_rn(cx, dw), __fadd_rn(cy, dh));
}

// n_out[0] = candidates; order[i] = the anchor of sorted position i; obox[i] = its class-offset box
__global__ void __launch_bounds__(YOLO_SORT_BLOCK) yolo_sort_kernel(int A, const float* __restrict__ score, const int* __restrict__ cls,
                                                                    const float4* __restrict__ box, int* __restrict__ order,
                                                                    float4* __restrict__ obox, int* __restrict__ n_out)
{
    __shared__ unsigned long long keys[YOLO_MAX_ANCHORS];
    __shared__ int wave_count[YOLO_SORT_BLOCK / 64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    int base = 0;
    for (int a0 = 0; a0 < A; a0 += YOLO_SORT_BLOCK) {
        const int a = a0 + t;
        const float s = a < A ? score[a] : -1.f;
        const bool f = s > 0.f;
        const unsigned long long ballot = __ballot(f);
        const int below = __builtin_amdgcn_mbcnt_hi((unsigned)(ballot >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)ballot, 0u));
        if (lane == 0) wave_count[wave] = __popcll(ballot);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int q = 0; q < YOLO_SORT_BLOCK / 64; ++q) {
            const int c = wave_count[q];
            before += q < wave ? c : 0;
            total += c;
        }
        if (f) keys[base + before + below] = ((unsigned long long)__float_as_uint(s) << 32) | (unsigned long long)(0xffffffffu - (unsigned)a);
        base += total;
        __syncthreads();
    }
    const int n = base;
    int n2 = 1;
    while (n2 < n) n2 <<= 1;
    for (int i = n + t; i < n2; i += YOLO_SORT_BLOCK) keys[i] = 0ull;      // below every candidate's key (scores are > 0)
    __syncthreads();
    for (int k = 2; k <= n2; k <<= 1)
        for (int jj = k >> 1; jj > 0; jj >>= 1) {
            for (int i = t; i < n2; i += YOLO_SORT_BLOCK) {
                const int ixj = i ^ jj;
                if (ixj > i) {
                    const unsigned long long u = keys[i], v = keys[ixj];
                    if ((i & k) == 0 ? u < v : u > v) {              // descending runs where (i & k) == 0: the whole array descends
                        keys[i] = v;
                        keys[ixj] = u;
                    }
                }
            }
            __syncthreads();
        }
    for (int i = t; i < n; i += YOLO_SORT_BLOCK) {
        const int a = (int)(0xffffffffu - (unsigned)(keys[i] & 0xffffffffull));
        const float off = __fmul_rn((float)cls[a], YOLO_CLASS_OFFSET);
        const float4 b = box[a];
        order[i] = a;
        obox[i] = make_float4(__fadd_rn(b.x, off), __fadd_rn(b.y, off), __fadd_rn(b.z, off), __fadd_rn(b.w, off));
    }
    if (t == 0) n_out[0] = n;
}

// torchvision's devIoU (float, no contraction)
__device__ __forceinline__ bool yolo_iou_above(float4 a, float4 b, float thr)
{
    const float left = fmaxf(a.x, b.x), right = fminf(a.z, b.z), top = fmaxf(a.y, b.y), bottom = fminf(a.w, b.w);
    const float width = fmaxf(__fsub_rn(right, left), 0.f), height = fmaxf(__fsub_rn(bottom, top), 0.f);
    const float inter = __fmul_rn(width, height);
    const float sa = __fmul_rn(__fsub_rn(a.z, a.x), __fsub_rn(a.w, a.y)), sb = __fmul_rn(__fsub_rn(b.z, b.x), __fsub_rn(b.w, b.y));
    return __fdiv_rn(inter, __fsub_rn(__fadd_rn(sa, sb), inter)) > thr;
}

// grid (column block, row block) of 64 x 64; mask row i holds `words` words, of which the select pass reads those >= i / 64 only
__global__ void __launch_bounds__(64) yolo_iou_kernel(const int* __restrict__ n_ptr, const float4* __restrict__ obox, float thr, int words,
                                                      unsigned long long* __restrict__ mask)
{
    const int n = n_ptr[0];
    const int rb = blockIdx.y, cb = blockIdx.x, t = threadIdx.x;
    if (cb < rb || rb * 64 >= n || cb * 64 >= n) return;
    __shared__ float4 cols[64];
    const int j0 = cb * 64;
    if (j0 + t < n) cols[t] = obox[j0 + t];
    __syncthreads();
    const int i = rb * 64 + t;
    if (i >= n) return;
    const float4 bi = obox[i];
    const int jn = min(64, n - j0);
    unsigned long long bits = 0ull;
    for (int q = (cb == rb ? t + 1 : 0); q < jn; ++q)
        if (yolo_iou_above(bi, cols[q], thr)) bits |= 1ull << q;
    mask[(size_t)i * words + cb] = bits;
}

__device__ __forceinline__ unsigned long long yolo_readlane64(unsigned long long v, int lane)
{
    const unsigned lo = __builtin_amdgcn_readlane((unsigned)v, lane), hi = __builtin_amdgcn_readlane((unsigned)(v >> 32), lane);
    return ((unsigned long long)hi << 32) | lo;
}

// one wave. counts[0] = detections emitted, counts[1] = candidates, counts[2] = boxes NMS kept (before max_det)
__global__ void __launch_bounds__(64) yolo_select_kernel(const YoloLevels L, const int* __restrict__ n_ptr, const int* __restrict__ order,
                                                         const float* __restrict__ score, const int* __restrict__ cls,
                                                         const float4* __restrict__ box, const unsigned long long* __restrict__ mask,
                                                         int words, int nc, int nm, int max_det, int max_dets, float* __restrict__ dets,
                                                         int* __restrict__ counts)
{
    __shared__ int per_class[YOLO_MAX_CLASSES];
    const int lane = threadIdx.x;
    for (int c = lane; c < nc; c += 64) per_class[c] = 0;
    __syncthreads();
    const int n = n_ptr[0];
    const int nw = (n + 63) >> 6;
    unsigned long long removed0 = 0ull, removed1 = 0ull;          // words lane and 64 + lane
    int kept = 0, emitted = 0;
    const int rec = YOLO_DET_HEAD + nm;
    for (int i = 0; i < n; ++i) {
        const int w = i >> 6;
        const unsigned long long word = yolo_readlane64(w < 64 ? removed0 : removed1, w & 63);
        if ((word >> (i & 63)) & 1ull) continue;
        ++kept;
        const int a = order[i];
        const int c = cls[a];
        const int have = per_class[c];
        if (have < max_det && emitted < max_dets) {
            float* o = dets + (size_t)emitted * rec;
            const int l = yolo_level_of(L, a);
            const int hw = L.h[l] * L.w[l], p = a - L.first[l];
            for (int q = lane; q < rec; q += 64) {
                float v;
                if (q >= YOLO_DET_HEAD) v = L.coef[l][(size_t)(q - YOLO_DET_HEAD) * hw + p];
                else if (q < 4) { const float4 b = box[a]; v = q == 0 ? b.x : q == 1 ? b.y : q == 2 ? b.z : b.w; }
                else v = q == 4 ? score[a] : q == 5 ? (float)c : (float)a;
                o[q] = v;
            }
            ++emitted;
            __syncthreads();                                       // every lane has read per_class[c] before it changes
            if (lane == 0) per_class[c] = have + 1;
            __syncthreads();
        }
        const unsigned long long* row = mask + (size_t)i * words;
        if (lane >= w && lane < nw) removed0 |= row[lane];
        if (64 + lane >= w && 64 + lane < nw) removed1 |= row[64 + lane];
    }
    if (lane == 0) {
        counts[0] = emitted;
        counts[1] = n;
        counts[2] = kept;
    }
}

// PyTorch's upsample_bilinear2d source index (align_corners=False): src = scale (dst + 0.5) - 0.5, clamped at 0
__device__ __forceinline__ void yolo_src_index(float scale, int dst, int in_size, int& i0, int& i1, float& l0, float& l1)
{
    float src = __fsub_rn(__fmul_rn(scale, __fadd_rn((float)dst, 0.5f)), 0.5f);
    src = src < 0.f ? 0.f : src;
    i0 = (int)src;
    i1 = i0 + (i0 < in_size - 1 ? 1 : 0);
    l1 = __fsub_rn(src, (float)i0);
    l0 = __fsub_rn(1.f, l1);
}

// one block per 32 x 32 output tile; proto [nm, ph, pw] with H = 4 ph, W = 4 pw; dets rows of YOLO_DET_HEAD + nm floats
__global__ void __launch_bounds__(256) yolo_mask_kernel(const int* __restrict__ counts, int max_dets, const float* __restrict__ dets, int nm,
                                                        const float* __restrict__ proto, int ph, int pw, int H, int W,
                                                        unsigned char* __restrict__ yolo, unsigned char* __restrict__ motion)
{
    __shared__ float sp[YOLO_MAX_NM * YOLO_PT * YOLO_PT];
    __shared__ float logit[YOLO_PT * YOLO_PT];
    const int t = threadIdx.x;
    const int X0 = blockIdx.x * YOLO_TILE, Y0 = blockIdx.y * YOLO_TILE;
    const float sy = __fdiv_rn((float)ph, (float)H), sx = __fdiv_rn((float)pw, (float)W);
    int r_lo, c_lo, r_hi, c_hi, dummy;
    float fd0, fd1;
    yolo_src_index(sy, Y0, ph, r_lo, dummy, fd0, fd1);
    yolo_src_index(sx, X0, pw, c_lo, dummy, fd0, fd1);
    yolo_src_index(sy, min(Y0 + YOLO_TILE, H) - 1, ph, dummy, r_hi, fd0, fd1);
    yolo_src_index(sx, min(X0 + YOLO_TILE, W) - 1, pw, dummy, c_hi, fd0, fd1);
    const int psz = ph * pw;
    for (int q = t; q < nm * YOLO_PT * YOLO_PT; q += 256) {
        const int m = q / (YOLO_PT * YOLO_PT), rc = q - m * (YOLO_PT * YOLO_PT), rr = rc / YOLO_PT, cc = rc - rr * YOLO_PT;
        const int r = r_lo + rr, c = c_lo + cc;
        sp[q] = (r <= r_hi && c <= c_hi) ? proto[(size_t)m * psz + r * pw + c] : 0.f;
    }
    // the 4 output pixels of this thread: tile row t / 32 + 8 k, column t % 32
    int i0[4], i1[4];
    float a0[4], a1[4];
    const int X = X0 + (t & 31);
    int j0, j1;
    float b0, b1;
    yolo_src_index(sx, X, pw, j0, j1, b0, b1);
    j0 -= c_lo;
    j1 -= c_lo;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        yolo_src_index(sy, Y0 + (t >> 5) + 8 * k, ph, i0[k], i1[k], a0[k], a1[k]);
        i0[k] -= r_lo;
        i1[k] -= r_lo;
    }
    bool hit[4] = {false, false, false, false};
    const int n = min(counts[0], max_dets);
    const int rec = YOLO_DET_HEAD + nm;
    __syncthreads();
    for (int d = 0; d < n; ++d) {
        const float* dr = dets + (size_t)d * rec;
        // process_mask: the box scaled by (pw / W, ph / H); proto pixel (row r, column c) kept iff x1 <= c < x2 and y1 <= r < y2
        const float bx1 = __fmul_rn(dr[0], sx), by1 = __fmul_rn(dr[1], sy), bx2 = __fmul_rn(dr[2], sx), by2 = __fmul_rn(dr[3], sy);
        const float cmin = fmaxf((float)c_lo, ceilf(bx1)), rmin = fmaxf((float)r_lo, ceilf(by1));
        if (!(cmin < bx2 && cmin <= (float)c_hi && rmin < by2 && rmin <= (float)r_hi)) continue;     // every logit of the tile is 0
        if (t < YOLO_PT * YOLO_PT) {
            const int rr = t / YOLO_PT, cc = t - rr * YOLO_PT;
            const float r = (float)(r_lo + rr), c = (float)(c_lo + cc);
            float v = 0.f;
            if (c >= bx1 && c < bx2 && r >= by1 && r < by2)
                for (int m = 0; m < nm; ++m) v = fmaf(dr[YOLO_DET_HEAD + m], sp[m * YOLO_PT * YOLO_PT + t], v);
            logit[t] = v;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float* r0 = logit + i0[k] * YOLO_PT;
            const float* r1 = logit + i1[k] * YOLO_PT;
            const float v = __fadd_rn(__fmul_rn(a0[k], __fadd_rn(__fmul_rn(b0, r0[j0]), __fmul_rn(b1, r0[j1]))),
                                      __fmul_rn(a1[k], __fadd_rn(__fmul_rn(b0, r1[j0]), __fmul_rn(b1, r1[j1]))));
            hit[k] = hit[k] || v > 0.f;
        }
        __syncthreads();
    }
    if (X >= W) return;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int Y = Y0 + (t >> 5) + 8 * k;
        if (Y >= H) continue;
        const size_t o = (size_t)Y * W + X;
        if (yolo) yolo[o] = hit[k] ? 1 : 0;
        if (motion && hit[k]) motion[o] = 0;
    }
}

}  // namespace gsr
