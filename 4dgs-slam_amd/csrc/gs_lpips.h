// gs_lpips.h -- the LPIPS-specific part of the perceptual metric (include/perceptual.h): the input scaling of both images of every pair
// into one network batch, and the distance over the taps of the feature network, in three launches that never leave the device.
// gfx950 / wave64. The convolutions stay with the caller.
//
//   prepare   one thread per value of the [2B, 3, H, W] network batch (renders first, then ground truths): (2 v - 1 - shift) / scale.
//   distance  one wave per 64 pixels of one pair at one tap: a lane owns a pixel and walks the channel axis of the NCHW tensors twice
//             (consecutive lanes read consecutive addresses; the second walk comes from L2). Walk 1: the two sums of squares, in
//             double. Walk 2: sum_c lin[c] (a_c / |a| - b_c / |b|)^2, the difference of the NORMALISED values (taken in double, then
//             float: the square, the weight and every sum are float), never the expanded form
//             sum w a^2 / |a|^2 + sum w b^2 / |b|^2 - 2 sum w a b / (|a| |b|): for a good render the score is a small difference of numbers
//             near sum w, which the expanded form loses to cancellation. The 64 pixel sums are added by a shuffle tree and
//             lane 0 writes one partial per block.
//   finish    one wave per pair: per tap, lane i adds the partials i, i + 64, ... in index order, a shuffle tree adds the lanes, the
//             sum is divided by the tap's pixel count; the taps are added in order. No float atomics anywhere: same bits every run.
//
// Why the norms and the difference are double: with b = a (1 + r n) the difference a / |a| - b / |b| is of size r and perpendicular to
// a / |a|; an error e in |a| relative to |b| adds e a / |a| to it, so e^2 / r^2 to the score, always upwards. Restated on the host with
// the kernel's summation order, a serial float sum of the squares over 384 channels costs 1e-5 of the score at r = 1e-4, and
// normalised values rounded to float before the subtraction 2e-6 at 64 channels; with both in double the score is within 5e-7 of fp64
// on every row of DESIGN.md's table. The walks are bound by their loads, not by the double rate.
// Exactness: walk 2 is compiled with floating-point contraction off (both products rounded, then subtracted), so d(x, x) == 0 and
// d(x, y) and d(y, x) have the same bits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gsr {

constexpr int LPIPS_MAX_LEVELS = 8;
constexpr int LPIPS_BLOCK = 64;                         // one wave: the block's reduction is the wave's
constexpr int LPIPS_PREPARE_BLOCK = 256;
constexpr int LPIPS_NORM_TORCHMETRICS = 0;              // f / sqrt(1e-8 + sum f^2)
constexpr int LPIPS_NORM_LPIPS = 1;                     // f / (sqrt(sum f^2) + 1e-10)

struct LpipsLevels {                                    // passed by value: no table in device memory
    const float* feat[LPIPS_MAX_LEVELS];                // [2B, C, h, w]: rows 0 .. B-1 the first images, B .. 2B-1 the second
    const float* lin[LPIPS_MAX_LEVELS];                 // [C]
    int c[LPIPS_MAX_LEVELS], hw[LPIPS_MAX_LEVELS];
    int blocks[LPIPS_MAX_LEVELS];                       // blocks per pair: ceil(hw / 64)
    int first[LPIPS_MAX_LEVELS + 1];                    // first block (= first partial) of the level; pair b's follow at b * blocks
    int levels;
};

// LPIPS' ScalingLayer, per channel
__device__ __forceinline__ float lpips_shift(int c) { return c == 0 ? -.030f : c == 1 ? -.088f : -.188f; }
__device__ __forceinline__ float lpips_scale(int c) { return c == 0 ? .458f : c == 1 ? .448f : .450f; }

// x, y: [B, 3, H, W] in [0, 1]; out: [2B, 3, H, W]. n = B * 3 * hw values per input.
__global__ void __launch_bounds__(LPIPS_PREPARE_BLOCK) lpips_prepare_kernel(int n, int hw, const float* __restrict__ x,
                                                                            const float* __restrict__ y, float* __restrict__ out)
{
    const int i = blockIdx.x * LPIPS_PREPARE_BLOCK + threadIdx.x;
    if (i >= n) return;
    const int c = (i / hw) % 3;
    const float sh = lpips_shift(c), sc = lpips_scale(c);
    out[i] = __fdiv_rn(__fsub_rn(__fsub_rn(__fmul_rn(2.f, x[i]), 1.f), sh), sc);
    out[(size_t)n + i] = __fdiv_rn(__fsub_rn(__fsub_rn(__fmul_rn(2.f, y[i]), 1.f), sh), sc);
}

__device__ __forceinline__ float lpips_wave_sum(float v)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v = __fadd_rn(v, __shfl_down(v, d, 64));
    return v;                                            // lane 0 holds the sum; one fixed tree
}

// 1 / norm of a feature vector whose squares sum to s, in the chosen published form
__device__ __forceinline__ double lpips_inv_norm(double s, int norm)
{
    return norm == LPIPS_NORM_LPIPS ? 1.0 / (sqrt(s) + 1e-10) : 1.0 / sqrt(1e-8 + s);
}

__global__ void __launch_bounds__(LPIPS_BLOCK) lpips_distance_kernel(const LpipsLevels L, int batch, int norm, float* __restrict__ partial)
{
    const int blk = blockIdx.x;
    int l = 0;
    while (l + 1 < L.levels && blk >= L.first[l + 1]) ++l;
    const int r = blk - L.first[l];
    const int b = r / L.blocks[l], chunk = r - b * L.blocks[l];
    const int C = L.c[l], hw = L.hw[l];
    const int p = chunk * LPIPS_BLOCK + (int)threadIdx.x;
    float v = 0.f;
    if (p < hw) {
        const float* fa = L.feat[l] + (size_t)b * C * hw + p;
        const float* fb = L.feat[l] + (size_t)(batch + b) * C * hw + p;
        const float* w = L.lin[l];
        double sa = 0.0, sb = 0.0;
#pragma unroll 8
        for (int c = 0; c < C; ++c) {
            const double a = (double)fa[(size_t)c * hw], bb = (double)fb[(size_t)c * hw];
            sa = fma(a, a, sa);
            sb = fma(bb, bb, sb);
        }
        const double ia = lpips_inv_norm(sa, norm), ib = lpips_inv_norm(sb, norm);
#pragma unroll 8
        for (int c = 0; c < C; ++c) {
            // contraction off for these statements: a fused a ia - (b ib) rounds one product and not the other, so it is neither 0 for
            // a == b nor antisymmetric (the __dmul_rn / __dsub_rn spellings are plain operators here and contract like them)
#pragma clang fp contract(off)
            const double an = (double)fa[(size_t)c * hw] * ia, bn = (double)fb[(size_t)c * hw] * ib;
            const float d = (float)(an - bn);
            const float d2 = d * d;
            v += w[c] * d2;
        }
    }
    v = lpips_wave_sum(v);
    if (threadIdx.x == 0) partial[blk] = v;
}

// taps: [batch, levels] per-tap means, or NULL; scores: [batch]
__global__ void __launch_bounds__(64) lpips_finish_kernel(const LpipsLevels L, const float* __restrict__ partial, float* __restrict__ taps,
                                                          float* __restrict__ scores)
{
    const int b = blockIdx.x, lane = threadIdx.x;
    float score = 0.f;
    for (int l = 0; l < L.levels; ++l) {
        const float* q = partial + L.first[l] + (size_t)b * L.blocks[l];
        float s = 0.f;
        for (int k = lane; k < L.blocks[l]; k += 64) s = __fadd_rn(s, q[k]);
        s = lpips_wave_sum(s);
        const float mean = __fdiv_rn(s, (float)L.hw[l]);
        if (lane == 0 && taps) taps[b * L.levels + l] = mean;
        score = __fadd_rn(score, mean);
    }
    if (lane == 0) scores[b] = score;
}

}  // namespace gsr
