// gs_sweep.h -- the plane sweep of include/multiview_depth.h: a census cost over 64 inverse-depth hypotheses against up to four partner
// views, the stereo matcher's eight-path aggregation on that cost, selection and depth. gfx950 / wave64, no atomics, no LDS, no scratch.
// The census codes come from stereo_census_kernel (gs_stereo.h), and so do the wave shifts and the butterfly minimum of the path step.
//
// Layout. The hypotheses of one pixel are the lanes of one wave, as the disparities are in gs_stereo.h: a pixel's row of C (uint8
// [H, W, 64]) is one 64-byte line, its row of S (uint16 [H, W, 64]) one 128-byte line.
//   sweep_cost_kernel     one wave per pixel, lane = hypothesis k. The ray and the reference code are wave-uniform; per partner a lane
//                         does one projection (single rounded float32 operations, the header's order), one 8-byte gather of the
//                         partner's code and one 64-bit popcount. Neighbouring lanes land on neighbouring pixels of the epipolar line. The
//                         observability flag is read off lanes 0 and 63 (their depth in the partner and their projections).
//   sweep_path_kernel     stereo_path_kernel<1>'s recurrence with C loaded from the byte volume instead of formed from two codes: one wave
//                         per path, L_r of the previous pixel in a register, four steps' loads ahead of their dependent arithmetic.
//   sweep_select_kernel   one wave per pixel: first-minimum argmin as a keyed minimum, the uniqueness scan as a ballot, the sub-hypothesis
//                         parabola step and the depth.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "gs_stereo.h"

namespace gsr {

constexpr int SWEEP_D = 64;                 // hypotheses: the lanes of a wave
constexpr int SWEEP_MAX_PARTNERS = 4;
constexpr int SWEEP_INVISIBLE = 62;         // the cost of a hypothesis a partner does not see: every census bit differs

struct SweepCamera { float fx, fy, cx, cy, w_min, w_step; };

// One wave per pixel; blockDim.x = STEREO_BLOCK (four pixels per block). codes: [1 + J, H, W], the reference's first. transforms: [J, 12].
__global__ void __launch_bounds__(STEREO_BLOCK) sweep_cost_kernel(int W, int H, int J, SweepCamera cam, int min_span_px,
                                                                  const uint64_t* __restrict__ codes, const float* __restrict__ transforms,
                                                                  unsigned char* __restrict__ cost, unsigned char* __restrict__ observable)
{
    // contraction off for the whole body: a * b + c would otherwise become one fma, which rounds once where the header rounds twice. Plain
    // operators, not the __fmul_rn / __fadd_rn spellings: those are inline functions around the same operators, compiled outside this
    // pragma's reach, and contract all the same.
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const size_t n = (size_t)W * H;
    const size_t p = (size_t)blockIdx.x * (STEREO_BLOCK / 64) + (threadIdx.x >> 6);
    if (p >= n) return;                                               // wave-uniform
    const int v = (int)(p / W), u = (int)(p - (size_t)v * W);
    const float rx = ((float)u - cam.cx) / cam.fx, ry = ((float)v - cam.cy) / cam.fy;
    const float w = cam.w_min + (float)lane * cam.w_step;
    const float u_end = (float)W - 0.5f, v_end = (float)H - 0.5f;
    const uint64_t code = codes[p];
    int c = 0;
    bool seen = false;
    for (int j = 0; j < J; ++j) {                                     // wave-uniform
        const float* T = transforms + 12 * j;
        float X[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const float a = (T[4 * i] * rx + T[4 * i + 1] * ry) + T[4 * i + 2];
            X[i] = a + T[4 * i + 3] * w;
        }
        const float up = cam.fx * (X[0] / X[2]) + cam.cx;
        const float vp = cam.fy * (X[1] / X[2]) + cam.cy;
        // (every comparison is false on a NaN: an overflowing transform makes the hypothesis invisible)
        const bool visible = X[2] > 1e-6f && up >= -0.5f && up < u_end && vp >= -0.5f && vp < v_end;
        // up + 0.5 lies in [0, W) and cannot round up to W (the sum is below W and at least as finely spaced as W - 0.5 is): the clamp
        // only keeps the address inside the image whatever the arithmetic does
        const int xq = visible ? min(max((int)floorf(up + 0.5f), 0), W - 1) : 0;
        const int yq = visible ? min(max((int)floorf(vp + 0.5f), 0), H - 1) : 0;
        const uint64_t other = codes[(size_t)(j + 1) * n + (size_t)yq * W + xq];
        c += visible ? __popcll(code ^ other) : SWEEP_INVISIBLE;
        // observability: both ends of the swept range in front of this partner, and their projections (inside the image or not) far enough apart
        const unsigned long long front = __ballot(X[2] > 1e-6f);
        const float up0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(up), 0));
        const float up1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(up), 63));
        const float vp0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(vp), 0));
        const float vp1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(vp), 63));
        const float du = fabsf(up1 - up0), dv = fabsf(vp1 - vp0);
        const float span = du > dv ? du : dv;                         // (a NaN in du yields dv, a NaN in dv yields itself and fails the test)
        seen |= (front & 1ull) && (front >> 63) && truncf(span) >= (float)min_span_px;
    }
    cost[p * SWEEP_D + lane] = (unsigned char)c;                      // <= 4 * 62
    if (lane == 0) observable[p] = seen ? 1 : 0;
}

// One wave per path of direction (dx, dy); gridDim.x = number of paths (H, W or W + H - 1), blockDim.x = 64. The walk and the step are
// stereo_path_kernel<1>'s.
__global__ void __launch_bounds__(64) sweep_path_kernel(int W, int H, int dx, int dy, int p1, int p2, const unsigned char* __restrict__ C,
                                                        unsigned short* S, int first)
{
    constexpr int U = STEREO_PATH_UNROLL;
    const int lane = threadIdx.x;
    const int path = blockIdx.x;
    int x0, y0;
    if (dy == 0) { x0 = dx > 0 ? 0 : W - 1; y0 = path; }                                  // H row paths
    else if (path < W) { x0 = path; y0 = dy > 0 ? 0 : H - 1; }                            // W paths from the first row in walking order
    else { x0 = dx > 0 ? 0 : W - 1; y0 = dy > 0 ? path - W + 1 : H - 2 - (path - W); }    // H - 1 diagonal paths from the side border
    int n = 0x7fffffff;                                                                   // pixels on the path
    if (dx) n = min(n, dx > 0 ? W - x0 : x0 + 1);
    if (dy) n = min(n, dy > 0 ? H - y0 : y0 + 1);
    int Lp = 0, m = 0;
    for (int k0 = 0; k0 < n; k0 += U) {
        int c[U], s[U];
#pragma unroll
        for (int j = 0; j < U; ++j) {
            if (k0 + j >= n) continue;                                                    // wave-uniform
            const size_t p = (size_t)(y0 + (k0 + j) * dy) * W + (x0 + (k0 + j) * dx);
            c[j] = C[p * SWEEP_D + lane];
            s[j] = first ? 0 : S[p * SWEEP_D + lane];
        }
#pragma unroll
        for (int j = 0; j < U; ++j) {
            if (k0 + j >= n) continue;
            const size_t p = (size_t)(y0 + (k0 + j) * dy) * W + (x0 + (k0 + j) * dx);
            int L = c[j];
            if (k0 + j > 0) L += min(min(Lp, m + p2), min(stereo_from_lane_below(Lp), stereo_from_lane_above(Lp)) + p1) - m;
            Lp = L;
            m = stereo_wave_min(L);
            S[p * SWEEP_D + lane] = (unsigned short)(s[j] + L);
        }
    }
}

// One wave per pixel; blockDim.x = STEREO_BLOCK (four pixels per block).
__global__ void __launch_bounds__(STEREO_BLOCK) sweep_select_kernel(int W, int H, int uniqueness_ratio, float w_min, float w_step,
                                                                    const unsigned short* __restrict__ S,
                                                                    const unsigned char* __restrict__ observable, short* __restrict__ index16,
                                                                    float* __restrict__ depth)
{
#pragma clang fp contract(off)                                        // the depth: plain operators, each rounded (see sweep_cost_kernel)
    const int lane = threadIdx.x & 63;
    const size_t p = (size_t)blockIdx.x * (STEREO_BLOCK / 64) + (threadIdx.x >> 6);
    if (p >= (size_t)W * H) return;                                   // wave-uniform
    const unsigned short* row = S + p * SWEEP_D;
    const int s = row[lane];
    const unsigned key = stereo_wave_min_key(((unsigned)s << 8) | (unsigned)lane);
    const int best = (int)(key & 255u), smin = (int)(key >> 8);
    const bool rival = (lane < best - 1 || lane > best + 1) && s * (100 - uniqueness_ratio) < smin * 100;       // S <= 18360: fits 32 bits
    const bool valid = !__any(rival) && best > 0 && best < SWEEP_D - 1 && observable[p] != 0;                   // wave-uniform
    if (lane != 0) return;
    int out = -16;
    if (valid) {
        const int a = row[best - 1], b = row[best + 1];
        const int den = max(a + b - 2 * smin, 1);
        out = 16 * best + ((a - b) * 16 + den) / (2 * den);           // C's truncating division
    }
    index16[p] = (short)out;
    depth[p] = out >= 0 ? 1.0f / (w_min + ((float)out / 16.0f) * w_step) : 0.0f;
}

}  // namespace gsr
