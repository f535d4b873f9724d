// gs_stereo.h -- the on-device stereo matcher of include/stereo_depth.h: rectification, census, eight-path semi-global aggregation,
// selection and depth. gfx950 / wave64, integer arithmetic throughout the matching, no atomics, no LDS, no scratch.
//
// Layout. The disparities of one pixel are the lanes of one wave: lane l holds d = l (D = 64) or d = 2 l, 2 l + 1 (D = 128, DPL = 2), so
// a pixel's row of S (uint16 [H, W, D]) is one 128- or 256-byte line that a wave loads and stores as one 2- or 4-byte access per lane.
//   stereo_path_kernel     one wave per PATH of one direction (a maximal run of pixels along r inside the image: H row paths, W column
//                          paths, W + H - 1 diagonal ones -- a diagonal that leaves through a side border ends there and the pixel that has
//                          no predecessor starts a new one). The previous pixel's L_r stays in a register; the neighbours d - 1 / d + 1
//                          come from a one-lane wave shift (DPP wave_shr:1 / wave_shl:1, bound_ctrl off: the edge lane keeps `old`, a
//                          large value, which IS the absent term), m is a six-step butterfly minimum (lane_xor_value, VALU only).
//                          C is never stored: it is one xor and one 64-bit popcount of the two census codes. The loads of a step (the
//                          census codes and S) do not depend on the recurrence, so four steps' loads are issued before the four steps'
//                          dependent arithmetic. The eight directions are eight launches in stream order; the first stores S, the
//                          others add to it, each pixel owned by exactly one wave per launch.
//   stereo_select_kernel   one wave per pixel: first-minimum argmin as a minimum of (S << 8 | d) keys, the uniqueness scan as a ballot,
//                          dR as a second keyed minimum over the diagonal read S(x' + d, y, d), the sub-pixel step and the depth.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gsr {

constexpr int STEREO_BLOCK = 256;
constexpr int STEREO_CENSUS_BITS = 62;      // 9 x 7 window, centre excluded
constexpr int STEREO_ABSENT = 1 << 20;      // larger than any L_r + p1

// cv2.remap's fixed-point bilinear rule on one grey channel (the rule of frame_prepare_kernel, gs_frame.h)
__device__ __forceinline__ int stereo_remap_byte(int W, int H, const unsigned char* __restrict__ src, float2 m)
{
    const float fx = fminf(fmaxf(m.x * 32.0f, -1073741824.0f), 1073741824.0f);
    const float fy = fminf(fmaxf(m.y * 32.0f, -1073741824.0f), 1073741824.0f);
    const int X = (int)rintf(fx), Y = (int)rintf(fy);
    const int ax = X & 31, ay = Y & 31;
    const int x0 = min(max(X >> 5, -32768), 32767), y0 = min(max(Y >> 5, -32768), 32767);
    const int w00 = (32 - ax) * (32 - ay) * 32, w01 = ax * (32 - ay) * 32, w10 = (32 - ax) * ay * 32, w11 = ax * ay * 32;
    const bool cx0 = x0 >= 0 && x0 < W, cx1 = x0 + 1 >= 0 && x0 + 1 < W;
    const bool cy0 = y0 >= 0 && y0 < H, cy1 = y0 + 1 >= 0 && y0 + 1 < H;
    int acc = 16384;
    if (cx0 && cy0) acc += w00 * src[(size_t)y0 * W + x0];
    if (cx1 && cy0) acc += w01 * src[(size_t)y0 * W + x0 + 1];
    if (cx0 && cy1) acc += w10 * src[(size_t)(y0 + 1) * W + x0];
    if (cx1 && cy1) acc += w11 * src[(size_t)(y0 + 1) * W + x0 + 1];
    return acc >> 15;
}

// blockIdx.y = side (0 left, 1 right). rect may be NULL (no maps and no copy asked for); image is the left side's only.
__global__ void __launch_bounds__(STEREO_BLOCK) stereo_rectify_kernel(int W, int H, const unsigned char* __restrict__ raw_l,
                                                                      const unsigned char* __restrict__ raw_r, const float2* __restrict__ map_l,
                                                                      const float2* __restrict__ map_r, const float* __restrict__ lut,
                                                                      unsigned char* __restrict__ rect_l, unsigned char* __restrict__ rect_r,
                                                                      float* __restrict__ image)
{
    const size_t N = (size_t)W * H;
    const size_t p = (size_t)blockIdx.x * STEREO_BLOCK + threadIdx.x;
    if (p >= N) return;
    const bool right = blockIdx.y != 0;
    const unsigned char* raw = right ? raw_r : raw_l;
    const float2* map = right ? map_r : map_l;
    unsigned char* rect = right ? rect_r : rect_l;
    const int b = map ? stereo_remap_byte(W, H, raw, map[p]) : raw[p];
    if (rect) rect[p] = (unsigned char)b;
    if (!right && image) {
        const float v = lut[b];
        image[p] = v; image[N + p] = v; image[2 * N + p] = v;
    }
}

// blockIdx.y = side. Bit order: rows top to bottom, columns left to right (only the popcount of an xor is ever used).
__global__ void __launch_bounds__(STEREO_BLOCK) stereo_census_kernel(int W, int H, const unsigned char* __restrict__ img_l,
                                                                     const unsigned char* __restrict__ img_r, uint64_t* __restrict__ code_l,
                                                                     uint64_t* __restrict__ code_r)
{
    const size_t p = (size_t)blockIdx.x * STEREO_BLOCK + threadIdx.x;
    if (p >= (size_t)W * H) return;
    const unsigned char* img = blockIdx.y ? img_r : img_l;
    const int y = (int)(p / W), x = (int)(p - (size_t)y * W);
    const int c = img[p];
    uint64_t code = 0;
#pragma unroll
    for (int dy = -3; dy <= 3; ++dy) {
        const unsigned char* row = img + (size_t)min(max(y + dy, 0), H - 1) * W;
#pragma unroll
        for (int dx = -4; dx <= 4; ++dx) {
            if (dy == 0 && dx == 0) continue;
            code = (code << 1) | (uint64_t)(row[min(max(x + dx, 0), W - 1)] < c);
        }
    }
    (blockIdx.y ? code_r : code_l)[p] = code;
}

__device__ __forceinline__ int stereo_from_lane_below(int v)      // lane l reads lane l - 1; lane 0 gets STEREO_ABSENT
{
    return __builtin_amdgcn_update_dpp(STEREO_ABSENT, v, 0x138, 0xf, 0xf, false);      // wave_shr:1
}
__device__ __forceinline__ int stereo_from_lane_above(int v)      // lane l reads lane l + 1; lane 63 gets STEREO_ABSENT
{
    return __builtin_amdgcn_update_dpp(STEREO_ABSENT, v, 0x130, 0xf, 0xf, false);      // wave_shl:1
}
__device__ __forceinline__ int stereo_wave_min(int v)             // every lane gets the minimum of the 64
{
    unsigned u = (unsigned)v;                                       // the values are non-negative
    u = min(u, lane_xor_value<1>(u));
    u = min(u, lane_xor_value<2>(u));
    u = min(u, lane_xor_value<4>(u));
    u = min(u, lane_xor_value<8>(u));
    u = min(u, lane_xor_value<16>(u));
    u = min(u, lane_xor_value<32>(u));
    return (int)u;
}

template <int DPL> struct StereoRow;                                // a lane's DPL uint16 entries of a pixel's row of S
template <> struct StereoRow<1> { typedef unsigned short type; };
template <> struct StereoRow<2> { typedef unsigned int type; };

constexpr int STEREO_PATH_UNROLL = 4;

// One wave per path of direction (dx, dy); gridDim.x = number of paths (H, W or W + H - 1), blockDim.x = 64.
template <int DPL>
__global__ void __launch_bounds__(64) stereo_path_kernel(int W, int H, int dx, int dy, int p1, int p2, const uint64_t* __restrict__ code_l,
                                                         const uint64_t* __restrict__ code_r, unsigned short* S, int first)
{
    typedef typename StereoRow<DPL>::type row_t;
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
    int Lp[DPL];
    int m = 0;
    for (int k0 = 0; k0 < n; k0 += U) {
        uint64_t cl[U], cr[U][DPL];
        row_t s[U];
#pragma unroll
        for (int j = 0; j < U; ++j) {
            if (k0 + j >= n) continue;                                                    // wave-uniform
            const int x = x0 + (k0 + j) * dx, y = y0 + (k0 + j) * dy;
            const size_t p = (size_t)y * W + x;
            cl[j] = code_l[p];
#pragma unroll
            for (int k = 0; k < DPL; ++k) cr[j][k] = code_r[p - min(lane * DPL + k, x)];  // clamped: the value is unused where x - d < 0
            s[j] = first ? (row_t)0 : reinterpret_cast<const row_t*>(S + p * (size_t)(64 * DPL))[lane];
        }
#pragma unroll
        for (int j = 0; j < U; ++j) {
            if (k0 + j >= n) continue;
            const int x = x0 + (k0 + j) * dx, y = y0 + (k0 + j) * dy;
            const size_t p = (size_t)y * W + x;
            int L[DPL];
#pragma unroll
            for (int k = 0; k < DPL; ++k) L[k] = lane * DPL + k <= x ? __popcll(cl[j] ^ cr[j][k]) : STEREO_CENSUS_BITS;
            if (k0 + j > 0) {
                const int below = stereo_from_lane_below(Lp[DPL - 1]), above = stereo_from_lane_above(Lp[0]);
#pragma unroll
                for (int k = 0; k < DPL; ++k) {
                    const int dn = k == 0 ? below : Lp[k - 1], up = k == DPL - 1 ? above : Lp[k + 1];
                    L[k] += min(min(Lp[k], m + p2), min(dn, up) + p1) - m;
                }
            }
            int lm = L[0];
#pragma unroll
            for (int k = 0; k < DPL; ++k) { Lp[k] = L[k]; lm = min(lm, L[k]); }
            m = stereo_wave_min(lm);
            row_t out;
            if constexpr (DPL == 1) out = (row_t)(s[j] + L[0]);
            else out = (row_t)(((s[j] & 0xffffu) + L[0]) | (((s[j] >> 16) + L[1]) << 16));
            reinterpret_cast<row_t*>(S + p * (size_t)(64 * DPL))[lane] = out;
        }
    }
}

// (S << 8 | d) of the lane's disparities, minimised over the wave: the smallest S, and among equals the smallest d
__device__ __forceinline__ unsigned stereo_wave_min_key(unsigned key)
{
    return (unsigned)stereo_wave_min((int)key);
}

// One wave per pixel; blockDim.x = STEREO_BLOCK (four pixels per block).
template <int DPL>
__global__ void __launch_bounds__(STEREO_BLOCK) stereo_select_kernel(int W, int H, int uniqueness_ratio, int disp12_max_diff, float bf16,
                                                                     const unsigned short* __restrict__ S, short* __restrict__ disparity16,
                                                                     float* __restrict__ depth)
{
    constexpr int D = 64 * DPL;
    constexpr unsigned NONE = 0xffffffffu >> 1;                       // above every key; non-negative as an int
    const int lane = threadIdx.x & 63;
    const size_t p = (size_t)blockIdx.x * (STEREO_BLOCK / 64) + (threadIdx.x >> 6);
    if (p >= (size_t)W * H) return;                                   // wave-uniform
    const int y = (int)(p / W), x = (int)(p - (size_t)y * W);
    const unsigned short* row = S + p * D;
    int s[DPL];
    unsigned key = NONE;
#pragma unroll
    for (int k = 0; k < DPL; ++k) { s[k] = row[lane * DPL + k]; key = min(key, ((unsigned)s[k] << 8) | (unsigned)(lane * DPL + k)); }
    key = stereo_wave_min_key(key);
    const int best = (int)(key & 255u), smin = (int)(key >> 8);
    bool rival = false;                                               // S <= 16872: S * 100 fits 32 bits
#pragma unroll
    for (int k = 0; k < DPL; ++k) {
        const int d = lane * DPL + k;
        rival |= (d < best - 1 || d > best + 1) && s[k] * (100 - uniqueness_ratio) < smin * 100;
    }
    bool valid = x - best >= 0 && !__any(rival);                      // wave-uniform from here on
    if (valid && disp12_max_diff >= 0) {
        const int xr = x - best;
        unsigned rkey = NONE;
#pragma unroll
        for (int k = 0; k < DPL; ++k) {
            const int d = lane * DPL + k;
            if (xr + d < W) rkey = min(rkey, ((unsigned)S[(p - best + d) * D + d] << 8) | (unsigned)d);
        }
        const int dr = (int)(stereo_wave_min_key(rkey) & 255u);
        valid = abs(dr - best) <= disp12_max_diff;
    }
    if (lane != 0) return;
    int out = -16;
    if (valid) {
        out = 16 * best;
        if (best > 0 && best < D - 1) {
            const int a = row[best - 1], b = row[best + 1];
            const int den = max(a + b - 2 * smin, 1);
            out += ((a - b) * 16 + den) / (2 * den);                  // C's truncating division
        }
    }
    disparity16[p] = (short)out;
    if (depth) depth[p] = out > 0 ? __fdiv_rn(bf16, (float)out) : 0.0f;
}

}  // namespace gsr
