// gs_frame.h -- on-device preparation of one recorded RGB-D frame (include/frame_io.h): cv2.remap's INTER_LINEAR fixed-point path on
// 8-bit data (imgproc/src/imgwarp.cpp, remapBilinear with BORDER_CONSTANT 0), the byte -> float table, the HWC -> CHW transpose and the
// motion-mask threshold, one thread per output pixel. gfx950 / wave64. The source frame (0.9 MB at 640 x 480) stays L2-resident, so
// the byte gathers of the four taps are cheap; every output plane is written coalesced. No atomics, no scratch.
// frame_export_kernel is the way back: rendered float planes of V views to the bytes of image files (gsr_frame_export), one launch.
#pragma once
#include <hip/hip_runtime.h>

namespace gsr {

constexpr int FRAME_BLOCK = 256;

__global__ void __launch_bounds__(FRAME_BLOCK) frame_prepare_kernel(int W, int H, const unsigned char* __restrict__ rgb,
                                                                    const float2* __restrict__ map_xy, const float* __restrict__ lut,
                                                                    const unsigned char* __restrict__ mask_l, float mask_threshold,
                                                                    float* __restrict__ image, unsigned char* __restrict__ motion)
{
    __shared__ float s_lut[256];
    s_lut[threadIdx.x] = lut[threadIdx.x];          // FRAME_BLOCK == 256: one table entry per thread
    __syncthreads();
    const int N = W * H;
    const int p = blockIdx.x * FRAME_BLOCK + threadIdx.x;
    if (p >= N) return;
    int b0, b1, b2;
    if (!map_xy) {
        const unsigned char* s = rgb + 3 * (size_t)p;
        b0 = s[0]; b1 = s[1]; b2 = s[2];
    } else {
        const float2 m = map_xy[p];
        // cvRound(m * INTER_TAB_SIZE): round half to even. The clamp keeps the conversion defined for wild maps (NaN -> outside too).
        const float fx = fminf(fmaxf(m.x * 32.0f, -1073741824.0f), 1073741824.0f);
        const float fy = fminf(fmaxf(m.y * 32.0f, -1073741824.0f), 1073741824.0f);
        const int X = (int)rintf(fx), Y = (int)rintf(fy);
        const int ax = X & 31, ay = Y & 31;
        const int x0 = min(max(X >> 5, -32768), 32767), y0 = min(max(Y >> 5, -32768), 32767);   // cv2 keeps the taps as int16
        const int w00 = (32 - ax) * (32 - ay) * 32, w01 = ax * (32 - ay) * 32, w10 = (32 - ax) * ay * 32, w11 = ax * ay * 32;
        const bool cx0 = x0 >= 0 && x0 < W, cx1 = x0 + 1 >= 0 && x0 + 1 < W;
        const bool cy0 = y0 >= 0 && y0 < H, cy1 = y0 + 1 >= 0 && y0 + 1 < H;
        int acc0 = 16384, acc1 = 16384, acc2 = 16384;         // + (1 << 14): FixedPtCast's rounding
        auto tap = [&](bool ok, int x, int y, int w) {
            if (!ok) return;                                    // BORDER_CONSTANT: the constant is 0
            const unsigned char* s = rgb + 3 * ((size_t)y * W + x);
            acc0 += w * s[0]; acc1 += w * s[1]; acc2 += w * s[2];
        };
        tap(cx0 && cy0, x0, y0, w00);
        tap(cx1 && cy0, x0 + 1, y0, w01);
        tap(cx0 && cy1, x0, y0 + 1, w10);
        tap(cx1 && cy1, x0 + 1, y0 + 1, w11);
        b0 = acc0 >> 15; b1 = acc1 >> 15; b2 = acc2 >> 15;       // <= (255 * 32768 + 16384) >> 15 = 255
    }
    image[p] = s_lut[b0];
    image[N + p] = s_lut[b1];
    image[2 * (size_t)N + p] = s_lut[b2];
    if (motion) motion[p] = mask_l ? (unsigned char)!(__fdiv_rn((float)mask_l[p], 255.0f) > mask_threshold) : (unsigned char)1;
}

// ---- gsr_frame_export: V rendered views -> 8-bit RGB, colour-mapped depth and 16-bit depth, blockIdx.y = view -------------------------
// A thread owns 4 consecutive pixels of a row: one float4 load per plane, three dword stores per RGB output, one 8-byte store of the
// 16-bit depth. That needs the group's first pixel at a multiple of 4 in every buffer (checked per thread from the addresses); the last
// partial group of a row, and every group of a frame whose rows do not start on such a boundary, goes pixel by pixel.
__device__ __forceinline__ unsigned export_colour_byte(float x)
{
    const float c = x > 0.0f ? (x < 1.0f ? x : 1.0f) : 0.0f;        // min(max(x, 0), 1); a NaN fails `x > 0`: 0
    return (unsigned)(int)__fmul_rn(c, 255.0f);                    // truncation, as (image * 255).astype(uint8) after the clamp
}

// index into the 256-row table, or -1 for NaN (bytes 0, 0, 0): matplotlib's rule for imshow(vmin = 0, vmax)
__device__ __forceinline__ int export_depth_index(float d, float vmax)
{
    const float n = __fdiv_rn(d, vmax);
    if (n != n) return -1;
    const float s = __fmul_rn(n, 256.0f);
    return s < 0.0f ? 0 : (s >= 255.0f ? 255 : (int)s);
}

__device__ __forceinline__ unsigned export_depth_u16(float d, float scale)
{
    const float r = rintf(__fmul_rn(d, scale));                     // round half to even
    return r > 0.0f ? (r < 65535.0f ? (unsigned)(int)r : 65535u) : 0u;   // NaN and negatives: 0
}

__device__ __forceinline__ void export_store_rgb4(unsigned char* dst, const unsigned (&r)[4], const unsigned (&g)[4], const unsigned (&b)[4])
{
    uint3 w;
    w.x = r[0] | (g[0] << 8) | (b[0] << 16) | (r[1] << 24);
    w.y = g[1] | (b[1] << 8) | (r[2] << 16) | (g[2] << 24);
    w.z = b[2] | (r[3] << 8) | (g[3] << 16) | (b[3] << 24);
    *reinterpret_cast<uint3*>(dst) = w;
}

__global__ void __launch_bounds__(FRAME_BLOCK) frame_export_kernel(int W, int H, const float* __restrict__ colour, long long colour_stride,
                                                                   const float* __restrict__ depth, long long depth_stride,
                                                                   const unsigned char* __restrict__ lut, float depth_vmax, float depth_scale,
                                                                   unsigned char* __restrict__ rgb8, unsigned char* __restrict__ depth_rgb8,
                                                                   unsigned short* __restrict__ depth_u16)
{
    __shared__ unsigned char s_lut[768];
    for (int k = threadIdx.x; k < 768; k += FRAME_BLOCK) s_lut[k] = lut[k];
    __syncthreads();
    const int groups = (W + 3) >> 2;                                 // 4-pixel groups per row
    const int t = blockIdx.x * FRAME_BLOCK + threadIdx.x;
    if (t >= groups * H) return;
    const int row = t / groups, x0 = (t - row * groups) << 2;
    const int n = min(4, W - x0);
    const size_t N = (size_t)W * H, v = blockIdx.y;
    const size_t p = (size_t)row * W + x0;                           // first pixel of the group in its plane
    const float* cr = colour + v * (size_t)colour_stride + p;
    const float* cd = depth ? depth + v * (size_t)depth_stride + p : nullptr;
    const size_t q = v * N + p;                                      // ... and in the [V, H, W] outputs
    const bool fast = n == 4 && (q & 3) == 0 && ((reinterpret_cast<size_t>(cr) | reinterpret_cast<size_t>(cr + N) | reinterpret_cast<size_t>(cr + 2 * N) |
                                                   reinterpret_cast<size_t>(cd)) & 15) == 0;
    if (fast) {
        const float4 fr = *reinterpret_cast<const float4*>(cr), fg = *reinterpret_cast<const float4*>(cr + N),
                     fb = *reinterpret_cast<const float4*>(cr + 2 * N);
        const unsigned r[4] = {export_colour_byte(fr.x), export_colour_byte(fr.y), export_colour_byte(fr.z), export_colour_byte(fr.w)};
        const unsigned g[4] = {export_colour_byte(fg.x), export_colour_byte(fg.y), export_colour_byte(fg.z), export_colour_byte(fg.w)};
        const unsigned b[4] = {export_colour_byte(fb.x), export_colour_byte(fb.y), export_colour_byte(fb.z), export_colour_byte(fb.w)};
        export_store_rgb4(rgb8 + 3 * q, r, g, b);
        if (!cd) return;
        const float4 fd = *reinterpret_cast<const float4*>(cd);
        if (depth_rgb8) {
            const int i4[4] = {export_depth_index(fd.x, depth_vmax), export_depth_index(fd.y, depth_vmax), export_depth_index(fd.z, depth_vmax),
                               export_depth_index(fd.w, depth_vmax)};
            unsigned dr[4], dg[4], db[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int i = max(i4[k], 0) * 3;
                const unsigned keep = i4[k] < 0 ? 0u : 0xffu;
                dr[k] = s_lut[i] & keep; dg[k] = s_lut[i + 1] & keep; db[k] = s_lut[i + 2] & keep;
            }
            export_store_rgb4(depth_rgb8 + 3 * q, dr, dg, db);
        }
        if (depth_u16) {
            uint2 w;
            w.x = export_depth_u16(fd.x, depth_scale) | (export_depth_u16(fd.y, depth_scale) << 16);
            w.y = export_depth_u16(fd.z, depth_scale) | (export_depth_u16(fd.w, depth_scale) << 16);
            *reinterpret_cast<uint2*>(depth_u16 + q) = w;
        }
        return;
    }
    for (int k = 0; k < n; ++k) {                                    // n <= 4
        unsigned char* o = rgb8 + 3 * (q + k);
        o[0] = (unsigned char)export_colour_byte(cr[k]);
        o[1] = (unsigned char)export_colour_byte(cr[N + k]);
        o[2] = (unsigned char)export_colour_byte(cr[2 * N + k]);
        if (!cd) continue;
        const float d = cd[k];
        if (depth_rgb8) {
            const int i = export_depth_index(d, depth_vmax);
            unsigned char* od = depth_rgb8 + 3 * (q + k);
            od[0] = i < 0 ? 0 : s_lut[3 * i]; od[1] = i < 0 ? 0 : s_lut[3 * i + 1]; od[2] = i < 0 ? 0 : s_lut[3 * i + 2];
        }
        if (depth_u16) depth_u16[q + k] = (unsigned short)export_depth_u16(d, depth_scale);
    }
}

}  // namespace gsr
