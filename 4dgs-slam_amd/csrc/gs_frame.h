// gs_frame.h -- on-device preparation of one recorded RGB-D frame (include/frame_io.h): cv2.remap's INTER_LINEAR fixed-point path on
// 8-bit data (imgproc/src/imgwarp.cpp, remapBilinear with BORDER_CONSTANT 0), the byte -> float table, the HWC -> CHW transpose and the
// motion-mask threshold, one thread per output pixel. gfx950 / wave64. The source frame (0.9 MB at 640 x 480) stays L2-resident, so
// the byte gathers of the four taps are cheap; every output plane is written coalesced. No atomics, no scratch.
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

}  // namespace gsr
