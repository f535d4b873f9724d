/*
 * frame_io.h -- C ABI of the on-device preparation of one recorded RGB-D frame (libgs_rasterizer_hip.so): lens undistortion, the
 * byte-to-float conversion, the HWC -> CHW transpose and the motion-mask threshold of the reference's monocular / TUM / Bonn /
 * CoFusion datasets (utils/dataset.py:294-300, 326-350, 593-623), in ONE launch per frame; and of the way back, rendered views to the bytes
 * of image files (gsr_frame_export). All pointers are DEVICE pointers.
 * Returns 0 or a negative GSR_ERR_* code (gs_rasterizer.h); gsr_last_error() has the text.
 */
#ifndef FRAME_IO_H_INCLUDED
#define FRAME_IO_H_INCLUDED

#include <stdint.h>
#include "gs_rasterizer.h"   /* GSR_ERR_* */

#ifdef __cplusplus
extern "C" {
#endif

/* gsr_frame_prepare: for every output pixel (u, v) of a width x height frame
 *   source sample   map_xy == NULL: the byte rgb[(v * width + u) * 3 + c]
 *                   otherwise cv2.remap(rgb, mx, my, INTER_LINEAR, BORDER_CONSTANT 0) on 8-bit data, (mx, my) = map_xy[v, u, 0..1]:
 *                     X = rint(mx * 32), Y = rint(my * 32) (round half to even);  x0 = X >> 5, y0 = Y >> 5 (floor; saturated to int16
 *                     as cv2 stores them);  ax = X & 31, ay = Y & 31
 *                     w00 = (32-ax)(32-ay)32, w01 = ax(32-ay)32, w10 = (32-ax)ay 32, w11 = ax ay 32   (sum 32768)
 *                     byte = (sum w * p + 16384) >> 15, with p = 0 for a tap outside the image
 *   image[c, v, u]  = lut[byte]        (lut: 256 floats, the host's float32(b / 255.0) in double -- exact by construction)
 *   motion[v, u]    = !(float(mask_l[v, u]) / 255.0f > mask_threshold)   (1 = static pixel, the reference's ~mask); all 1 when
 *                     mask_l == NULL.  motion may be NULL (no mask output).
 * rgb: HWC, 3 channels, width * height * 3 bytes; map_xy: [height, width, 2] float32 (computed once per camera on the host);
 * image: [3, height, width] float32. stream: hipStream_t or NULL. */
int gsr_frame_prepare(int width, int height, const unsigned char* rgb, const float* map_xy, const float* lut, const unsigned char* mask_l,
                      float mask_threshold, float* image, unsigned char* motion, void* stream);

/* gsr_frame_export: `views` rendered views to the bytes of image files, in ONE launch. colour: views x [3, height, width] float32, view v
 * at colour + v * colour_stride (strides in floats); depth: views x [height, width] float32 at depth + v * depth_stride.
 *   rgb8[v, y, x, c]        = (uint8)(min(max(colour, 0), 1) * 255.0f): truncation; NaN gives 0
 *   depth_rgb8[v, y, x, :]  = lut[i, :], i = (int)(depth / depth_vmax * 256) clamped to [0, 255] (a negative quotient gives 0), the rule of
 *                             matplotlib's imshow(vmin = 0, vmax = depth_vmax); a NaN depth gives the bytes 0, 0, 0. lut: 256 x 3 bytes
 *   depth_u16[v, y, x]      = rint(depth * depth_scale) (round half to even), saturated to [0, 65535]; NaN and negatives give 0
 * depth_rgb8 and depth_u16 may each be NULL (that output is not written); depth may be NULL when both are. rgb8 / depth_rgb8:
 * [views, height, width, 3] bytes, 4-byte aligned; depth_u16: [views, height, width], 8-byte aligned. stream: hipStream_t or NULL. */
int gsr_frame_export(int views, int width, int height, const float* colour, int64_t colour_stride, const float* depth, int64_t depth_stride,
                     const unsigned char* lut, float depth_vmax, float depth_scale, unsigned char* rgb8, unsigned char* depth_rgb8,
                     unsigned short* depth_u16, void* stream);

#ifdef __cplusplus
}
#endif

#endif
