/*
 * frame_io.h -- C ABI of the on-device preparation of one recorded RGB-D frame (libgs_rasterizer_hip.so): lens undistortion, the
 * byte-to-float conversion, the HWC -> CHW transpose and the motion-mask threshold of the reference's monocular / TUM / Bonn /
 * CoFusion datasets (utils/dataset.py:294-300, 326-350, 593-623), in ONE launch per frame. All pointers are DEVICE pointers.
 * Returns 0 or a negative GSR_ERR_* code (gs_rasterizer.h); gsr_last_error() has the text.
 */
#ifndef FRAME_IO_H_INCLUDED
#define FRAME_IO_H_INCLUDED

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

#ifdef __cplusplus
}
#endif

#endif
