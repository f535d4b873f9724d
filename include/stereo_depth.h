/*
 * stereo_depth.h -- C ABI of the on-device stereo matcher (libgs_rasterizer_hip.so): rectification of an 8-bit grey pair, a census cost,
 * eight-path semi-global aggregation, winner selection with OpenCV's public semantics (disparity x 16 as int16, -16 for "no match", the
 * meaning of uniquenessRatio and disp12MaxDiff) and metric depth bf / disparity -- what the reference's StereoDataset does at ingestion
 * (utils/dataset.py:376-487) with cv2.StereoSGBM on the host. The matcher is specified HERE and restated in integer numpy in
 * tests/stereo_reference.py, which the kernels equal bit for bit; equality with cv2's matcher is not claimed (its cost is block sums of a
 * Birchfield-Tomasi measure, this one is a census transform, so cv2's blockSize has no counterpart). All pointers are DEVICE pointers.
 * Returns 0 or a negative GSR_ERR_* code (gs_rasterizer.h); gsr_last_error() has the text. Nothing is enqueued on a bad argument.
 */
#ifndef STEREO_DEPTH_H_INCLUDED
#define STEREO_DEPTH_H_INCLUDED

#include <stddef.h>
#include "gs_rasterizer.h"   /* GSR_ERR_* */

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of workspace gsr_stereo_depth needs; 0 when the arguments are outside what it takes (width, height >= 1, num_disparities 64 or
 * 128, width * height * num_disparities below 2^31). */
size_t gsr_stereo_workspace_size(int width, int height, int num_disparities);

/* gsr_stereo_depth, with D = num_disparities, for a width x height pair:
 *   rectify      with maps, each byte of left_rect / right_rect is cv2.remap(raw, map, INTER_LINEAR, BORDER_CONSTANT 0) in the fixed-point
 *                form frame_io.h states for gsr_frame_prepare, on the one grey channel; without maps the raw bytes are used (and copied
 *                to left_rect / right_rect where those are given). image[c, v, u] = lut[left byte] for c = 0, 1, 2.
 *   census       a 62-bit code per pixel over the window 9 wide and 7 high around it, centre excluded: a bit is set where the neighbour
 *                is < the centre; neighbour coordinates are clamped to the image.
 *   cost         C(x, y, d) = popcount(cL(x, y) xor cR(x - d, y)) for x - d >= 0, 62 otherwise.
 *   aggregation  eight directions r (four along the axes, four diagonal). A path starts at every pixel p whose predecessor p - r is
 *                outside the image, with L_r(p, .) = C(p, .); afterwards, with q = p - r and m = min_k L_r(q, k),
 *                  L_r(p, d) = C(p, d) + min(L_r(q, d), L_r(q, d-1) + p1, L_r(q, d+1) + p1, m + p2) - m
 *                (the terms at d - 1 < 0 and d + 1 >= D are absent).  S = sum over r of L_r  (<= 8 (62 + p2): 16 bits).
 *   selection    d* = argmin_d S(x, y, d), the first minimum. The pixel is invalid (-16) when x - d* < 0, or some d with |d - d*| > 1
 *                has S(d) (100 - uniqueness_ratio) < S(d*) 100, or disp12_max_diff >= 0 and |dR(x - d*, y) - d*| > disp12_max_diff with
 *                dR(x', y) = argmin over d with x' + d < width of S(x' + d, y, d), the first minimum. A valid pixel stores 16 d* for
 *                d* = 0 or D - 1, else 16 d* + ((S(d*-1) - S(d*+1)) 16 + den) / (2 den), den = max(S(d*-1) + S(d*+1) - 2 S(d*), 1), the
 *                division truncating as C's does.
 *   depth        float32(16 bf) / float32(disparity16) (round to nearest, one division) where disparity16 > 0, else 0; 16 bf is
 *                formed in double and rounded once.
 * Ranges: 0 < p1 < p2 <= 2047, 0 <= uniqueness_ratio <= 99, disp12_max_diff >= -1.
 * left_raw, right_raw: [height, width] bytes. map_left, map_right: [height, width, 2] float32, or both NULL. lut: 256 floats (needed
 * with image). left_rect, right_rect: [height, width] bytes, required with maps, optional without. image: [3, height, width] float32 or
 * NULL. disparity16: [height, width] int16. depth: [height, width] float32 or NULL. cost_sum: [height, width, D] uint16 or NULL, the
 * aggregated volume S (for tests: a mismatch is then localised to the aggregation or to the selection by reading arrays).
 * workspace: gsr_stereo_workspace_size bytes, 16-byte aligned; a shorter one is refused. stream: hipStream_t or NULL. Eleven launches on
 * `stream`, no host read between them, integer arithmetic and no atomics in the matching: the same input gives the same bytes. */
int gsr_stereo_depth(int width, int height, int num_disparities, int p1, int p2, int uniqueness_ratio, int disp12_max_diff, float bf,
                     const unsigned char* left_raw, const unsigned char* right_raw, const float* map_left, const float* map_right,
                     const float* lut, unsigned char* left_rect, unsigned char* right_rect, float* image, short* disparity16, float* depth,
                     unsigned short* cost_sum, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif
