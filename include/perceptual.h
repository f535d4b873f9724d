/*
 * perceptual.h -- C ABI of the LPIPS-specific kernels of the perceptual image metric (libgs_rasterizer_hip.so): LPIPS v0.1 (Zhang et
 * al., CVPR 2018), the input scaling of a batch of image pairs and the distance over the taps of the feature network. The network's
 * convolutions stay with the caller. No launch copies anything to the host, waits for the device or uses a float atomic: the scores
 * stay in device memory and have the same bits on every run. Device pointers unless marked host; float32 and contiguous. Returns 0 or a
 * negative GSR_ERR_* code (gs_rasterizer.h); gsr_last_error() has the text. stream: hipStream_t or NULL.
 */
#ifndef PERCEPTUAL_H_INCLUDED
#define PERCEPTUAL_H_INCLUDED

#include <stddef.h>
#include "gs_rasterizer.h"   /* GSR_ERR_* */

#ifdef __cplusplus
extern "C" {
#endif

#define GSR_LPIPS_MAX_LEVELS 8
#define GSR_LPIPS_NORM_TORCHMETRICS 0   /* f / sqrt(1e-8 + sum f^2) */
#define GSR_LPIPS_NORM_LPIPS 1          /* f / (sqrt(sum f^2) + 1e-10) */

/* gsr_lpips_prepare: x, y [batch, 3, height, width] with values in [0, 1] -> out [2 batch, 3, height, width], the network's input: rows
 * 0 .. batch-1 from x, rows batch .. 2 batch-1 from y, each value (2 v - 1 - shift[c]) / scale[c] with LPIPS' ScalingLayer constants
 * shift = (-.030, -.088, -.188), scale = (.458, .448, .450). One launch. */
int gsr_lpips_prepare(int batch, int height, int width, const float* x, const float* y, float* out, void* stream);

/* gsr_lpips_workspace_size: bytes of the workspace gsr_lpips_distance needs. level_chw (host): 3 ints per level, its channels, height and
 * width. 0 when an argument is out of range (batch < 1, levels outside [1, GSR_LPIPS_MAX_LEVELS], an empty level). */
size_t gsr_lpips_workspace_size(int batch, int levels, const int* level_chw);

/* gsr_lpips_distance: the scores of `batch` pairs. Level l: feat[l] = [2 batch, C_l, h_l, w_l], the tap of the network run on
 * gsr_lpips_prepare's batch; lin[l] = [C_l], the non-negative channel weights. Per level and pixel both feature vectors are
 * unit-normalised over the channels (norm: GSR_LPIPS_NORM_*), sum_c lin[c] (a_c - b_c)^2 is taken of the normalised values, and averaged
 * over the level's pixels; scores[b] is the sum of the level means of pair (row b, row batch + b); taps [batch, levels], when given,
 * receives the level means. Every sum has one fixed order, so a pair's score does not depend on batch; identical rows give exactly 0
 * and exchanging the two images of a pair gives the same bits. workspace: gsr_lpips_workspace_size(batch, levels, level_chw) bytes.
 * Two launches. */
int gsr_lpips_distance(int batch, int levels, const int* level_chw, const float* const* feat, const float* const* lin, int norm,
                       void* workspace, float* taps, float* scores, void* stream);

#ifdef __cplusplus
}
#endif

#endif
