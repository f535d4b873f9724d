/*
 * motion_segmentation.h -- C ABI of the class-agnostic motion segmenter (libgs_rasterizer_hip.so). From the optical flow of a frame pair,
 * the depth of the first frame and the intrinsics: fit the ONE rigid camera motion that explains most of the flow (gsr_flow_rigid_fit: an
 * iteratively reweighted Gauss-Newton fit with Tukey weights whose cutoff follows the median residual of the same pass), call "candidate"
 * whatever the fit cannot explain, and clean the candidates into a few solid regions (gsr_motion_mask_clean: binary opening, 8-connected
 * components, an area filter, a dilation). The reference takes its motion masks from files or from YOLO classes; this is the project's own
 * addition and has no counterpart there. It is specified HERE and restated in float64 numpy / scipy.ndimage in tests/motion_reference.py:
 * the cleaning equals that bit for bit, the fit within the float32 rounding of its per-pixel terms. All pointers are DEVICE pointers.
 * Returns 0 or a negative GSR_ERR_* code (gs_rasterizer.h); gsr_last_error() has the text. Nothing is enqueued on a bad argument.
 */
#ifndef MOTION_SEGMENTATION_H_INCLUDED
#define MOTION_SEGMENTATION_H_INCLUDED

#include <stddef.h>
#include "gs_rasterizer.h"   /* GSR_ERR_* */

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of workspace gsr_flow_rigid_fit needs; 0 when the size is outside what it takes (width, height >= 1, width * height below 2^31). */
size_t gsr_flow_rigid_fit_workspace_size(int width, int height);

/* gsr_flow_rigid_fit, for integer pixel coordinates (u, v) of a width x height frame i and its partner frame j:
 *   X        = ((u - cx) / fx d, (v - cy) / fy d, d), d = depth_i[v, u]                      the pixel's point in camera i
 *   t        = (u + flow_ij[v, u, 0] width / 2, v + flow_ij[v, u, 1] height / 2)              where the flow says it is seen in frame j
 *   usable   d > 0 and finite, the flow finite, t in [0, width - 1] x [0, height - 1] and, with flow_ji, the forward-backward check
 *            |f_ij(p) + bilinear(f_ji, t)| <= occlusion_px with both flows in pixels (an occluded pixel is neither fitted nor called moving)
 *   fit set  usable and (fit_mask == NULL or fit_mask[v, u] != 0)
 * T starts as T_init (identity when NULL). Each of the `iters` passes does, under the current T = [R | t0]:
 *   1. Y = R X + t0, r = pi(Y) - t with pi(Y) = (fx Y_x / Y_z + cx, fy Y_y / Y_z + cy), e = |r|. A pixel with Y_z <= 1e-3 has weight 0 in
 *      this pass and counts in the last bin of the histogram.
 *   2. a histogram of e over the fit set: 1024 bins of 1/16 px (bin = floor(16 e)), the last one open. b = the first bin whose cumulative
 *      count reaches (n + 1) / 2 (integer division, n = pixels of the fit set; b = 0 when n = 0), med = (b + 1) / 16,
 *      c = clamp(scale_multiplier * 1.4826 * med, c_min, c_max). The cutoff of a pass comes from the residuals of that same pass.
 *   3. w = (1 - (e / c)^2)^2 for e < c, else 0;  H = sum w J^T J,  g = sum w J^T r,  with J the 2 x 6 Jacobian of r against a LEFT
 *      perturbation xi = [rho | theta] (the order of the camera deltas of slam_map.h): J = d pi / d Y [I | -[Y]x].
 *   4. (H + 1e-9 tr(H) / 6 I) xi = -g by Cholesky in double, T <- exp(xi) T. A matrix that is not positive definite (an empty fit set)
 *      leaves T unchanged.
 * After the last pass e and c are formed once more under the final T:
 *   residual [height, width] float32   e in pixels; -1 where the pixel is not usable; 3e38 for a usable pixel with Y_z <= 1e-3
 *   T        16 floats, row-major       camera i -> camera j, that is W2C_j C2W_i
 *   stats    4 doubles                  the final c, the number of usable pixels, the number of pixels of the fit set, sum w of the last pass
 *   candidate [height, width] bytes or NULL   1 where usable and residual > max(residual_px, c), else 0; c is read on the device
 *   trace    [iters, 32] doubles or NULL (tests): per pass the 21 entries of H (upper triangle, row-major), the 6 of g, sum w, sum w e^2,
 *            the number of pixels with w > 0, the median bin b, c.
 * Per-pixel terms are float32; every sum is formed in double in one fixed order (thread, wave, block, then the per-block partial sums in
 * block order by a later launch), and the histogram holds integers: T, residual, stats and candidate are the same bytes on every run.
 * Ranges: 1 <= iters <= 64, scale_multiplier > 0, 0 < c_min <= c_max, occlusion_px >= 0, residual_px >= 0; fx, fy > 0.
 * flow_ij, flow_ji: [height, width, 2] float32 in NDC units (pixels * 2 / (width, height)); flow_ji may be NULL. depth_i: [height, width]
 * float32, 0 = no depth. fit_mask: [height, width] bytes or NULL. workspace: gsr_flow_rigid_fit_workspace_size bytes, 16-byte aligned; a
 * shorter one is refused. stream: hipStream_t or NULL. One memset node and 3 iters + 3 launches on `stream`; no host read anywhere. */
int gsr_flow_rigid_fit(int width, int height, float fx, float fy, float cx, float cy, const float* flow_ij, const float* depth_i,
                       const float* flow_ji, const unsigned char* fit_mask, const float* T_init, int iters, float scale_multiplier,
                       float c_min, float c_max, float occlusion_px, float residual_px, float* T, float* residual, double* stats,
                       unsigned char* candidate, double* trace, void* workspace, size_t workspace_bytes, void* stream);

/* Bytes of workspace gsr_motion_mask_clean needs; 0 when the size is outside what it takes (as above). */
size_t gsr_motion_mask_clean_workspace_size(int width, int height);

/* gsr_motion_mask_clean, integers only:
 *   opening     with the (2 open_radius + 1)^2 square: an erosion, then a dilation; pixels outside the image count as 0 (what
 *               scipy.ndimage.binary_erosion / binary_dilation do with border_value = 0)
 *   components  8-connected. labels[v, u] = -1 for background, else the SMALLEST linear index v width + u of the pixel's component
 *               (scipy.ndimage.label with a 3 x 3 structure of ones, relabelled)
 *   filter      a component with fewer than min_area pixels is dropped: its labels become -1
 *   grow        moving = the dilation of the survivors with the (2 grow_radius + 1)^2 square; labels are not grown
 * candidate: [height, width] bytes, non-zero = candidate. moving: [height, width] bytes (0 / 1). labels: [height, width] int32.
 * counts: 4 int32 -- components found, components kept, moving pixels before the grow, moving pixels after it. motion: [height, width]
 * bytes or NULL, updated in place: motion[p] = 0 where moving[p] (True = static, the convention of the motion masks of the datasets).
 * Ranges: 0 <= open_radius, grow_radius <= 8, min_area >= 1. workspace: gsr_motion_mask_clean_workspace_size bytes, 16-byte aligned; a
 * shorter one is refused. Eight launches on `stream`, no host read; the result does not depend on how the blocks were scheduled. */
int gsr_motion_mask_clean(int width, int height, const unsigned char* candidate, int open_radius, int grow_radius, int min_area,
                          unsigned char* moving, int* labels, int* counts, unsigned char* motion, void* workspace, size_t workspace_bytes,
                          void* stream);

#ifdef __cplusplus
}
#endif

#endif
