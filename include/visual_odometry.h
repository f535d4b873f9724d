/*
 * visual_odometry.h -- C ABI of the dense frame-to-frame odometry (libgs_rasterizer_hip.so). From two consecutive frames -- the previous one
 * with a depth, the current one as an image alone -- estimate the rigid motion between the two cameras by direct photometric alignment: an
 * intensity / depth pyramid per frame (gsr_odometry_pyramid), then a coarse-to-fine Gauss-Newton on SE(3) with Student-t weights
 * (gsr_odometry_align) and an acceptance gate decided on the device. The front-end uses the result as the start of a frame's tracking
 * (slam/frontend.py, Training.pose_prior); the reference starts every frame at the previous pose and has no counterpart. It is specified
 * HERE and restated in float64 numpy in tests/odometry_reference.py: the pyramid equals its float32 restatement bit for bit, the sums of a
 * pass agree within the float32 rounding of their per-pixel terms. gsr_odometry_align models no brightness change between the frames and uses
 * no depth of the current one; gsr_odometry_align_rgbd (restated in tests/odometry_rgbd_reference.py) adds both. All pointers are
 * DEVICE pointers unless said otherwise. Returns 0 or a negative GSR_ERR_* code (gs_rasterizer.h); gsr_last_error() has the text. Nothing is
 * enqueued on a bad argument.
 */
#ifndef VISUAL_ODOMETRY_H_INCLUDED
#define VISUAL_ODOMETRY_H_INCLUDED

#include <stddef.h>
#include "gs_rasterizer.h"   /* GSR_ERR_* */

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of one pyramid buffer; 0 when the size is outside what the pyramid takes: 1 <= levels <= 6, the coarsest level
 * (width >> (levels - 1)) x (height >> (levels - 1)) at least 8 x 8, width * height below 2^31. */
size_t gsr_odometry_pyramid_size(int width, int height, int levels);

/* gsr_odometry_pyramid: the pyramid of one frame into `pyramid` (gsr_odometry_pyramid_size bytes, 16-byte aligned; a shorter one is refused).
 *   level 0    I = (0.299 R + 0.587 G) + 0.114 B in float32, every operation rounded. D = depth where it is finite, positive, inside
 *              [depth_min, depth_max] and mask != 0; else 0.
 *   level l+1  floor(w / 2) x floor(h / 2): an odd last row or column is dropped. I = ((a + b) + (c + d)) * 0.25f over the 2 x 2 block
 *              (a b the upper row, c d the lower), D = the smallest non-zero depth of the block, 0 if it has none.
 * The buffer: a 16-byte head (int32 count of the level-0 pixels with D > 0, then padding), then per level I [h, w] float32 and D [h, w]
 * float32, each starting on a multiple of 16 bytes. image: [3, height, width] float32 in [0, 1]. depth: [height, width] float32 or NULL
 * (all zero). mask: [height, width] bytes or NULL, 0 = exclude. Ranges: 0 <= depth_min <= depth_max. One memset node and `levels`
 * launches on `stream`; the same input gives the same bytes. */
int gsr_odometry_pyramid(int width, int height, int levels, const float* image, const float* depth, const unsigned char* mask,
                         float depth_min, float depth_max, void* pyramid, size_t pyramid_bytes, void* stream);

/* Bytes of workspace gsr_odometry_align needs; 0 for a size gsr_odometry_pyramid_size refuses. */
size_t gsr_odometry_align_workspace_size(int width, int height, int levels);

/* gsr_odometry_align: previous pyramid P (intensity and depth) against current pyramid C (intensity). T maps previous-camera coordinates
 * to current-camera coordinates, T = W2C_cur C2W_prev; it starts at T_init (12 floats are read: the rows of [R | t]; identity when NULL).
 * Level l has fx_l = fx / 2^l, cx_l = (cx + 0.5) / 2^l - 0.5 (pixel centres at integers), likewise y. Levels run from the coarsest to
 * level 0; level l runs iters[l] passes (iters: HOST array of `levels` ints, finest first, each in [0, 64]). One pass, under T = [R | t],
 * for every pixel (u, v) of P_l with depth d > 0:
 *   X = ((u - cx_l) / fx_l d, (v - cy_l) / fy_l d, d),  Y = R X + t,  (x, y) = pi(Y) = (fx_l Y_x / Y_z + cx_l, fy_l Y_y / Y_z + cy_l)
 *   in       Y_z > 1e-3 and 1 <= x < w - 2 and 1 <= y < h - 2
 *   r        bilinear(C_l, x, y) - P_l(u, v)
 *   G        the bilinear sample at (x, y) of the central-difference gradient (C(x+1) - C(x-1)) / 2 of C_l
 *   J        G d pi / d Y [I | -[Y]x], 1 x 6, against a LEFT perturbation xi = [rho | theta] (the order of slam_map.h)
 *   w        (nu + 1) / (nu + (r / sigma)^2), sigma the LAGGED scale: sigma_init in the first pass of the call, afterwards
 *            max(sigma_min, sqrt(sum w r^2 / n)) of the latest earlier pass with n > 0; it carries across levels
 *   H = sum w J^T J,  g = sum w J^T r,  n = the number of pixels in
 *   (H + 1e-9 tr(H) / 6 I) xi = -g by Cholesky in double, T <- exp(xi) T. With n < 6, a matrix that is not positive definite or a step
 *   that is not finite, T is left unchanged and the pass's |xi| counts as infinite.
 * The gate, on the device after the last pass: inlier_share = n of the last pass / the count of D > 0 at level 0 of P (0 when that is 0);
 * accepted when inlier_share >= min_share, the last |xi| <= max_last_step, |t| <= max_translation, the rotation angle <= max_rotation
 * (radians), every entry of T is finite and T_init was finite. A T_init that is not finite cannot be seen by the host, which reads no
 * device memory: the passes then run from identity and the gate refuses the result.
 *   T      16 floats, row-major   the aligned motion when accepted, identity otherwise -- never T_init
 *   stats  8 doubles              accepted (0 / 1), inlier_share, the final sigma, the last |xi|, n of the last pass, |t|, the angle in
 *                                 radians, the count of D > 0 at level 0 of P
 *   trace  [sum of iters, 32] doubles or NULL (tests): per pass in the order run the 21 entries of H (upper triangle, row-major), the 6
 *          of g, sum w, sum w r^2, n, the sigma the pass used, the level
 * Per-pixel terms are float32; every sum is formed in double in one fixed order (thread, wave, block, then the per-block partial sums in
 * block order by the next launch); no float atomics: T, stats and trace are the same bytes on every run. Ranges: nu > 0, sigma_init > 0,
 * 0 < sigma_min, 0 <= min_share <= 1, max_last_step, max_translation, max_rotation >= 0; fx, fy > 0. workspace:
 * gsr_odometry_align_workspace_size bytes, 16-byte aligned; a shorter one is refused. stream: hipStream_t or NULL. Two launches per pass
 * and two more on `stream`; no host read anywhere. */
int gsr_odometry_align(int width, int height, int levels, float fx, float fy, float cx, float cy, const void* previous, const void* current,
                       const float* T_init, const int* iters, float nu, float sigma_init, float sigma_min, float min_share, float max_last_step,
                       float max_translation, float max_rotation, float* T, double* stats, double* trace, void* workspace,
                       size_t workspace_bytes, void* stream);

/* Bytes of workspace gsr_odometry_align_rgbd needs; 0 for a size gsr_odometry_pyramid_size refuses. */
size_t gsr_odometry_align_rgbd_workspace_size(int width, int height, int levels);

/* gsr_odometry_align_rgbd: gsr_odometry_align with two more terms, each switched by an argument: an affine brightness (alpha, beta) between the
 * frames (affine = 1) and an inverse-depth residual against the CURRENT frame's depth (geometric_weight = lambda > 0; the current pyramid is then
 * built with its depth). P, C, T, T_init, the levels, iters and the order of the passes are gsr_odometry_align's. n = 8 unknowns with affine,
 * xi = [rho | theta | d alpha | d beta], else n = 6. alpha = beta = 0 at the start of every call; both carry across passes and levels. One
 * pass, for every pixel (u, v) of P_l with depth d > 0:
 *   X, Y, (x, y), in   exactly as in gsr_odometry_align; (x0, y0) = floor(x, y), (a_x, a_y) = (x, y) - (x0, y0)
 *   photometric  r_I = (bilinear(C_l, x, y) - (1 + alpha) P_l(u, v)) - beta, with 1 + alpha rounded to float32 (affine = 0: as gsr_odometry_align)
 *                J_I = [G d pi / d Y [I | -[Y]x], -P_l(u, v), -1], 1 x 8 (affine = 0: the first six)
 *   depth        taken only where lambda > 0 and the four neighbours D00 = D(y0, x0), D01 = D(y0, x0 + 1), D10 = D(y0 + 1, x0), D11 of C_l's
 *                depth are all > 0 and max - min <= edge_ratio * min; elsewhere the pixel adds its photometric term alone
 *                W.. = 1 / D..,  r_D = bilinear(W, a_x, a_y) - 1 / Y_z
 *                grad W = ((1 - a_y) (W01 - W00) + a_y (W11 - W10), (1 - a_x) (W10 - W00) + a_x (W11 - W01))
 *                J_D = grad W d pi / d Y [I | -[Y]x] + (1 / Y_z^2) e_z^T [I | -[Y]x], 1 x 6; zero in the columns of alpha and beta
 *   weights      w_I = (nu + 1) / (nu + (r_I / sigma_I)^2), w_D likewise with sigma_D; both scales LAGGED as sigma is in gsr_odometry_align,
 *                each from its own sums: sigma_I from sigma_init, max(sigma_min, sqrt(sum w_I r_I^2 / n_I)); sigma_D from sigma_depth_init,
 *                max(sigma_depth_min, sqrt(sum w_D r_D^2 / n_D)) of the latest earlier pass with n_D > 0 (in 1 / metres)
 *   H = sum (w_I / sigma_I^2) J_I^T J_I + sum (lambda w_D / sigma_D^2) J_D^T J_D, g likewise with r_I and r_D; n_I the pixels in, n_D the depth
 *   terms taken. A pixel's photometric term is added to a sum before its depth term.
 *   A = H + 1e-9 tr(H) / n I, A xi = -g by Cholesky in double; T <- exp(xi[0..5]) T, alpha += xi[6], beta += xi[7]. A counts as not positive
 *   definite where a pivot of the factorisation is not above 0 or not above 1e-6 of its diagonal entry A_jj (two columns collinear: the
 *   small multiple of I would otherwise carry them). With n_I < n, such a matrix or a step that is not finite, T, alpha and beta are left
 *   unchanged and the pass's |xi| counts as infinite. |xi| is the norm of all n entries.
 * The gate: gsr_odometry_align's tests with n_I for n, and with affine also |alpha| <= max_gain and |beta| <= max_offset (a value that is not
 * finite fails them). Refused: T is identity.
 *   stats  12 doubles   the 8 of gsr_odometry_align (sigma is sigma_I, n is n_I), then alpha, beta, the final sigma_D, n_D of the last pass
 *   trace  [sum of iters, 64] doubles or NULL (tests): per pass the n (n + 1) / 2 entries of H (upper triangle, row-major), the n of g, then
 *          sum w_I, sum w_I r_I^2, n_I, sum w_D, sum w_D r_D^2, n_D, the sigma_I, sigma_D, alpha and beta the pass used, the level; zeros after
 * A known degeneracy: on a constant previous image the columns -P and -1 of J_I are collinear, alpha and beta cannot be told apart, the
 * factorisation fails at beta's pivot and no step is taken in any pass: the call ends and the gate refuses, with or without the depth term.
 * Callers with such input pass affine = 0.
 * Per-pixel terms are float32; every sum is formed in double in one fixed order (thread, wave, block, then the per-block partial sums in
 * block order by the next launch); no float atomics: T, stats and trace are the same bytes on every run. Ranges: affine 0 or 1;
 * geometric_weight, edge_ratio, max_gain, max_offset >= 0 and the first two finite; sigma_depth_init, sigma_depth_min > 0; the others as in
 * gsr_odometry_align. workspace: gsr_odometry_align_rgbd_workspace_size bytes, 16-byte aligned; a shorter one is refused. Two launches per
 * pass and two more on `stream`; no host read anywhere; nothing is enqueued on a bad argument. */
int gsr_odometry_align_rgbd(int width, int height, int levels, float fx, float fy, float cx, float cy, const void* previous, const void* current,
                            const float* T_init, const int* iters, int affine, float geometric_weight, float edge_ratio, float nu, float sigma_init,
                            float sigma_min, float sigma_depth_init, float sigma_depth_min, float min_share, float max_last_step,
                            float max_translation, float max_rotation, float max_gain, float max_offset, float* T, double* stats, double* trace,
                            void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif
