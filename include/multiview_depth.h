/*
 * multiview_depth.h -- C ABI of the on-device plane sweep (libgs_rasterizer_hip.so): depth of a reference view from up to four partner views
 * with known relative poses. 64 inverse-depth hypotheses per pixel, the census cost and the eight-path semi-global aggregation of
 * stereo_depth.h, a selection that refuses what the sweep cannot decide, and depth = 1 / inverse depth. It seeds the keyframes of a
 * monocular run from the window's keyframes (slam/sweep.py, slam/frontend.py); the reference has no counterpart (it seeds the median of the
 * rendered depth plus noise). The sweep is specified HERE and restated in numpy in tests/sweep_reference.py -- integer for the matching,
 * float32 operation by operation for the projection -- which the kernels equal bit for bit. All pointers are DEVICE pointers. Returns 0 or
 * a negative GSR_ERR_* code (gs_rasterizer.h); gsr_last_error() has the text. Nothing is enqueued on a bad argument.
 */
#ifndef MULTIVIEW_DEPTH_H_INCLUDED
#define MULTIVIEW_DEPTH_H_INCLUDED

#include <stddef.h>
#include "gs_rasterizer.h"   /* GSR_ERR_* */

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of workspace gsr_sweep_depth needs; 0 when the arguments are outside what it takes (width, height >= 1, 1 <= partners <= 4,
 * width * height * 64 below 2^31). */
size_t gsr_sweep_workspace_size(int width, int height, int partners);

/* gsr_sweep_depth, for a width x height reference view and J = partners views of the same size and intrinsics (fx, fy, cx, cy). There are
 * D = 64 hypotheses; hypothesis k is the inverse depth w_k = w_min + float(k) * w_step. Every float operation named below is ONE float32
 * operation rounded to nearest, in the order written, none contracted into a fused multiply-add.
 *   census         of the reference and of every partner: exactly stereo_depth.h's (62 bits, 9 wide and 7 high, centre excluded, a bit set
 *                  where the neighbour is < the centre, coordinates clamped to the image).
 *   projection     of pixel (u, v) into partner j, whose row of `transforms` is T = [R | t], row-major 3 x 4, reference camera to partner
 *                  camera:
 *                    rx = (float(u) - cx) / fx,  ry = (float(v) - cy) / fy
 *                    a_i = (R_i0 * rx + R_i1 * ry) + R_i2,  X_i = a_i + t_i * w_k            (i = 0, 1, 2)
 *                    up = fx * (X_0 / X_2) + cx,  vp = fy * (X_1 / X_2) + cy
 *                  hypothesis k is VISIBLE in j when X_2 > 1e-6f, -0.5 <= up < float(width) - 0.5 and -0.5 <= vp < float(height) - 0.5 (a
 *                  comparison with a NaN is false); it then samples the partner's pixel q = (floor(up + 0.5f), floor(vp + 0.5f)).
 *   cost           C(p, k) = sum over j of (visible ? popcount(code_ref(p) xor code_j(q)) : 62)   (<= 248: 8 bits).
 *   observability  a pixel is OBSERVABLE when for at least one partner hypotheses 0 and 63 both lie in front of it (X_2 > 1e-6f) and
 *                  trunc(max(|up_63 - up_0|, |vp_63 - vp_0|)) >= float(min_span_px) (one subtraction each; the maximum of du and dv is
 *                  du > dv ? du : dv): the swept range moves the pixel far enough in that partner to tell its ends apart. The two
 *                  projections need not fall inside the partner's image: the rule is about parallax, and a pixel near the border the
 *                  partner lies towards is matched by the hypotheses that do fall inside.
 *   aggregation    stereo_depth.h's, on this C, over k in place of d: eight directions r; a path starts at every pixel p whose predecessor
 *                  p - r is outside the image, with L_r(p, .) = C(p, .); afterwards, with q = p - r and m = min_k L_r(q, k),
 *                    L_r(p, k) = C(p, k) + min(L_r(q, k), L_r(q, k-1) + p1, L_r(q, k+1) + p1, m + p2) - m
 *                  (the terms at k - 1 < 0 and k + 1 >= 64 are absent).  S = sum over r of L_r  (<= 8 (248 + p2): 16 bits).
 *   selection      k* = argmin_k S(p, k), the first minimum. The pixel is invalid (index16 = -16, depth 0) when it is not observable, or k*
 *                  is 0 or 63 (the answer lies outside the swept range), or some k with |k - k*| > 1 has
 *                  S(k) (100 - uniqueness_ratio) < S(k*) 100; the three tests are independent. A valid pixel stores
 *                  index16 = 16 k* + ((S(k*-1) - S(k*+1)) 16 + den) / (2 den), den = max(S(k*-1) + S(k*+1) - 2 S(k*), 1), the division
 *                  truncating as C's does.
 *   depth          1 / (w_min + (float(index16) / 16) * w_step) for a valid pixel: a division, a multiplication, an addition, a division.
 * Ranges: 1 <= partners <= 4, 0 < p1 < p2 <= 2047, 0 <= uniqueness_ratio <= 99, min_span_px >= 0, w_min >= 0 and w_step > 0, both finite.
 * ref_grey: [height, width] bytes. partner_grey: [J, height, width] bytes. transforms: [J, 12] float32. index16: [height, width] int16.
 * depth: [height, width] float32. cost: [height, width, 64] uint8 or NULL, the volume C; cost_sum: [height, width, 64] uint16 or NULL, the
 * volume S (for tests: a mismatch is then localised to the projection, the aggregation or the selection by reading arrays). workspace:
 * gsr_sweep_workspace_size bytes, 16-byte aligned; a shorter one is refused. stream: hipStream_t or NULL. One to three census launches, one
 * cost launch, eight path launches and one selection on `stream`, no host read between them and no atomics: the same input gives the same
 * bytes. Census windows are compared fronto-parallel: strong rotation or forward motion between the views weakens the cost. */
int gsr_sweep_depth(int width, int height, int partners, float fx, float fy, float cx, float cy, float w_min, float w_step, int p1, int p2,
                    int uniqueness_ratio, int min_span_px, const unsigned char* ref_grey, const unsigned char* partner_grey,
                    const float* transforms, short* index16, float* depth, unsigned char* cost, unsigned short* cost_sum, void* workspace,
                    size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif
