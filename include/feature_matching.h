/*
 * feature_matching.h -- C ABI of the sparse-feature pose stage (libgs_rasterizer_hip.so): the relative pose of two RGB-D frames from
 * matched binary features, the wide-baseline step between place recognition (relocalisation.h) and the dense alignment
 * (visual_odometry.h). Three calls: FAST-9 corners with rotated BRIEF descriptors in a fixed slot layout (gsr_feat_extract; Rosten &
 * Drummond, "Machine learning for high-speed corner detection"; Rublee et al., "ORB: an efficient alternative to SIFT or SURF"), the
 * mutual ratio-tested Hamming match of two such sets (gsr_feat_match), and three-point RANSAC with a point-to-point refinement and a gate
 * on the back-projected matches (gsr_feat_pose). gsr_feat_pose_pnp is the same pose from the 3D points of A and the PIXELS of B alone, for a
 * frame B without depth (a minimal three-point solver for the ranges, then the same triads; restated in tests/pnp_reference.py).
 * slam/features.py builds the stage from them; the reference has no counterpart.
 * Everything is specified HERE, in integers wherever possible, and restated in numpy in tests/features_reference.py: keypoints,
 * descriptors, matches, the count of every hypothesis, the winner and stats equal the restatement bit for bit; T equals it to the last
 * float32 digit or two (below). All pointers are DEVICE pointers. Returns 0 or a negative GSR_ERR_* code (gs_rasterizer.h);
 * gsr_last_error() has the text. Nothing is enqueued on a bad argument. No host read, no allocation, no atomics of any kind; the same
 * input gives the same bytes. Every call can be captured into a graph. stream: hipStream_t or NULL.
 */
#ifndef FEATURE_MATCHING_H_INCLUDED
#define FEATURE_MATCHING_H_INCLUDED

#include <stddef.h>
#include "gs_rasterizer.h"   /* GSR_ERR_* */

#ifdef __cplusplus
extern "C" {
#endif

/* The number of slots of a frame: ceil(width / cell) * ceil(height / cell) * per_cell; 0 outside the ranges of gsr_feat_extract. */
int gsr_feat_slots(int width, int height, int cell, int per_cell);

/* Bytes of workspace gsr_feat_extract needs (luma, corner score, 5 x 5 sums); 0 when width < 1, height < 1 or width * height >= 2^24. */
size_t gsr_feat_extract_workspace_size(int width, int height);

/* gsr_feat_extract: keypoints and descriptors of one frame. image: [3, height, width] float32; mask: [height, width] bytes or NULL, 0 =
 * no corner at the pixel. Pixel p = (x, y) has the index y width + x.
 *   luma         L = (77 qR + 150 qG + 29 qB + 128) >> 8 in [0, 255], q the colour quantisation of relocalisation.h (a NaN gives 0). L
 *                is 0 outside the image.
 *   score        o_0 .. o_15 = (0,-3) (1,-3) (2,-2) (3,-1) (3,0) (3,1) (2,2) (1,3) (0,3) (-1,3) (-2,2) (-3,1) (-3,0) (-3,-1) (-2,-2)
 *                (-1,-3): the radius-3 circle from the top, clockwise with y down. d_k = L(p + o_k) - L(p); bright = max over s of the
 *                minimum of d_(s + j) % 16, j = 0 .. 8; dark the same on -d; score = max(bright, dark, 0): the largest threshold at which
 *                p is still a FAST-9 corner. p is a CORNER where score > threshold, mask != 0, 18 <= x < width - 18 and 18 <= y <
 *                height - 18. c(p) = score at a corner, 0 at every other pixel and outside the image.
 *   suppression  a corner is KEPT when no 8-neighbour n has c(n) > c(p), or c(n) == c(p) and a smaller index.
 *   selection    cells of cell x cell pixels, cells_x = ceil(width / cell), cells_y likewise; the last ones may be cut by the image.
 *                Per cell the per_cell kept corners with the largest score, ties to the smaller index, in that order: rank 0, 1, ...
 *                The corner of rank r of cell (i, j) has the slot (j cells_x + i) per_cell + r. No compaction, no counter: an empty slot
 *                holds the keypoint (-1, -1, 0, 0) and a zero descriptor.
 *   orientation  m10 = the sum of dx L(p + (dx, dy)), m01 = the sum of dy L(p + (dx, dy)) over dx^2 + dy^2 <= 225. directions: int32
 *                [32, 2], rows (c_k, s_k) -- the host passes round(256 cos(2 pi k / 32)), round(256 sin(2 pi k / 32)); no trigonometry
 *                on the device. bin = the k with the largest c_k m10 + s_k m01 in 64-bit integers, the lowest k on a tie.
 *   descriptor   S(p) = the sum of L over the 5 x 5 pixels around p. pattern: int8 [32, 256, 4], rows (ax, ay, bx, by) of the 256 point
 *                pairs of every orientation bin, rotated and rounded by the host; the kernel clamps every entry to [-16, 16], so no
 *                table reads outside the image. Bit i = S(p + a_i) < S(p + b_i) with the pairs of the keypoint's bin, at bit i % 32 of
 *                word i / 32.
 * keypoints: int32 [slots, 4] rows (x, y, score, bin); descriptors: uint32 [slots, 8]. Ranges: width, height >= 1 (below 37 there is no
 * interior and every slot is empty), width * height below 2^24, 8 <= cell <= 64, 1 <= per_cell <= 8, slots <= 4096, 0 <= threshold <=
 * 255. workspace: gsr_feat_extract_workspace_size bytes, 16-byte aligned; a shorter one is refused. Three launches on `stream` (luma,
 * score and sums; suppression and selection, one block per cell; orientation and descriptor, one wave per slot). */
int gsr_feat_extract(int width, int height, const float* image, const unsigned char* mask, int cell, int per_cell, int threshold,
                     const int* directions, const signed char* pattern, int* keypoints, unsigned int* descriptors, void* workspace,
                     size_t workspace_bytes, void* stream);

/* Bytes of workspace gsr_feat_match needs; 0 when slots_a or slots_b is outside [1, 4096]. */
size_t gsr_feat_match_workspace_size(int slots_a, int slots_b);

/* gsr_feat_match: the VALID slots (x >= 0) of A against those of B. d(a, b) = the number of differing bits of the two descriptors.
 *   best      of a: the b with the lexicographically smallest (d, b) over the valid slots of B; second = the smallest d over the other
 *             valid b, 257 where there is none. The best of b over A likewise, with (d, a).
 *   accepted  d <= max_distance, 8 d <= ratio_eighths * second, and the best of b over A is a.
 *   matches   int32 [slots_a, 2]: (b, d) when accepted, otherwise (-1, d) with d of the best; (-1, 257) for an invalid a and against a B
 *             without a valid slot.
 * Ranges: 1 <= slots_a, slots_b <= 4096, 0 <= max_distance <= 256, 0 <= ratio_eighths <= 8. workspace: gsr_feat_match_workspace_size
 * bytes, 16-byte aligned. Three launches on `stream` (A over B and B over A, one wave per slot; the mutual test). */
int gsr_feat_match(int slots_a, const int* keypoints_a, const unsigned int* descriptors_a, int slots_b, const int* keypoints_b,
                   const unsigned int* descriptors_b, int max_distance, int ratio_eighths, int* matches, void* workspace,
                   size_t workspace_bytes, void* stream);

/* Bytes of workspace gsr_feat_pose needs; 0 when slots_a is outside [1, 4096] or hypotheses outside [1, 1024]. */
size_t gsr_feat_pose_workspace_size(int slots_a, int hypotheses);

/* gsr_feat_pose: the motion T with P_b = R P_a + t of the points two frames share, from their matched keypoints and depths. depth_a,
 * depth_b: [height, width] float32; matches: what gsr_feat_match wrote; K_a, K_b: float32 [4] = (fx, fy, cx, cy) each, on the device.
 * Every float32 operation below is rounded by itself (nothing fused), in the order written, sums left to right:
 *   pairs       slot a takes part where matches[a] = (b, .) has 0 <= b < slots_b, both keypoints lie inside the image and both depths
 *               z_a, z_b at the keypoint pixels are finite and positive. The list of such pairs in ascending a has M entries.
 *               P = (((float)x - cx) * z / fx, ((float)y - cy) * z / fy, z) with the frame's own K; (x_b, y_b, z_b) are kept as floats.
 *   draw        hypothesis h: i_k = lowbias32(seed * 0x9E3779B9 + 3 h + k) % M, k = 0, 1, 2, in uint32 arithmetic; lowbias32(x): x ^= x
 *               >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16.
 *   triad       of the points p1, p2, p3: d = p2 - p1; n1 = sqrt(d_x d_x + d_y d_y + d_z d_z); e1 = d / n1; g = p3 - p1; c = e1 x g with
 *               (u x v)_x = u_y v_z - u_z v_y and cyclic; n3 = sqrt(c_x c_x + c_y c_y + c_z c_z); e3 = c / n3; e2 = e3 x e1.
 *   void        a hypothesis is void, and counts 0, with M < 3, two equal indices, or n3 >= min_area false for either frame's triad.
 *   R, t        R_ij = e1b_i e1a_j + e2b_i e2a_j + e3b_i e3a_j; m = (p1 + p2 + p3) / 3 per frame; t_i = mb_i - (R_i0 ma_0 + R_i1 ma_1 +
 *               R_i2 ma_2).
 *   inlier      Q_i = R_i0 P_0 + R_i1 P_1 + R_i2 P_2 + t_i with P of frame A; pair m is an inlier where Q_z > 0, ex = fx_b (Q_x / Q_z)
 *               + cx_b - x_b and ey likewise give ex ex + ey ey <= tau_px tau_px, and |Q_z - z_b| <= tau_depth z_b.
 *   winner      the hypothesis with the most inliers, the lowest h on a tie. With fewer than 3 inliers there is no pose: refused, with
 *               0 final inliers.
 *   refinement  refine_iters Gauss-Newton passes in float64 from the winner's (R, t) over the winner's inliers, the set fixed: q = R P_a
 *               + t, r = q - P_b, J = [I | -[q]x] against a LEFT perturbation xi = [rho | theta] (the order of visual_odometry.h), H =
 *               sum J^T J, g = sum J^T r, every sum in float64 in one fixed order (thread, wave, block); H xi = -g by Cholesky; T <-
 *               exp(xi) T. A matrix that is not positive definite or a step that is not finite ends the refinement where it stands.
 *   recount     R, t are rounded to float32 and the inliers are counted once more, by the rule above.
 *   gate        accepted when M >= min_matches, final inliers >= min_inliers, final inliers >= min_share * M (in float64), |t| <=
 *               max_translation, the rotation angle <= max_rotation (radians), and every entry is finite.
 * Outputs: T float32 [16], row-major: the refined motion when accepted, the identity exactly when refused. stats int32 [8] =
 * (valid keypoints of A, of B, M, winner, the winner's count, final inliers, accepted, 0). counts int32 [hypotheses] or NULL: the count
 * of every hypothesis. The device and the float64 restatement differ in the order of the float64 sums and in the last bits of sin and
 * cos; both round T to float32 once, so T agrees within 2.4e-7 max(1, |entry|).
 * Ranges: width, height >= 1, width * height below 2^31, 1 <= slots_a, slots_b <= 4096, 1 <= hypotheses <= 1024, min_area > 0, tau_px >=
 * 0, tau_depth >= 0, 0 <= refine_iters <= 16, min_matches >= 0, min_inliers >= 3, 0 <= min_share <= 1, max_translation, max_rotation >=
 * 0, all finite. workspace: gsr_feat_pose_workspace_size bytes, 16-byte aligned. Three launches on `stream` (the pair list, one block;
 * the hypotheses, one wave each; winner, refinement and gate, one block). */
int gsr_feat_pose(int width, int height, int slots_a, const int* keypoints_a, const float* depth_a, int slots_b, const int* keypoints_b,
                  const float* depth_b, const int* matches, const float* K_a, const float* K_b, unsigned int seed, int hypotheses,
                  float min_area, float tau_px, float tau_depth, int refine_iters, int min_matches, int min_inliers, float min_share,
                  float max_translation, float max_rotation, float* T, int* stats, int* counts, void* workspace, size_t workspace_bytes,
                  void* stream);

/* Bytes of workspace gsr_feat_pose_pnp needs (those of gsr_feat_pose); 0 when slots_a is outside [1, 4096] or hypotheses outside [1, 1024]. */
size_t gsr_feat_pose_pnp_workspace_size(int slots_a, int hypotheses);

/* gsr_feat_pose_pnp: the motion T with P_b = R P_a + t from the matched keypoints, the depth of frame A and the pixels of frame B: a pose
 * from 2D-3D matches (PnP) for a frame B without depth. NO DEPTH OF B IS READ ANYWHERE. Arguments, outputs, stats and ranges are those of
 * gsr_feat_pose without depth_b and tau_depth. What differs from gsr_feat_pose, every float32 AND float64 operation rounded by itself
 * (nothing fused), in the order written, sums left to right:
 *   pairs       slot a takes part where matches[a] = (b, .) has 0 <= b < slots_b, both keypoints lie inside the image and z_a is finite and
 *               positive. P_a as in gsr_feat_pose; (x_b, y_b) are kept as floats; the bearing in float32 is u = (((float)x_b - cx_b) /
 *               fx_b, ((float)y_b - cy_b) / fy_b, 1).
 *   draw        as in gsr_feat_pose.
 *   ranges      in float64, for the three drawn pairs k = 1, 2, 3 (Grunert's equations, solved by Newton from the keyframe's own ranges;
 *               Haralick et al., "Review and analysis of solutions of the three point perspective pose estimation problem"):
 *               n_k = sqrt(u_x u_x + u_y u_y + u_z u_z), f_k = u_k / n_k; l_k = sqrt(P_x P_x + P_y P_y + P_z P_z) of A's point; for the
 *               pairs (i, j) = (1, 2), (1, 3), (2, 3): c_ij = f_ix f_jx + f_iy f_jy + f_iz f_jz; D = P_i - P_j, d_ij = D_x D_x + D_y D_y +
 *               D_z D_z. Eight times:
 *                 F_ij = l_i l_i + l_j l_j - 2 l_i l_j c_ij - d_ij     (F1 = F_12, F2 = F_13, F3 = F_23; products left to right)
 *                 a = 2 l_1 - 2 l_2 c_12, b = 2 l_2 - 2 l_1 c_12, c = 2 l_1 - 2 l_3 c_13, d = 2 l_3 - 2 l_1 c_13, e = 2 l_2 - 2 l_3 c_23,
 *                 g = 2 l_3 - 2 l_2 c_23                               (the Jacobian [a b 0; c 0 d; 0 e g])
 *                 det = -a d e - b c g; w = F2 g - d F3
 *                 n_1 = -F1 d e - b w, n_2 = a w - F1 c g, n_3 = -a F2 e - b c F3 + F1 c e     (Cramer's rule)
 *                 l_k = l_k - n_k / det
 *               then F_ij once more at the final ranges. Pb_k = (float)(l_k f_k): each of the nine products is rounded to float32 once.
 *   void        a hypothesis is void, and counts 0, with M < 3, two equal indices, a det that is zero or not finite in any step, a final
 *               l_k that is not finite or not positive, |F_ij| <= 1e-9 d_ij false for any pair, or n3 >= min_area false for the triad
 *               of A's triple or of Pb.
 *   R, t        as in gsr_feat_pose, from the triads of A's triple and of Pb_1, Pb_2, Pb_3.
 *   inlier      Q as in gsr_feat_pose; pair m is an inlier where Q_z > 0 and ex ex + ey ey <= tau_px tau_px. There is no depth test.
 *   winner      as in gsr_feat_pose.
 *   refinement  refine_iters Gauss-Newton passes in float64 on the REPROJECTION error over the winner's inliers, the set fixed: q = R P_a
 *               + t, r = (fx_b q_x / q_z + cx_b - x_b, fy_b q_y / q_z + cy_b - y_b), J = d(proj)/dq [I | -[q]x] (two rows per pair)
 *               against the same left perturbation; H, g, the order of the sums, Cholesky, exp and the stopping rules as in gsr_feat_pose.
 *   recount, gate   as in gsr_feat_pose, with the inlier rule above.
 * The device and the restatement differ as those of gsr_feat_pose do (the order of the float64 sums of H and g, the last bits of sin and
 * cos): counts, winner and stats are equal bit for bit, T agrees within 2.4e-7 max(1, |entry|). The ranges rely on the float64 division
 * and square root of the device being correctly rounded, which they are under the library's compiler options (no fast-math flag).
 * One root only: Newton finds the root next to A's ranges, which is the right one while the view of B is not too far from that of A
 * (tests/test_pnp_host.py measures the reach); a complete P3P solver that returns all four roots is not part of this call.
 * Ranges: those of gsr_feat_pose. workspace: gsr_feat_pose_pnp_workspace_size bytes, 16-byte aligned. Three launches on `stream` (the pair
 * list, one block; the hypotheses, one wave each, every lane running the Newton itself; winner, refinement and gate, one block). */
int gsr_feat_pose_pnp(int width, int height, int slots_a, const int* keypoints_a, const float* depth_a, int slots_b, const int* keypoints_b,
                      const int* matches, const float* K_a, const float* K_b, unsigned int seed, int hypotheses, float min_area, float tau_px,
                      int refine_iters, int min_matches, int min_inliers, float min_share, float max_translation, float max_rotation, float* T,
                      int* stats, int* counts, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif
