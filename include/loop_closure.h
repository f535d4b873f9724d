/*
 * loop_closure.h -- C ABI of loop closure (libgs_rasterizer_hip.so): a pose graph over keyframes solved on the device
 * (gsr_pose_graph_solve) and the rigid, piecewise correction of the Gaussian map that follows the corrected keyframes (gsr_map_correct).
 * slam/loop_closure.py builds the loop closer from them; the reference has no counterpart. Everything is specified HERE and restated in
 * float64 numpy in tests/pose_graph_reference.py.
 * All pointers are DEVICE pointers unless said otherwise. Returns 0 or a negative GSR_ERR_* code (gs_rasterizer.h); gsr_last_error() has the
 * text. Nothing is enqueued on a bad argument. No float atomics, no atomics at all; nothing is read by the host. stream: hipStream_t or NULL.
 *
 * Poses. A pose is 12 numbers, the rows of [R | t] (R 3x3 row-major, t the fourth column): x_cam = R x_world + t, a world-to-camera pose.
 * Products and inverses below are those of the 4x4 matrices with the row (0, 0, 0, 1) appended.
 * Exp and Log. tau = (rho | theta), six numbers. Exp(tau) = [R | t] with W = [theta]x, a = |theta|,
 *   R = I + A W + B W^2,  t = (I + B W + C W^2) rho,  A = sin a / a, B = (1 - cos a) / a^2, C = (a - sin a) / a^3;
 *   for a < 1e-5: A = 1, B = 1/2, C = 1/6 (SE3_exp of slam/camera.py). Log is its inverse with |theta| <= pi:
 *   c = (trace R - 1) / 2 clamped to [-1, 1], s = |(R21 - R12, R02 - R20, R10 - R01)| / 2, a = atan2(s, c);
 *   a < 1e-5:            theta = (R21 - R12, R02 - R20, R10 - R01) / 2
 *   c > -0.99:           theta = (a / (2 s)) (R21 - R12, R02 - R20, R10 - R01)
 *   otherwise (near pi): with k the index of the largest diagonal element of R (the lowest on a tie), v = column k of
 *                        (R + R^T) / 2 - c I scaled to unit length, its sign flipped where v . (R21 - R12, R02 - R20, R10 - R01) < 0;
 *                        theta = a v
 *   rho = Vinv t,  Vinv = I - W / 2 + G W^2,  G = 1/12 for a < 1e-5, else (1 - (a / 2) cos(a / 2) / sin(a / 2)) / a^2 (this form of
 *   (1 - A / (2 B)) / a^2 keeps its digits at small angles, where 1 - cos a has lost them).
 */
#ifndef LOOP_CLOSURE_H_INCLUDED
#define LOOP_CLOSURE_H_INCLUDED

#include <stddef.h>
#include "gs_rasterizer.h"   /* GSR_ERR_* */

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of workspace gsr_pose_graph_solve needs; 0 when nodes is outside [1, 4096] or edges outside [0, 65536]. */
size_t gsr_pose_graph_workspace_size(int nodes, int edges);

/* gsr_pose_graph_solve: damped Gauss-Newton on a pose graph, all arithmetic fp64.
 *   poses         double [nodes, 12], world-to-camera X_k; read, and overwritten with the result
 *   fixed         int32 [nodes]; a node with fixed[k] != 0 is not moved
 *   edge_nodes    int32 [edges, 2], rows (i, j);  edge_Z double [edges, 12]: the measured motion Z from camera i to camera j in the
 *                 convention of camera.compose_pose, X_j ~ Z X_i;  edge_weights double [edges, 2], rows (w_t, w_r). All three may be NULL
 *                 with edges == 0.
 * Residual r_e = Log(Z^-1 X_j X_i^-1) = (rho, theta); cost F = sum_e w_t |rho_e|^2 + w_r |theta_e|^2; update X_k <- Exp(delta_k) X_k.
 * Broken edges: an edge with i or j outside [0, nodes), i == j, a non-finite number in Z, or a weight that is not finite or is negative,
 *   is SKIPPED and counted (stats[5]); every other edge is used (stats[4]), one with both weights 0 included. The result is bytewise that of
 *   the graph without the skipped edges.
 * Active nodes: a node is active when fixed[k] == 0 and it is an end of at least one used edge with w_t > 0 and w_r > 0. Every other
 *   node has delta = 0 exactly in every iteration and its pose comes out bit-identical.
 * Linearisation, with E = Z^-1 X_j X_i^-1, r = Log(E): r(delta) ~ r + A_j delta_j + A_i delta_i,
 *   A_j = Jinv(r) Ad(Z^-1),  A_i = -Jinv(-r),  Ad([R | t]) = [[R, [t]x R], [0, R]],
 *   Jinv(r) = I - ad/2 + ad^2/12 - ad^4/720 with ad = [[ [theta]x, [rho]x ], [0, [theta]x ]]: the series of the inverse left Jacobian of
 *   SE(3) cut after the fourth power (its next term is ad^6 / 30240: the cut changes the minimum found by less than |r|^6 / 30240 of a step).
 * One outer iteration: H = sum_e A^T W A, b = -sum_e A^T W r (W = diag(w_t x3, w_r x3)), rows and columns of the active nodes only;
 *   (H + lambda diag(H)) delta = b is solved by conjugate gradients from delta = 0, preconditioned by the inverse of the 6x6 diagonal blocks
 *   of the damped matrix (Cholesky), for at most cg_iters passes; the passes end early where p^T H p <= 0 or r^T M^-1 r falls to 1e-32 of
 *   its first value or to 0. Then the update; the step norm is sqrt(sum_k |delta_k|^2); the outer loop ends after the update whose step
 *   norm is <= step_tol, decided on the device, or after outer_iters updates. lambda is constant; no step is ever rejected.
 * Order of every sum, so that the same input gives the same bytes: per node over its used edges in ascending (edge index, end: i before
 *   j); a dot product or the cost: per node its own terms in component order (the cost of an edge belongs to its node j), then per thread
 *   t of 256 the nodes t, t + 256, ... ascending, then a binary tree over the 256 threads (stride 128, 64, ... 1).
 * Outputs:
 *   D      float32 [nodes, 12]: D_k = X_k,new^-1 X_k,old ([R | t] rows as above), formed in fp64 and rounded once: the map from an old
 *          world point of keyframe k to its new place. A node that did not move has the exact identity.
 *   stats  double [8]: initial cost, final cost, outer iterations used, last step norm, edges used, edges skipped, the largest |t| of any
 *          D_k in metres, the largest rotation angle of any D_k in radians (of the fp64 D_k).
 * Ranges: 1 <= nodes <= 4096, 0 <= edges <= 65536, 0 <= outer_iters <= 1000, 1 <= cg_iters <= 100000, lambda finite and >= 0, step_tol
 *   finite and >= 0. workspace: gsr_pose_graph_workspace_size bytes, 16-byte aligned; a shorter or misaligned one is refused.
 * ONE launch of ONE workgroup of 256 threads on `stream`; its state is in the workspace and in LDS, synchronised by workgroup barriers
 *   alone; every loop is bounded by nodes, edges, outer_iters or cg_iters. The edge lists per node come from a bitonic sort of the keys
 *   (node, 2 edge + end) by that workgroup. */
int gsr_pose_graph_solve(int nodes, int edges, double* poses, const int* fixed, const int* edge_nodes, const double* edge_Z,
                         const double* edge_weights, int outer_iters, int cg_iters, double lambda, double step_tol, float* D, double* stats,
                         void* workspace, size_t workspace_bytes, void* stream);

/* gsr_map_correct: move every Gaussian with the correction of the keyframe that seeded it, in place.
 *   xyz float32 [P, 3]; rotation float32 [P, 4], the raw quaternion (w, x, y, z) as the model stores it, NOT normalised; kf_id int32 [P];
 *   slot_of_frame int32 [frames] (NULL with frames == 0); D float32 [nodes, 12] as gsr_pose_graph_solve writes it.
 * Per Gaussian: s = slot_of_frame[kf_id] where 0 <= kf_id < frames, else -1. s < 0 or s >= nodes: xyz and rotation stay bit-identical
 *   (they are not written). Otherwise, every operation float32, with [R | t] = D_s:
 *     x'_r = fma(R_r2, x_2, fma(R_r1, x_1, fma(R_r0, x_0, t_r)))                        for each row r
 *     q'   = q_D (x) q, the Hamilton product, q_D = (a_w, a_x, a_y, a_z):
 *       w' = fma(-a_z, z, fma(-a_y, y, fma(-a_x, x, a_w w)))      x' = fma(-a_z, y, fma(a_y, z, fma(a_x, w, a_w x)))
 *       y' = fma( a_z, x, fma( a_y, w, fma(-a_x, z, a_w y)))      z' = fma( a_z, w, fma(-a_y, x, fma(a_x, y, a_w z)))
 *   q_D is the unit quaternion of R, computed ONCE per node by a prologue launch (one thread per node), in fp64 from the float32 R and
 *   rounded once: with T = trace R, the branch is the first that holds of T > 0 (from w), R00 >= R11 and R00 >= R22 (from x), R11 >= R22
 *   (from y), else from z (Shepperd's four forms, s = 2 sqrt(1 + the branch's signed diagonal sum)); the result is divided by its norm and
 *   negated where w < 0. A node whose D is the exact identity has q_D = (1, 0, 0, 0) and leaves every byte of its Gaussians as it was.
 * The update is in place on the parameter storage: no pointer changes, so captured graphs that read the parameters stay valid. Adam's
 *   moments are NOT touched: a momentum that is stale by the angle of a correction is harmless, and exp_avg_sq cannot be rotated.
 * Ranges: 0 <= P < 2^31, 0 <= frames, 1 <= nodes <= 4096; xyz, rotation and kf_id 16-byte aligned (four Gaussians per thread, float4 /
 *   int4 loads and stores; the last P % 4 by scalar accesses). quat_workspace: float32 [nodes, 4], 16-byte aligned, written by the prologue.
 * Two launches on `stream`: the prologue (nodes threads) and ONE streaming launch, its grid sized by P. P == 0 enqueues nothing. */
int gsr_map_correct(int P, float* xyz, float* rotation, const int* kf_id, int frames, const int* slot_of_frame, int nodes, const float* D,
                    float* quat_workspace, void* stream);

#ifdef __cplusplus
}
#endif

#endif
