/*
 * optical_flow.h -- C ABI of the RAFT-specific kernels of the optical-flow estimator (libgs_rasterizer_hip.so): the all-pairs
 * correlation pyramid of RAFT/corr.py CorrBlock in both directions, its 9x9 window lookup, and RAFT.upsample_flow's convex upsampling
 * with the InputPadder crop and the NDC scaling of utils/camera_utils.py:412-413; and of the two kernels GMA (GMA/gma.py, RAFT with
 * global motion aggregation) adds: the attention over all low-resolution pixels and its aggregation of the motion features. The
 * convolutions of the network stay with the caller.
 * All pointers are DEVICE pointers, float32, contiguous. Returns 0 or a negative GSR_ERR_* code (gs_rasterizer.h); gsr_last_error()
 * has the text. stream: hipStream_t or NULL.
 */
#ifndef OPTICAL_FLOW_H_INCLUDED
#define OPTICAL_FLOW_H_INCLUDED

#include "gs_rasterizer.h"   /* GSR_ERR_* */

#ifdef __cplusplus
extern "C" {
#endif

#define GSR_RAFT_LEVELS 4
#define GSR_RAFT_CORR_CHANNELS 324   /* 4 levels x 9 x 9 */
#define GSR_RAFT_MASK_CHANNELS 576   /* 9 neighbours x 8 x 8 sub-pixels */

/* gsr_raft_corr_pyramid: with N = h * w and the fmaps f1, f2 [dim, h, w],
 *   level 0:  c12[p1][p2] = sum_k f1[k][p1] f2[k][p2] / sqrt(dim)   ([N, h, w]: row p1, image 2's pixel grid)
 *             c21[p2][p1] = c12[p1][p2]                              ([N, h, w]: row p2, image 1's pixel grid)
 *   level l:  avg_pool2d(level l-1, 2, 2) over the last two axes, floor sizes ([N, h_l, w_l], each level halving the previous, floored)
 * pyr12[l] / pyr21[l]: the level-l volume of each direction; pyr21 == NULL computes the 1->2 pyramid only, with the same bits.
 * Every element is reduced over k in one fixed order, so c21 is bitwise the transpose of c12. Needs h >> 3 >= 1 and w >> 3 >= 1. */
int gsr_raft_corr_pyramid(int dim, int h, int w, const float* f1, const float* f2, float* const* pyr12, float* const* pyr21, void* stream);

/* gsr_raft_corr_lookup: CorrBlock.__call__ for `batch` (1 or 2) coordinate fields coords [batch, 2, h, w] (x, y in low-res pixels),
 * batch b sampling the pyramid pyr[4 b .. 4 b + 3] (as written by gsr_raft_corr_pyramid):
 *   out[b][81 l + 9 a + c][y][x] = bilinear sample of level l, row (y, x), at (coords_x / 2^l + a - 4, coords_y / 2^l + c - 4)
 * with grid_sample's align_corners=True arithmetic and zero padding. out: [batch, 324, h, w]. Needs h >> 3 >= 2 and w >> 3 >= 2
 * (bilinear_sampler divides by each level's side - 1). */
int gsr_raft_corr_lookup(int batch, int h, int w, const float* const* pyr, const float* coords, float* out, void* stream);

/* gsr_raft_upsample: RAFT.upsample_flow of flow [batch, 2, h, w] with the mask [batch, 576, h, w] (softmax over the 9 neighbours of each
 * 8 x 8 sub-pixel), cropped to the out_w x out_h window at (pad_left, pad_top) of the 8h x 8w result. out: [batch, out_h, out_w, 2]; with
 * ndc != 0 the flow is divided by (out_w, out_h) and multiplied by 2. */
int gsr_raft_upsample(int batch, int h, int w, const float* flow, const float* mask, int pad_left, int pad_top, int out_w, int out_h, int ndc,
                      float* out, void* stream);

/* gsr_gma_attention: GMA/gma.py Attention.forward with one head and content only, for `batch` (1 or 2) maps q, k [batch, dim, h, w]
 * (the two halves of to_qk's output). With N = h * w and pixels flattened row-major,
 *   sim[b][i][j]  = sum_c (scale * q[b][c][i]) k[b][c][j]     (q is scaled before the product; c ascending, exact f32 products)
 *   attn[b][i][j] = exp(sim[b][i][j] - max_j sim[b][i]) / sum_j exp(sim[b][i][j] - max_j sim[b][i])
 * attn: [batch, N, N], written as sim and normalised in place. The row maximum is subtracted, and every sum is taken in one fixed order
 * with no atomics, so the result is bitwise the same on every call and a batch-2 call equals two batch-1 calls. Needs dim % 4 == 0,
 * h, w >= 1 and N <= 65535. */
int gsr_gma_attention(int batch, int dim, int h, int w, const float* q, const float* k, float scale, float* attn, void* stream);

/* gsr_gma_aggregate: GMA/gma.py Aggregate.forward after its to_v convolution (one head, no projection), one launch for the batch:
 *   out[b][c][i] = x[b][c][i] + gamma * sum_j attn[b][i][j] v[b][c][j]
 * attn: [batch, N, N] (gsr_gma_attention); v, x, out: [batch, dim, h, w]; out must not alias x or v. Each element is reduced by one block
 * in one fixed order (exact f32 products; four interleaved partial sums, s_g over the j with j / 32 mod 4 = g ascending, added as (s0 + s1) + (s2 + s3); no split
 * across blocks, no atomics): bitwise the same on every call, and a batch-2 call equals two batch-1 calls. The same size limits as
 * gsr_gma_attention. */
int gsr_gma_aggregate(int batch, int dim, int h, int w, const float* attn, const float* v, const float* x, float gamma, float* out,
                      void* stream);

#ifdef __cplusplus
}
#endif

#endif
