/*
 * relocalisation.h -- C ABI of the keyframe relocaliser (libgs_rasterizer_hip.so): recover a camera whose pose is unknown. Three calls:
 * the randomised-fern code of a frame (gsr_reloc_encode; Glocker et al., "Real-Time RGB-D Camera Relocalization via Randomized Ferns for
 * Keyframe Encoding", the relocaliser of ElasticFusion and InfiniTAM), the block-wise Hamming search of a code in a database of keyframe
 * codes (gsr_reloc_search), and the verdict counts that say whether the map rendered at a pose agrees with a frame (gsr_reloc_score; the
 * "am I lost?" test of a run). slam/relocalise.py builds the relocaliser from them; the reference has no counterpart. Everything is
 * specified HERE in integers and restated in numpy in tests/reloc_reference.py: the three outputs equal the restatement bit for bit.
 * All pointers are DEVICE pointers unless said otherwise. Returns 0 or a negative GSR_ERR_* code (gs_rasterizer.h); gsr_last_error() has
 * the text. Nothing is enqueued on a bad argument. No host read anywhere, no float atomics; the integer atomics of gsr_reloc_score add
 * counters, whose value does not depend on the order. stream: hipStream_t or NULL.
 *
 * Quantisation (both gsr_reloc_encode and gsr_reloc_score), every operation rounded to float32, nothing fused:
 *   colour  q(v) = (int)(min(max(v, 0), 1) * 255.0f + 0.5f), in [0, 255]; a NaN gives 0.
 */
#ifndef RELOCALISATION_H_INCLUDED
#define RELOCALISATION_H_INCLUDED

#include <stddef.h>
#include "gs_rasterizer.h"   /* GSR_ERR_* */

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of workspace gsr_reloc_encode needs (the sums of every cell); 0 when grid_w < 1, grid_h < 1 or grid_w * grid_h > 4096. */
size_t gsr_reloc_encode_workspace_size(int grid_w, int grid_h);

/* gsr_reloc_encode: the fern code of one frame. image: [3, height, width] float32. depth: [height, width] float32 or NULL. mask:
 * [height, width] bytes or NULL, 0 = exclude the pixel.
 *   depth   a pixel's depth d is valid where it is finite, d > 0 and mask != 0; then s = d * depth_scale, dq = 65535 where s >= 65535,
 *           else (int)(s + 0.5f); dq == 0 makes the pixel invalid after all.
 *   cells   cell (i, j), 0 <= i < grid_w, 0 <= j < grid_h, covers x in [floor(i width / grid_w), floor((i + 1) width / grid_w)) and y
 *           likewise; its number is j grid_w + i. Per cell: S_R, S_G, S_B = the sums of q over its pixels with mask != 0, n their count;
 *           S_D = the sum of dq over its valid depth pixels, n_D their count.
 *   ferns   fern_table: int32 [ferns, 5], rows (cell, tR, tG, tB, tD). Fern f reads cell (unsigned)cell % (grid_w * grid_h): no table
 *           reads out of bounds. bR = S_R > tR n, likewise G and B; bD = S_D > tD n_D. Sums, products and comparisons are 32-bit: S, t n
 *           are taken modulo 2^32 and compared as int32 (no sum of a frame within the ranges below wraps for n <= 32768 pixels per
 *           cell; a table may hold any thresholds). An empty cell (n = 0, or n_D = 0 for bD) gives bit 0; depth == NULL gives bD = 0.
 *   code    ferns / 8 uint32 words: the nibble bR | bG << 1 | bB << 2 | bD << 3 of fern f at bits 4 (f % 8) of word f / 8. It may
 *           point into a row of a database: appending a keyframe is this call.
 * Ranges: 1 <= grid_w <= width, 1 <= grid_h <= height, grid_w * grid_h <= 4096, ferns a multiple of 8 in [8, 2048], width * height
 * below 2^23, depth_scale finite and > 0. workspace: gsr_reloc_encode_workspace_size bytes, 16-byte aligned; a shorter one is refused.
 * Two launches on `stream` (cell sums: one block per cell, integer sums in one block, no atomics; ferns); the same input gives the same
 * bytes. */
int gsr_reloc_encode(int width, int height, const float* image, const float* depth, const unsigned char* mask, int grid_w, int grid_h,
                     int ferns, const int* fern_table, float depth_scale, unsigned int* code, void* workspace, size_t workspace_bytes,
                     void* stream);

/* gsr_reloc_search: a query code against a database of `rows` codes. database: uint32 [rows, ferns / 8] (NULL with rows == 0); query:
 * uint32 [ferns / 8]; nibble_mask in [1, 15] selects the bits of a nibble that count (0x7 ignores the depth bit, 0xF uses it).
 *   distance  int32 [rows] (NULL with rows == 0): distance[k] = the number of ferns whose masked nibble differs from the query's.
 *   best      int32 [topk, 2], rows (index, distance): the topk rows of the database with the smallest (distance, index), ascending in
 *             that lexicographic order -- ties go to the lower index. Slots past `rows` hold (-1, ferns + 1).
 * Ranges: 0 <= rows <= 2^20, ferns a multiple of 8 in [8, 2048], 1 <= topk <= 16. Two launches on `stream` (distances; selection by one
 * block), one with rows == 0. */
int gsr_reloc_search(int rows, int ferns, const unsigned int* database, const unsigned int* query, int nibble_mask, int topk, int* distance,
                     int* best, void* stream);

/* gsr_reloc_score: does the map rendered at a pose agree with the frame? render: [3, height, width] float32 with its render_depth and
 * opacity [height, width] float32; image: [3, height, width] float32, depth: [height, width] float32 or NULL, mask: [height, width]
 * bytes or NULL (0 = exclude) of the frame. counts: int32 [8]
 *   [0]  pixels with mask != 0 (all pixels with mask == NULL)
 *   [1]  CONSIDERED pixels: those of [0] with opacity > 0.5f
 *   [2]  considered pixels with |q(R_r) - q(R_f)| + |q(G_r) - q(G_f)| + |q(B_r) - q(B_f)| <= tau_colour
 *   [3]  considered pixels whose frame depth Df is finite and > 0 (0 with depth == NULL)
 *   [4]  pixels of [3] with fabsf(Dr - Df) <= tau_depth * Df, Dr the rendered depth (of a considered pixel: opacity > 0.5), every
 *        operation rounded to float32, no fused multiply-add; a comparison with a NaN on either side is false
 *   [5..7]  0
 * Ranges: width, height >= 1, width * height below 2^31, 0 <= tau_colour <= 765, tau_depth finite and >= 0. One memset node and one
 * launch on `stream`; the counters are integer atomics, one per block and counter. */
int gsr_reloc_score(int width, int height, const float* render, const float* render_depth, const float* opacity, const float* image,
                    const float* depth, const unsigned char* mask, int tau_colour, float tau_depth, int* counts, void* stream);

#ifdef __cplusplus
}
#endif

#endif
