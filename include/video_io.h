/*
 * video_io.h -- C ABI of the on-device JPEG encoder (libgs_rasterizer_hip.so): baseline sequential JPEG (ITU-T T.81), 8 bit, Y Cb Cr with 4:2:0
 * chroma, the Annex K Huffman tables, no restart markers, of `views` pictures in one call. The call produces each view's entropy-coded segment;
 * a file is the caller's header (SOI .. SOS: slam/mjpeg.py jfif_header) + that segment + EOI. All pointers are DEVICE pointers.
 * Returns 0 or a negative GSR_ERR_* code (gs_rasterizer.h); gsr_last_error() has the text. Nothing is enqueued on a bad argument.
 */
#ifndef VIDEO_IO_H_INCLUDED
#define VIDEO_IO_H_INCLUDED

#include <stddef.h>
#include <stdint.h>
#include "gs_rasterizer.h"   /* GSR_ERR_* */

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of workspace gsr_jpeg_encode needs for `views` pictures of width x height; 0 when the arguments are outside what it takes (views in
 * [1, 65535], width and height in [1, 65535], at most 1 290 000 8 x 8 blocks per view). */
size_t gsr_jpeg_workspace_size(int views, int width, int height);

/* gsr_jpeg_encode: per view, with the picture padded to multiples of 16 by edge replication,
 *   Y = 0.299 R + 0.587 G + 0.114 B - 128,  Cb = -0.168736 R - 0.331264 G + 0.5 B,  Cr = 0.5 R - 0.418688 G - 0.081312 B   (float32, unrounded)
 *   Cb, Cr: 0.25 * (sum of each 2 x 2);  8 x 8 orthonormal DCT-II;  coefficient = rint(F / q) (round half to even)
 *   scan: MCUs row-major, blocks Y00 Y01 Y10 Y11 Cb Cr, zigzag, DC prediction per component through the whole scan, ZRL for runs above 15,
 *   EOB unless coefficient 63 is non-zero, the last byte padded with 1-bits, 0x00 after every 0xFF.
 * rgb8: [views, height, width, 3] bytes, as gsr_frame_export writes them. qtables: [2][64] (luminance, chrominance) in zigzag order, entries
 * 1 .. 255. scan: view v's segment starts at scan + v * scan_stride and may take scan_stride bytes. sizes: [views], the bytes written, or
 * -(bytes needed) for a view that does not fit: nothing is written beyond its capacity, the other views are complete. coefficients: NULL, or
 * [views, mcu_rows, mcu_cols, 6, 64] int16, the quantised coefficients in scan order (one more store per coefficient). workspace:
 * gsr_jpeg_workspace_size bytes, 16-byte aligned. stream: hipStream_t or NULL. Four launches on `stream`, no host read between them; the
 * same input gives the same bytes. */
int gsr_jpeg_encode(int views, int width, int height, const unsigned char* rgb8, const unsigned short* qtables, unsigned char* scan,
                    int64_t scan_stride, int* sizes, short* coefficients, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif
