/*
 * video_io.h -- C ABI of the on-device picture encoders (libgs_rasterizer_hip.so): JPEG first, the lossless deflate encoder for PNG files
 * (gsr_png_encode) further down. JPEG: baseline sequential JPEG (ITU-T T.81), 8 bit, Y Cb Cr with 4:2:0
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

/*
 * The on-device deflate encoder: lossless zlib streams (RFC 1950 / 1951) of the two picture kinds gsr_frame_export produces, one complete
 * stream per view. A stream is the payload of that view's PNG IDAT chunk (slam/png.py assemble adds the signature, IHDR, the chunk framing
 * with its CRCs and IEND on the host).
 *   kind 0: 8-bit RGB [views, height, width, 3], pixel size D = 3 bytes;  kind 1: 16-bit grey [views, height, width] in the device's byte
 *   order, written most significant byte first as PNG requires, D = 2.  filter: 0 (None) or 2 (Up), the same for every row.
 *   The filtered scanlines are n = height * (width * D + 1) bytes: per row the filter type, then the row's bytes (filter 2: minus the byte
 *   above, modulo 256; the row above the first is zero). They are formed from the pixels on the fly.
 * The stream:
 *   78 01
 *   the filtered bytes in segments of GSR_PNG_SEGMENT bytes (the last may be shorter), ceil(n / GSR_PNG_SEGMENT) of them, each coded on
 *   its own: no match reaches before its segment's start. Per segment
 *     tokens: byte q >= D of the segment REPEATS when b[q] == b[q - D]. A maximal run of repeating bytes is cut into pieces of 258 from
 *       its start; a piece of 3 or more bytes is one match (its length, distance D); the 1 or 2 bytes of a shorter piece and every byte
 *       that does not repeat are literals.
 *     one deflate block, BFINAL 0, BTYPE 2 (dynamic Huffman codes from the segment's own histogram): literal/length code lengths at most
 *       15 bits, the code-length code at most 7; the distance alphabet has HDIST = D codes of which only the last (distance D) has a length,
 *       1, or, in a segment without a match, one code of length 0. Code construction: symbols ranked by (frequency, symbol); two-queue merge,
 *       a leaf before an internal node of equal weight; depths clamped to the limit and the Kraft sum repaired as zlib does; lengths dealt
 *       to the ranked symbols longest first; canonical codes. The lengths of both alphabets form one sequence, run-coded greedily: a run
 *       of zeros as 18s of up to 138, then one 17 for 3 .. 10, then single zeros; a run of a non-zero length as the length, then 16s of up
 *       to 6, then the length again for a remainder below 3.
 *     an empty stored block (000, zero bits to the next byte, 00 00 FF FF), so that every segment ends on a byte and segments join by copy
 *     a segment whose dynamic block and empty block together would take more than its stored form is written as that form: one stored
 *       block (00, LEN, ~LEN, the bytes) and the empty stored block, len + 10 bytes
 *   a final empty stored block with BFINAL set: 01 00 00 FF FF
 *   the Adler-32 of the n filtered bytes, big-endian, combined from the segments' partial sums in segment order in integer arithmetic
 * so a stream never takes more than
 *   gsr_png_stream_bound = 2 + n + 10 * ceil(n / GSR_PNG_SEGMENT) + 9 bytes.
 * The same input gives the same bytes.
 */
#define GSR_PNG_SEGMENT 16384

/* Bytes of workspace gsr_png_encode needs; 0 when the arguments are outside what it takes: views in [1, 65535], width and height
 * positive, kind 0 or 1, gsr_png_stream_bound below 2^31. */
size_t gsr_png_workspace_size(int views, int width, int height, int kind);

/* The most bytes one view's stream can take (the closed form above); 0 outside the same range. */
size_t gsr_png_stream_bound(int width, int height, int kind);

/* gsr_png_encode: pixels as above; view v's stream starts at out + v * out_stride, and out_stride must be at least
 * gsr_png_stream_bound(width, height, kind): there is no "does not fit". sizes: [views], the bytes written. workspace:
 * gsr_png_workspace_size bytes, 16-byte aligned. stream: hipStream_t or NULL. Three launches on `stream`, no host read between them. */
int gsr_png_encode(int views, int width, int height, int kind, int filter, const void* pixels, unsigned char* out, int64_t out_stride,
                   int* sizes, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif
