/*
 * video_io.h -- C ABI of the on-device picture coders (libgs_rasterizer_hip.so): the JPEG encoder first, then the JPEG decoder
 * (gsr_jpeg_decode), the lossless deflate encoder for PNG files (gsr_png_encode) further down. JPEG encoder: baseline sequential JPEG (ITU-T T.81), 8 bit, Y Cb Cr with 4:2:0
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
 * The on-device JPEG decoder, the inverse of gsr_jpeg_encode: baseline sequential JPEG (SOF0), 8 bit, ONE scan with all components, of
 * `frames` pictures of one size and sampling in one call. The host parses SOI .. SOS (slam/jpeg_decode.py) and hands over the
 * entropy-coded bytes with the tables; everything from the first bit of the scan on runs on the device. The arithmetic is libjpeg's default
 * one ("slow integer" inverse DCT, "fancy" upsampling, 16-bit fixed-point colour), which PIL and the common viewers use, so a picture an
 * encoder wrote decodes to libjpeg's bytes (tests/jpeg_decode_reference.py restates it; tests hold both against PIL):
 *   entropy     T.81 Annex F.2.2. Stuffed 0x00 after 0xFF dropped; DC prediction per component, from 0 at the start of every restart
 *               interval; AC (run, size) pairs, EOB, ZRL; coefficients in zigzag order, what is not coded is 0
 *   dequantise  coefficient * table entry, integers
 *   transform   jidctint.c: constants of 13 bits 2446, 3196, 4433, 6270, 7373, 9633, 12299, 15137, 16069, 16819, 20995, 25172; columns
 *               first, (x + 2^10) >> 11; then rows, (x + 2^17) >> 18, plus 128; clamp to 0 .. 255
 *               32-bit integers. Every intermediate value of a pass is a sum of the pass' eight inputs times integers of magnitude at most
 *               27431 < 2^15, and a column result is at most 5.56 times the column's sum of magnitudes plus 1. With A the sum of the
 *               magnitudes of a block's 64 dequantised coefficients, the column pass stays below 2^15 A and the row pass below
 *               2^15 (5.56 A + 8) + 2^17, so nothing overflows while A <= 11000. An 8 x 8 block of 8-bit samples has a DCT of
 *               Euclidean norm at most 1024; the bound leaves room for that and for quantisation error, but it is a bound on the block, not
 *               on a single coefficient: 8-bit tables and coefficients of 11 bits (the format's limits) admit A up to 64 * 2047 * 255,
 *               which no DCT of a picture produces. The device forms the sums modulo 2^32, so such a block gives defined samples that
 *               differ from libjpeg's (which computes in `long`). libjpeg also wraps samples more than 384 levels outside 0 .. 255 through
 *               a 1024-entry table where this clamps; no encoder's output reaches that either. Equality with libjpeg is therefore
 *               claimed, and tested, for files that encoders wrote, not for arbitrary coefficients.
 *   chroma      4:2:0, libjpeg's h2v2 triangle filter: per output row s = 3 * (this chroma row) + (the nearer neighbouring chroma row);
 *               the row above the first is the first, the row below the last REAL row, ceil(H / 2) - 1, is that row (block padding is
 *               not used). Even columns (3 s[x] + s[x-1] + 8) >> 4, odd columns (3 s[x] + s[x+1] + 7) >> 4; the first column is
 *               (4 s[0] + 8) >> 4, the last (4 s[last] + 7) >> 4 with last = ceil(W / 2) - 1.
 *               4:2:2, h2v1: even (3 c[x] + c[x-1] + 1) >> 2, odd (3 c[x] + c[x+1] + 2) >> 2, the first column c[0], the last c[last].
 *               4:4:4 and grey: none.
 *   colour      F(v) = int(v * 65536 + 0.5), Cb and Cr minus 128:
 *               R = Y + ((F(1.402) Cr + 32768) >> 16),  G = Y + ((-F(0.34414) Cb - F(0.71414) Cr + 32768) >> 16),
 *               B = Y + ((F(1.772) Cb + 32768) >> 16), each clamped to 0 .. 255. Grey: R = G = B = Y.
 * Blocks per MCU: grey 1; 4:4:4 Y Cb Cr; 4:2:2 Y0 Y1 Cb Cr; 4:2:0 Y00 Y01 Y10 Y11 Cb Cr. MCUs row-major.
 */
#define GSR_JPEG_GREY 0
#define GSR_JPEG_444 1
#define GSR_JPEG_422 2
#define GSR_JPEG_420 3

/* status[f] of gsr_jpeg_decode. A restart interval that cannot be decoded ends where it fails: it keeps the coefficients it decoded, the
 * rest of it is zero, and the frame reports the code of its first such interval (GSR_JPEG_BAD_RESTART first when the scan holds more
 * restart markers than its intervals need). The other intervals, and the other frames of the call, are complete. */
#define GSR_JPEG_OK 0
#define GSR_JPEG_OUT_OF_BYTES 1     /* the interval's bytes ended (or a marker stood) before its last block did */
#define GSR_JPEG_LONG_CODE 2        /* 16 bits matched no Huffman code, or a DC category above 16 */
#define GSR_JPEG_INDEX_PAST_63 3    /* a run led past coefficient 63 */
#define GSR_JPEG_BAD_RESTART 4      /* the restart marker before the interval is missing or is not RST((interval - 1) mod 8) */

/* Bytes of workspace gsr_jpeg_decode needs; 0 when the arguments are outside what it takes: frames, width and height in [1, 65535], at most
 * 1 290 000 8 x 8 blocks per frame, sampling one of GSR_JPEG_GREY .. GSR_JPEG_420, max_intervals in [1, MCUs per frame]. */
size_t gsr_jpeg_decode_workspace_size(int frames, int width, int height, int sampling, int max_intervals);

/* gsr_jpeg_decode. All pointers are device pointers.
 * scans: the entropy-coded bytes of all frames (what follows the SOS header, up to EOI), frame f in [offsets[f], offsets[f + 1]); offsets:
 * [frames + 1]; scan_bytes: the size of `scans`, to which every range is clamped (of one frame's scan at most 2^30 bytes are looked at).
 * qtables: [frames, 3, 64] 16-bit, the table of each COMPONENT in natural (row-major) order. huffman: [frames, 4, 96] int32, the tables
 * DC 0, DC 1, AC 0, AC 1, each as limit[16] (one past the largest code of length l, shifted left to 16 bits; the previous limit where no code
 * has that length), offset[16] (index of the length's first symbol minus its first code) and the 256 symbols, four to a word, lowest byte
 * first. descriptors: [frames, 8] int32: the restart interval in MCUs (0: none), the DC table (0 / 1) of the three components, their AC
 * tables, 0. max_intervals: the largest number of restart intervals of any frame, ceil(MCUs / restart interval); it sizes the launch (one
 * lane per interval) -- with a smaller value a lane decodes several intervals and those past the marker slots report
 * GSR_JPEG_BAD_RESTART.
 * rgb8: [frames, height, width, 3] bytes, the layout gsr_frame_prepare reads. status: [frames] int32, a GSR_JPEG_* code above.
 * coefficients: NULL, or 16-byte aligned [frames, mcu_rows, mcu_cols, blocks per MCU, 64] int16: the quantised coefficients in scan
 * order, zigzag, with the DC values (for 4:2:0 the layout of gsr_jpeg_encode's `coefficients`). workspace:
 * gsr_jpeg_decode_workspace_size bytes, 16-byte aligned. stream: hipStream_t or NULL. Four launches on `stream`, no host read between them,
 * no atomics; the same bytes in give the same bytes out. Nothing is read outside `scans` and the tables, nothing written outside the
 * outputs and the workspace, whatever the bytes are. */
int gsr_jpeg_decode(int frames, int width, int height, int sampling, int max_intervals, const unsigned char* scans, const int64_t* offsets,
                    int64_t scan_bytes, const unsigned short* qtables, const int* huffman, const int* descriptors, unsigned char* rgb8,
                    int* status, short* coefficients, void* workspace, size_t workspace_bytes, void* stream);

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
