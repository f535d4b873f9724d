// gs_jpeg_decode.h -- baseline JPEG (ITU-T T.81: 8 bit, one sequential scan; grey, 4:4:4, 4:2:2 or 4:2:0) of `frames` pictures of one size
// and sampling, decoded on the device (include/video_io.h gsr_jpeg_decode): the inverse of gs_jpeg.h, in libjpeg's default arithmetic.
// gfx950 / wave64. Four launches, no host read between them, no atomics; the same bytes in give the same bytes out:
//   jpegd_markers_kernel  one block per frame: finds the restart markers (0xFF 0xD0 .. 0xD7) of the frame's scan in byte order (count,
//                         block scan, write), so that every restart interval has its byte range
//   jpegd_entropy_kernel  one LANE per restart interval (a frame without markers is one interval): drops the stuffed 0x00, decodes the DC
//                         differences and the AC (run, size) pairs, zero-fills and writes its blocks' coefficients. DC prediction starts at
//                         0 in every interval, so the lane sums the differences itself: there is no DC pass. This is the serial part.
//   jpegd_idct_kernel     one lane per 8 x 8 block: dequantisation and jidctint.c's transform in registers -> component planes (bytes)
//   jpegd_colour_kernel   one lane per pixel: chroma upsampling (libjpeg's triangle filters) and Y Cb Cr -> R G B; its first block per frame
//                         folds the intervals' results into the frame's status
// The transform and the colour step are two launches, not one: "fancy" upsampling reads chroma samples of the neighbouring blocks, so a fused
// kernel would transform a halo of chroma blocks per tile again (22 block transforms per 16 x 16 MCU instead of 6). The planes between them
// are 1.5 bytes per pixel and stay in L2.
// Untrusted input: every loop is bounded by the interval's byte count and block count, every table index is masked to its table, and a
// frame's byte range is clamped to the scan buffer; an interval that cannot be decoded keeps what it decoded (zero elsewhere) and reports why.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "gs_jpeg.h"                         // jpeg_wave_inclusive_sum

namespace gsr {

constexpr int JPEGD_BLOCK = 256;             // markers / idct / colour
constexpr int JPEGD_ENTROPY_BLOCK = 64;      // one wave: the lanes are long serial loops, small blocks spread them over the CUs
constexpr int JPEGD_HUFF_WORDS = 96;         // one Huffman table: limit[16] | offset[16] | 256 symbols, four to a word
constexpr int JPEGD_DESC_WORDS = 8;          // restart interval | DC table of the 3 components | AC table of the 3 components | 0
constexpr int JPEGD_NO_FAILURE = 0x7fffffff;
constexpr long long JPEGD_MAX_SCAN = 1ll << 30;   // bytes of one frame's scan that are looked at
enum { JPEGD_OK = 0, JPEGD_OUT_OF_BYTES = 1, JPEGD_LONG_CODE = 2, JPEGD_INDEX_PAST_63 = 3, JPEGD_RESTART = 4 };

// zigzag position -> natural index (T.81 figure 5)
constexpr unsigned char JPEGD_ZIGZAG[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                            41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                            30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct JpegDecodeShape {
    int frames, W, H;
    int hs, vs, comps, bpm;                  // luminance blocks per MCU across and down, components, blocks per MCU
    int mcu_cols, mcus, cap;                 // cap = max_intervals: lanes, marker slots and result slots per frame
    int yW, yH, cW, cH;                      // the planes, padded to whole blocks
    int cw, ch;                              // the real chroma samples: ceil(W / hs), ceil(H / vs)
    long long scan_bytes;
};

// the byte range of a frame's scan, clamped to the buffer
__device__ __forceinline__ const unsigned char* jpegd_frame_scan(const JpegDecodeShape& s, const unsigned char* scans, const long long* offsets,
                                                                 int frame, int& n)
{
    const long long a = min(max(offsets[frame], 0ll), s.scan_bytes);
    const long long b = min(max(offsets[frame + 1], a), s.scan_bytes);
    n = (int)min(b - a, JPEGD_MAX_SCAN);
    return scans + a;
}

// restart interval and number of intervals of a frame
__device__ __forceinline__ int jpegd_intervals(const JpegDecodeShape& s, const int* desc, int& ri)
{
    ri = desc[0];
    if (ri <= 0 || ri > s.mcus) ri = s.mcus;
    return (s.mcus + ri - 1) / ri;
}

// ---- 1: restart markers, one block per frame --------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(JPEGD_BLOCK) jpegd_markers_kernel(JpegDecodeShape s, const unsigned char* __restrict__ scans,
                                                                    const long long* __restrict__ offsets, int* __restrict__ marks,
                                                                    int* __restrict__ mcount)
{
    __shared__ int s_part[JPEGD_BLOCK / 64];
    const int frame = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int n;
    const unsigned char* p = jpegd_frame_scan(s, scans, offsets, frame, n);
    int found = 0;
    for (int base = 0; base < n; base += JPEGD_BLOCK * 16) {         // (uniform trip count: the barriers inside are reached by all)
        const int off = base + (int)threadIdx.x * 16;
        uint32_t hits = 0;
        if (off < n) {
            unsigned prev = p[off];
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                if (off + j + 1 < n) {
                    const unsigned next = p[off + j + 1];
                    if (prev == 0xFFu && (next & 0xF8u) == 0xD0u) hits |= 1u << j;
                    prev = next;
                }
            }
        }
        const int c = __popc(hits);
        const int incl = jpeg_wave_inclusive_sum(c, lane);
        __syncthreads();                                             // (the previous round's readers of s_part are done)
        if (lane == 63) s_part[wave] = incl;
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < JPEGD_BLOCK / 64; ++w) {
            const int q = s_part[w];
            if (w < wave) before += q;
            total += q;
        }
        int at = found + before + incl - c;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            if ((hits >> j) & 1u) {
                if (at < s.cap) marks[(size_t)frame * s.cap + at] = off + j;
                ++at;
            }
        }
        found += total;
    }
    if (threadIdx.x == 0) mcount[frame] = found;
}

// ---- 2: entropy decoding, one lane per restart interval ------------------------------------------------------------------------------------
struct JpegdBits {
    const unsigned char* p;
    int at, end;                             // next byte, end of the interval
    uint64_t acc;                            // the low `cnt` bits are the unread bits, the next one highest
    int cnt;
};

// At most 8 rounds; every round moves `at` forward or ends the data. 0xFF 0x00 is the byte 0xFF; 0xFF before anything else ends the data.
__device__ __forceinline__ void jpegd_refill(JpegdBits& b)
{
    while (b.cnt <= 56 && b.at < b.end) {
        const unsigned v = b.p[b.at];
        if (v == 0xFFu) {
            if (b.at + 1 < b.end && b.p[b.at + 1] == 0) b.at += 2;
            else { b.at = b.end; break; }
        } else {
            ++b.at;
        }
        b.acc = (b.acc << 8) | v;
        b.cnt += 8;
    }
}

// One Huffman symbol (T.81 F.2.2.3 on 16 bits at once: limit[l - 1] is one past the largest code of length l, left-aligned), or -1 with
// `status` set. After the refill the buffer holds 57 bits or everything that is left, enough for a code and its extra bits (32 at most).
__device__ __forceinline__ int jpegd_symbol(JpegdBits& b, const int* __restrict__ table, int& status)
{
    jpegd_refill(b);
    const int peek = (int)((b.cnt >= 16 ? b.acc >> (b.cnt - 16) : b.acc << (16 - b.cnt)) & 0xFFFFu);    // zeros behind the last bit
    int len = 0;
    for (int l = 1; l <= 16; ++l)
        if (peek < table[l - 1]) { len = l; break; }
    if (len == 0 || len > b.cnt) {
        status = b.cnt < 16 ? JPEGD_OUT_OF_BYTES : JPEGD_LONG_CODE;
        return -1;
    }
    const int idx = (table[16 + len - 1] + (peek >> (16 - len))) & 255;
    b.cnt -= len;
    return (table[32 + (idx >> 2)] >> ((idx & 3) * 8)) & 0xFF;
}

// `size` (0 .. 16) extra bits as a signed value (T.81 F.2.2.1 EXTEND); false when the interval has fewer bits left
__device__ __forceinline__ bool jpegd_receive(JpegdBits& b, int size, int& v)
{
    v = 0;
    if (size == 0) return true;
    if (size > b.cnt) return false;
    v = (int)((b.acc >> (b.cnt - size)) & ((1u << size) - 1u));
    b.cnt -= size;
    if (v < (1 << (size - 1))) v -= (1 << size) - 1;
    return true;
}

__global__ void __launch_bounds__(JPEGD_ENTROPY_BLOCK) jpegd_entropy_kernel(JpegDecodeShape s, const unsigned char* __restrict__ scans,
                                                                            const long long* __restrict__ offsets, const int* __restrict__ huffman,
                                                                            const int* __restrict__ descriptors, const int* __restrict__ marks,
                                                                            const int* __restrict__ mcount, short* __restrict__ coef,
                                                                            int* __restrict__ ivfail)
{
    const long long t = (long long)blockIdx.x * JPEGD_ENTROPY_BLOCK + threadIdx.x;
    const int frame = (int)(t / s.cap), k0 = (int)(t % s.cap);
    if (frame >= s.frames) return;
    int n, ri;
    const unsigned char* p = jpegd_frame_scan(s, scans, offsets, frame, n);
    const int* desc = descriptors + (size_t)frame * JPEGD_DESC_WORDS;
    const int nint = jpegd_intervals(s, desc, ri);
    const int* mk = marks + (size_t)frame * s.cap;
    const int have = min(max(mcount[frame], 0), s.cap);              // marker slots that were written
    const int* tables = huffman + (size_t)frame * 4 * JPEGD_HUFF_WORDS;
    const int ny = s.hs * s.vs;
    int fail = JPEGD_NO_FAILURE;
    for (int iv = k0; iv < nint; iv += s.cap) {                      // (one round unless the caller's max_intervals was too small)
        const int first = iv * ri, last = min(first + ri, s.mcus);
        int status = JPEGD_OK;
        JpegdBits b = {p, 0, n, 0ull, 0};
        if (iv > 0) {                                                // the interval starts behind marker iv - 1, which must be RST((iv - 1) mod 8)
            if (iv - 1 < have) {
                const int m = mk[iv - 1];
                b.at = m + 2;
                if ((int)(p[m + 1] & 7u) != ((iv - 1) & 7)) status = JPEGD_RESTART;
            } else {
                status = JPEGD_RESTART;
            }
        }
        if (iv < have) b.end = mk[iv];
        long long pred0 = 0, pred1 = 0, pred2 = 0;
        short* out = coef + ((size_t)frame * s.mcus + first) * s.bpm * 64;
        for (int mcu = first; mcu < last; ++mcu) {
            for (int j = 0; j < s.bpm; ++j, out += 64) {
                uint4* o4 = reinterpret_cast<uint4*>(out);
#pragma unroll
                for (int i = 0; i < 8; ++i) o4[i] = make_uint4(0u, 0u, 0u, 0u);
                if (status) continue;                                // the rest of a failed interval is zero
                const int comp = j < ny ? 0 : j - ny + 1;
                const int* dct = tables + (desc[1 + comp] & 1) * JPEGD_HUFF_WORDS;
                const int* act = tables + (2 + (desc[4 + comp] & 1)) * JPEGD_HUFF_WORDS;
                int v;
                const int cat = jpegd_symbol(b, dct, status);
                if (status) continue;
                if (cat > 16) { status = JPEGD_LONG_CODE; continue; }
                if (!jpegd_receive(b, cat, v)) { status = JPEGD_OUT_OF_BYTES; continue; }
                long long dc = (comp == 0 ? pred0 : comp == 1 ? pred1 : pred2) + v;
                if (comp == 0) pred0 = dc; else if (comp == 1) pred1 = dc; else pred2 = dc;
                out[0] = (short)min(max(dc, -32768ll), 32767ll);
                int z = 1;
                while (z < 64) {                                     // z grows in every round
                    const int rs = jpegd_symbol(b, act, status);
                    if (status) break;
                    const int run = rs >> 4, size = rs & 15;
                    if (size == 0) {
                        if (run != 15) break;                        // EOB
                        z += 16;                                     // ZRL
                        continue;
                    }
                    z += run;
                    if (z > 63) { status = JPEGD_INDEX_PAST_63; break; }
                    if (!jpegd_receive(b, size, v)) { status = JPEGD_OUT_OF_BYTES; break; }
                    out[z] = (short)v;
                    ++z;
                }
                if (!status && z > 64) status = JPEGD_INDEX_PAST_63;
            }
        }
        if (status && fail == JPEGD_NO_FAILURE) fail = iv * 8 + status;
    }
    ivfail[(size_t)frame * s.cap + k0] = fail;
}

// ---- 3: dequantisation and inverse DCT, one lane per block -----------------------------------------------------------------------------------
// jidctint.c's one-dimensional pass on eight values in place: (x + bias) >> shift at the end. 32-bit two's complement; the sums are formed
// modulo 2^32 (unsigned), so a block outside the bound stated in include/video_io.h gives defined, if different, samples.
__device__ __forceinline__ void jpegd_idct_1d(uint32_t& a0, uint32_t& a1, uint32_t& a2, uint32_t& a3, uint32_t& a4, uint32_t& a5, uint32_t& a6,
                                              uint32_t& a7, uint32_t bias, int shift)
{
    auto m = [](uint32_t x, int c) { return x * (uint32_t)c; };
    uint32_t z2 = a2, z3 = a6;
    uint32_t z1 = m(z2 + z3, 4433);
    uint32_t tmp2 = z1 + m(z3, -15137), tmp3 = z1 + m(z2, 6270);
    uint32_t tmp0 = (a0 + a4) << 13, tmp1 = (a0 - a4) << 13;
    const uint32_t tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = a7; tmp1 = a5; tmp2 = a3; tmp3 = a1;
    z1 = tmp0 + tmp3; z2 = tmp1 + tmp2; z3 = tmp0 + tmp2;
    uint32_t z4 = tmp1 + tmp3;
    const uint32_t z5 = m(z3 + z4, 9633);
    tmp0 = m(tmp0, 2446); tmp1 = m(tmp1, 16819); tmp2 = m(tmp2, 25172); tmp3 = m(tmp3, 12299);
    z1 = m(z1, -7373); z2 = m(z2, -20995); z3 = m(z3, -16069) + z5; z4 = m(z4, -3196) + z5;
    tmp0 += z1 + z3; tmp1 += z2 + z4; tmp2 += z2 + z3; tmp3 += z1 + z4;
    auto d = [&](uint32_t x) { return (uint32_t)((int)(x + bias) >> shift); };
    a0 = d(tmp10 + tmp3); a7 = d(tmp10 - tmp3);
    a1 = d(tmp11 + tmp2); a6 = d(tmp11 - tmp2);
    a2 = d(tmp12 + tmp1); a5 = d(tmp12 - tmp1);
    a3 = d(tmp13 + tmp0); a4 = d(tmp13 - tmp0);
}

__global__ void __launch_bounds__(JPEGD_BLOCK) jpegd_idct_kernel(JpegDecodeShape s, const short* __restrict__ coef,
                                                                 const unsigned short* __restrict__ qtables, unsigned char* __restrict__ planes)
{
    const int blk = blockIdx.x * JPEGD_BLOCK + threadIdx.x;
    const size_t frame = blockIdx.y;
    const int blocks = s.mcus * s.bpm;
    if (blk >= blocks) return;
    const int mcu = blk / s.bpm, j = blk - mcu * s.bpm;
    const int my = mcu / s.mcu_cols, mx = mcu - my * s.mcu_cols;
    const int ny = s.hs * s.vs;
    const int comp = j < ny ? 0 : j - ny + 1;
    const size_t ysize = (size_t)s.yW * s.yH, csize = (size_t)s.cW * s.cH;
    unsigned char* plane = planes + frame * (ysize + 2 * csize) + (comp == 0 ? 0 : ysize + (size_t)(comp - 1) * csize);
    const int stride = comp == 0 ? s.yW : s.cW;
    const int bx = comp == 0 ? mx * s.hs + j % s.hs : mx, by = comp == 0 ? my * s.vs + j / s.hs : my;
    const uint4* c4 = reinterpret_cast<const uint4*>(coef + (frame * blocks + blk) * 64);
    const unsigned short* q = qtables + (frame * 3 + comp) * 64;
    uint32_t w[64];                                                  // natural order; every index below is a compile-time constant
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const uint4 v = c4[i];
        const uint32_t words[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int c = (int)(short)((words[e >> 1] >> ((e & 1) * 16)) & 0xFFFFu);
            const int nat = JPEGD_ZIGZAG[i * 8 + e];
            w[nat] = (uint32_t)(c * (int)q[nat]);
        }
    }
#pragma unroll
    for (int c = 0; c < 8; ++c)                                      // columns
        jpegd_idct_1d(w[c], w[8 + c], w[16 + c], w[24 + c], w[32 + c], w[40 + c], w[48 + c], w[56 + c], 1u << 10, 11);
#pragma unroll
    for (int r = 0; r < 8; ++r) {                                    // rows
        jpegd_idct_1d(w[8 * r], w[8 * r + 1], w[8 * r + 2], w[8 * r + 3], w[8 * r + 4], w[8 * r + 5], w[8 * r + 6], w[8 * r + 7], 1u << 17, 18);
        uint32_t lo = 0, hi = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            lo |= (uint32_t)min(max((int)w[8 * r + e] + 128, 0), 255) << (8 * e);
            hi |= (uint32_t)min(max((int)w[8 * r + 4 + e] + 128, 0), 255) << (8 * e);
        }
        *reinterpret_cast<uint2*>(plane + (size_t)(by * 8 + r) * stride + bx * 8) = make_uint2(lo, hi);
    }
}

// ---- 4: chroma upsampling, colour, status ------------------------------------------------------------------------------------------------------
// one chroma sample at pixel (x, y), still times 16 (2 x 2), 4 (2 x 1) or 1 and rounded as libjpeg's h2v2 / h2v1 "fancy" filters round
__device__ __forceinline__ int jpegd_chroma(const JpegDecodeShape& s, const unsigned char* __restrict__ c, int x, int y)
{
    if (s.hs == 1) return c[(size_t)y * s.cW + x];
    const int k = x >> 1, kn = (x & 1) ? min(k + 1, s.cw - 1) : max(k - 1, 0);
    if (s.vs == 1) {
        const unsigned char* row = c + (size_t)y * s.cW;
        return (3 * row[k] + row[kn] + ((x & 1) ? 2 : 1)) >> 2;
    }
    const int cy = y >> 1, cn = (y & 1) ? min(cy + 1, s.ch - 1) : max(cy - 1, 0);
    const unsigned char* row = c + (size_t)cy * s.cW;
    const unsigned char* near = c + (size_t)cn * s.cW;
    const int sk = 3 * row[k] + near[k], sn = 3 * row[kn] + near[kn];
    return (3 * sk + sn + ((x & 1) ? 7 : 8)) >> 4;
}

__global__ void __launch_bounds__(JPEGD_BLOCK) jpegd_colour_kernel(JpegDecodeShape s, const unsigned char* __restrict__ planes,
                                                                   const int* __restrict__ descriptors, const int* __restrict__ mcount,
                                                                   const int* __restrict__ ivfail, unsigned char* __restrict__ rgb8,
                                                                   int* __restrict__ status)
{
    __shared__ int s_min[JPEGD_BLOCK / 64];
    const size_t frame = blockIdx.y;
    if (blockIdx.x == 0) {                                           // (block-uniform) the frame's status: too many markers, else the first
        int least = JPEGD_NO_FAILURE;                                //  interval that failed
        for (int i = threadIdx.x; i < s.cap; i += JPEGD_BLOCK) least = min(least, ivfail[frame * s.cap + i]);
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) least = min(least, __shfl_xor(least, d, 64));
        if ((threadIdx.x & 63) == 0) s_min[threadIdx.x >> 6] = least;
        __syncthreads();
        if (threadIdx.x == 0) {
#pragma unroll
            for (int w = 1; w < JPEGD_BLOCK / 64; ++w) least = min(least, s_min[w]);
            int ri;
            const int nint = jpegd_intervals(s, descriptors + frame * JPEGD_DESC_WORDS, ri);
            status[frame] = mcount[frame] > nint - 1 ? JPEGD_RESTART : least == JPEGD_NO_FAILURE ? JPEGD_OK : (least & 7);
        }
    }
    const long long pix = (long long)blockIdx.x * JPEGD_BLOCK + threadIdx.x;
    if (pix >= (long long)s.W * s.H) return;
    const int y = (int)(pix / s.W), x = (int)(pix - (long long)y * s.W);
    const size_t ysize = (size_t)s.yW * s.yH, csize = (size_t)s.cW * s.cH;
    const unsigned char* base = planes + frame * (ysize + 2 * csize);
    const int Y = base[(size_t)y * s.yW + x];
    int r = Y, g = Y, b = Y;
    if (s.comps == 3) {
        const int cb = jpegd_chroma(s, base + ysize, x, y) - 128, cr = jpegd_chroma(s, base + ysize + csize, x, y) - 128;
        r = Y + ((91881 * cr + 32768) >> 16);                        // F(1.402)
        g = Y + ((-22554 * cb - 46802 * cr + 32768) >> 16);          // F(0.34414), F(0.71414)
        b = Y + ((116130 * cb + 32768) >> 16);                       // F(1.772)
    }
    unsigned char* o = rgb8 + (frame * (size_t)s.W * s.H + (size_t)pix) * 3;
    o[0] = (unsigned char)min(max(r, 0), 255);
    o[1] = (unsigned char)min(max(g, 0), 255);
    o[2] = (unsigned char)min(max(b, 0), 255);
}

}  // namespace gsr
