// gs_jpeg.h -- baseline JPEG (ITU-T T.81: 8 bit, Y Cb Cr 4:2:0, Annex K Huffman tables, no restart markers) of V views on the device
// (include/video_io.h gsr_jpeg_encode). gfx950 / wave64. A wave owns one 8 x 8 block: its 64 lanes are the block's 64 samples, then its 64
// coefficients in zigzag order, so runs of zeros come from one ballot and a block's bits from one wave prefix sum. Four launches:
//   jpeg_transform_kernel  colour conversion, 2 x 2 chroma mean, 8 x 8 DCT, quantisation, zigzag -> coefficients (int16) and the bit length
//                          of every block's AC part; the wave also zero-fills its block's share of the bit buffer
//   jpeg_offsets_kernel    one block per view: adds the DC lengths (a difference of two stored DCs) and scans the lengths to bit offsets
//   jpeg_emit_kernel       a wave assembles its block's bits in LDS (ds_or), stores whole words and merges the first and the last word, which
//                          it may share with its neighbours, with integer atomicOr: the bits are disjoint, so the order does not matter
//   jpeg_stuff_kernel      one block per view: pads the last byte with 1-bits, inserts 0x00 after every 0xFF (count, block scan, write) and
//                          reports the size; a view that does not fit its capacity writes nothing beyond it and reports -(bytes needed)
// No float atomics, no host read between the launches; the same input gives the same bytes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gsr {

constexpr int JPEG_BLOCK = 256;              // transform / emit: four waves, one 8 x 8 block each
constexpr int JPEG_WAVES = JPEG_BLOCK / 64;
constexpr int JPEG_SCAN_BLOCK = 1024;        // offsets / stuff: one block per view
constexpr int JPEG_BLOCK_WORDS = 52;         // 32-bit words of the bit buffer per 8 x 8 block: DC 9 + 11 bits, 63 AC codes of 16 + 10 bits = 1658 <= 1664
constexpr int JPEG_TAIL_WORDS = 4;           // spare words behind a view's last block (keeps 16-byte loads inside the buffer)

struct JpegTables {
    uint32_t dc[2][16];                      // (code << 8) | length by magnitude category; 0 = no such symbol
    uint32_t ac[2][256];                     // ... by (run << 4) | size
    float dct[64];                           // dct[u * 8 + x] = 1/2 C(u) cos((2x + 1) u pi / 16)
    unsigned char natural_to_zigzag[64];
};

// T.81 Annex K.3 - K.6 as (counts of the code lengths 1 .. 16, symbols in code order); codes assigned as in Annex C
constexpr unsigned char JPEG_DC_BITS[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
constexpr unsigned char JPEG_AC_BITS[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119}};
constexpr unsigned char JPEG_AC_VALS[2][162] = {
    {
     0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1,
     0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37,
     0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a,
     0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
     0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3,
     0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa},
    {
     0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1,
     0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36,
     0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69,
     0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a,
     0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca,
     0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};
constexpr float JPEG_DCT[64] = {
    0.353553391f, 0.353553391f, 0.353553391f, 0.353553391f, 0.353553391f, 0.353553391f, 0.353553391f, 0.353553391f,
    0.49039264f, 0.415734806f, 0.277785117f, 0.097545161f, -0.097545161f, -0.277785117f, -0.415734806f, -0.49039264f,
    0.461939766f, 0.191341716f, -0.191341716f, -0.461939766f, -0.461939766f, -0.191341716f, 0.191341716f, 0.461939766f,
    0.415734806f, -0.097545161f, -0.49039264f, -0.277785117f, 0.277785117f, 0.49039264f, 0.097545161f, -0.415734806f,
    0.353553391f, -0.353553391f, -0.353553391f, 0.353553391f, 0.353553391f, -0.353553391f, -0.353553391f, 0.353553391f,
    0.277785117f, -0.49039264f, 0.097545161f, 0.415734806f, -0.415734806f, -0.097545161f, 0.49039264f, -0.277785117f,
    0.191341716f, -0.461939766f, 0.461939766f, -0.191341716f, -0.191341716f, 0.461939766f, -0.461939766f, 0.191341716f,
    0.097545161f, -0.277785117f, 0.415734806f, -0.49039264f, 0.49039264f, -0.415734806f, 0.277785117f, -0.097545161f};

constexpr JpegTables jpeg_make_tables()
{
    JpegTables t = {};
    for (int k = 0; k < 2; ++k) {
        uint32_t code = 0;
        int s = 0;
        for (int len = 1; len <= 16; ++len) {                       // DC: the symbols are 0 .. 11 in order
            for (int i = 0; i < JPEG_DC_BITS[k][len - 1]; ++i) t.dc[k][s++] = (code++ << 8) | (uint32_t)len;
            code <<= 1;
        }
        code = 0;
        s = 0;
        for (int len = 1; len <= 16; ++len) {
            for (int i = 0; i < JPEG_AC_BITS[k][len - 1]; ++i) t.ac[k][JPEG_AC_VALS[k][s++]] = (code++ << 8) | (uint32_t)len;
            code <<= 1;
        }
    }
    for (int i = 0; i < 64; ++i) t.dct[i] = JPEG_DCT[i];
    int z = 0;                                                       // zigzag walk over the anti-diagonals (T.81 figure 5)
    for (int d = 0; d < 15; ++d)
        for (int i = 0; i <= d; ++i) {
            const int r = (d & 1) ? i : d - i, c = d - r;            // odd diagonals run down-left, even ones up-right
            if (r < 8 && c < 8) t.natural_to_zigzag[r * 8 + c] = (unsigned char)z++;
        }
    return t;
}

__device__ const JpegTables g_jpeg_tables = jpeg_make_tables();

struct JpegShape {
    int W, H, mcu_cols, blocks;              // blocks = 8 x 8 blocks per view = MCUs * 6
    size_t raw_words;                        // 32-bit words of a view's bit buffer
};

// index of the block whose DC predicts block b's (same component, previous in scan order), or -1 for the first of its component
__device__ __forceinline__ int jpeg_dc_predecessor(int b)
{
    const int k = b % 6;
    if (k >= 1 && k <= 3) return b - 1;
    if (b < 6) return -1;
    return k == 0 ? b - 3 : b - 6;
}

__device__ __forceinline__ int jpeg_category(int v) { return 32 - __clz(v < 0 ? -v : v); }      // 0 for 0

__device__ __forceinline__ uint32_t jpeg_dc_code(int table, int diff, int& length)
{
    const int cat = jpeg_category(diff);
    const uint32_t e = g_jpeg_tables.dc[table][cat & 15];
    length = (int)(e & 0xff) + cat;
    return ((e >> 8) << cat) | ((uint32_t)(diff < 0 ? diff - 1 : diff) & ((1u << cat) - 1u));
}

// The bits lane `lane` (= zigzag index) contributes for its coefficient c: lane 0 the DC difference; a non-zero AC coefficient its ZRLs, its
// (run, size) code and its extra bits (at most 3 * 11 + 16 + 10 = 59 bits); lane 63 with a zero coefficient the EOB. Called by whole waves.
__device__ __forceinline__ uint64_t jpeg_lane_bits(int table, int lane, int c, int dc_diff, int& length)
{
    const bool nz = lane > 0 && c != 0;
    const unsigned long long mask = __ballot(nz);
    uint64_t bits = 0;
    length = 0;
    if (lane == 0) {
        bits = jpeg_dc_code(table, dc_diff, length);
    } else if (nz) {
        const unsigned long long below = mask & ((1ull << lane) - 1ull);
        const int prev = below ? 63 - __clzll((long long)below) : 0;
        const int run = lane - prev - 1;
        const uint32_t zrl = g_jpeg_tables.ac[table][0xF0];
        for (int i = 0; i < (run >> 4); ++i) { bits = (bits << (zrl & 0xff)) | (zrl >> 8); length += (int)(zrl & 0xff); }
        const int size = jpeg_category(c);                           // <= 11 (the coefficients are clamped to +-2047)
        const uint32_t e = g_jpeg_tables.ac[table][((run & 15) << 4) | size];
        bits = (bits << (e & 0xff)) | (e >> 8);
        bits = (bits << size) | ((uint32_t)(c < 0 ? c - 1 : c) & ((1u << size) - 1u));
        length += (int)(e & 0xff) + size;
    } else if (lane == 63) {
        const uint32_t e = g_jpeg_tables.ac[table][0];
        bits = e >> 8;
        length = (int)(e & 0xff);
    }
    return bits;
}

__device__ __forceinline__ int jpeg_wave_inclusive_sum(int v, int lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(v, d, 64);
        if (lane >= d) v += o;
    }
    return v;
}

// ---- 1: pixels -> quantised coefficients ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(JPEG_BLOCK) jpeg_transform_kernel(JpegShape s, const unsigned char* __restrict__ rgb8,
                                                                    const unsigned short* __restrict__ qtables, short* __restrict__ coef,
                                                                    short* __restrict__ coef_out, uint32_t* __restrict__ lengths,
                                                                    uint32_t* __restrict__ raw)
{
    __shared__ float s_a[JPEG_WAVES][64];
    __shared__ float s_b[JPEG_WAVES][64];
    __shared__ int s_c[JPEG_WAVES][64];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int b = blockIdx.x * JPEG_WAVES + wave;
    const bool live = b < s.blocks;                                  // (every wave runs to the end: the barriers below are block-wide)
    const size_t view = blockIdx.y;
    const int bb = live ? b : 0;
    const int mcu = bb / 6, k = bb - mcu * 6;
    const int my = mcu / s.mcu_cols, mx = mcu - my * s.mcu_cols;
    const int x = lane & 7, y = lane >> 3;
    const unsigned char* img = rgb8 + view * (size_t)s.W * s.H * 3;
    auto pixel = [&](int px, int py, float& r, float& g, float& bl) {                     // edge replication
        const unsigned char* p = img + ((size_t)min(py, s.H - 1) * s.W + min(px, s.W - 1)) * 3;
        r = (float)p[0]; g = (float)p[1]; bl = (float)p[2];
    };
    float sample;
    if (k < 4) {
        float r, g, bl;
        pixel(mx * 16 + (k & 1) * 8 + x, my * 16 + (k >> 1) * 8 + y, r, g, bl);
        sample = 0.299f * r + 0.587f * g + 0.114f * bl - 128.0f;
    } else {
        float acc = 0.0f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float r, g, bl;
            pixel(mx * 16 + 2 * x + (j & 1), my * 16 + 2 * y + (j >> 1), r, g, bl);
            acc += k == 4 ? -0.168736f * r - 0.331264f * g + 0.5f * bl : 0.5f * r - 0.418688f * g - 0.081312f * bl;
        }
        sample = 0.25f * acc;
    }
    s_a[wave][lane] = sample;
    __syncthreads();
    float t = 0.0f;                                                  // rows: lane (y, u = x)
#pragma unroll
    for (int j = 0; j < 8; ++j) t += s_a[wave][y * 8 + j] * g_jpeg_tables.dct[x * 8 + j];
    s_b[wave][lane] = t;
    __syncthreads();
    float F = 0.0f;                                                  // columns: lane (v = y, u = x), natural index = lane
#pragma unroll
    for (int j = 0; j < 8; ++j) F += s_b[wave][j * 8 + x] * g_jpeg_tables.dct[y * 8 + j];
    const int table = k < 4 ? 0 : 1;
    const int z = g_jpeg_tables.natural_to_zigzag[lane];
    const float q = (float)max((int)qtables[table * 64 + z], 1);
    const float quotient = fminf(fmaxf(rintf(__fdiv_rn(F, q)), -2047.0f), 2047.0f);      // round half to even
    s_c[wave][z] = (int)quotient;
    __syncthreads();
    const int c = s_c[wave][lane];                                   // lane = zigzag index from here on
    int length;
    jpeg_lane_bits(table, lane, c, 0, length);
    const int ac_bits = jpeg_wave_inclusive_sum(lane == 0 ? 0 : length, lane);
    if (!live) return;
    const size_t at = view * (size_t)s.blocks + b;
    coef[at * 64 + lane] = (short)c;
    if (coef_out) coef_out[at * 64 + lane] = (short)c;
    if (lane == 63) lengths[at] = (uint32_t)ac_bits;
    uint32_t* words = raw + view * s.raw_words + (size_t)b * JPEG_BLOCK_WORDS;
    if (lane < JPEG_BLOCK_WORDS) words[lane] = 0u;
    if (b == s.blocks - 1 && lane < JPEG_TAIL_WORDS) words[JPEG_BLOCK_WORDS + lane] = 0u;
}

// exclusive sum over the 1024 threads of a block; `total` gets the sum of all. s_part: 16 ints. Two barriers.
__device__ __forceinline__ int jpeg_block_exclusive_sum(int v, int* s_part, int& total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int incl = jpeg_wave_inclusive_sum(v, lane);
    __syncthreads();                                                 // (the previous round's readers of s_part are done)
    if (lane == 63) s_part[wave] = incl;
    __syncthreads();
    int before = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < JPEG_SCAN_BLOCK / 64; ++w) {
        const int p = s_part[w];
        if (w < wave) before += p;
        total += p;
    }
    return before + incl - v;
}

// ---- 2: bit lengths -> bit offsets, one block per view ----------------------------------------------------------------------------------
__global__ void __launch_bounds__(JPEG_SCAN_BLOCK) jpeg_offsets_kernel(JpegShape s, const short* __restrict__ coef, uint32_t* __restrict__ lengths,
                                                                       uint32_t* __restrict__ total_bits)
{
    __shared__ int s_part[JPEG_SCAN_BLOCK / 64];
    const size_t view = blockIdx.x;
    const short* cv = coef + view * (size_t)s.blocks * 64;
    uint32_t* lv = lengths + view * (size_t)s.blocks;
    uint32_t carry = 0;
    for (int base = 0; base < s.blocks; base += JPEG_SCAN_BLOCK) {    // (uniform trip count: the barriers inside are reached by all)
        const int b = base + (int)threadIdx.x;
        int n = 0;
        if (b < s.blocks) {
            const int p = jpeg_dc_predecessor(b);
            const int diff = (int)cv[(size_t)b * 64] - (p < 0 ? 0 : (int)cv[(size_t)p * 64]);
            jpeg_dc_code(b % 6 < 4 ? 0 : 1, diff, n);
            n += (int)lv[b];
        }
        int total;
        const int before = jpeg_block_exclusive_sum(n, s_part, total);
        if (b < s.blocks) lv[b] = carry + (uint32_t)before;
        carry += (uint32_t)total;
    }
    if (threadIdx.x == 0) total_bits[view] = carry;
}

// ---- 3: coefficients -> bits at their offsets ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(JPEG_BLOCK) jpeg_emit_kernel(JpegShape s, const short* __restrict__ coef, const uint32_t* __restrict__ offsets,
                                                               uint32_t* __restrict__ raw)
{
    __shared__ uint32_t s_w[JPEG_WAVES][64];                         // 31 + 1658 bits at most: 53 words
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int b = blockIdx.x * JPEG_WAVES + wave;
    const bool live = b < s.blocks;
    const size_t view = blockIdx.y;
    const int bb = live ? b : 0;
    const short* cv = coef + view * (size_t)s.blocks * 64;
    const int c = cv[(size_t)bb * 64 + lane];
    int diff = 0;
    if (lane == 0) {
        const int p = jpeg_dc_predecessor(bb);
        diff = c - (p < 0 ? 0 : (int)cv[(size_t)p * 64]);
    }
    int n;
    const uint64_t bits = jpeg_lane_bits(bb % 6 < 4 ? 0 : 1, lane, c, diff, n);
    const int incl = jpeg_wave_inclusive_sum(n, lane);
    const int total = __shfl(incl, 63, 64);
    const uint32_t start = offsets[view * (size_t)s.blocks + bb];
    s_w[wave][lane] = 0u;
    __syncthreads();
    if (n > 0) {
        const uint32_t p = (start & 31u) + (uint32_t)(incl - n);      // bit position inside the wave's words, most significant bit first
        const uint32_t o = p & 31u;
        const uint64_t v = bits << (64 - n);                          // left-aligned
        const uint64_t hi = v >> o;
        const uint32_t w2 = o ? (uint32_t)((v << (64 - o)) >> 32) : 0u;
        uint32_t* w = &s_w[wave][p >> 5];
        if ((uint32_t)(hi >> 32)) atomicOr(w, (uint32_t)(hi >> 32));
        if ((uint32_t)hi) atomicOr(w + 1, (uint32_t)hi);              // (non-zero only when the lane's bits reach that word: <= word 53)
        if (w2) atomicOr(w + 2, w2);
    }
    __syncthreads();
    if (!live) return;
    const int words = (int)(((start & 31u) + (uint32_t)total + 31u) >> 5);
    if (lane < words) {
        const uint32_t word = __builtin_bswap32(s_w[wave][lane]);    // the stream is big-endian, memory little-endian
        uint32_t* dst = raw + view * s.raw_words + (size_t)(start >> 5) + lane;
        if (lane == 0 || lane == words - 1) { if (word) atomicOr(dst, word); }
        else *dst = word;
    }
}

// ---- 4: padding, byte stuffing, sizes; one block per view ----------------------------------------------------------------------------------
__global__ void __launch_bounds__(JPEG_SCAN_BLOCK) jpeg_stuff_kernel(JpegShape s, const uint32_t* __restrict__ raw, const uint32_t* __restrict__ total_bits,
                                                                     unsigned char* __restrict__ scan, long long scan_stride, int* __restrict__ sizes)
{
    __shared__ int s_part[JPEG_SCAN_BLOCK / 64];
    const size_t view = blockIdx.x;
    const uint32_t T = total_bits[view];
    const long long n = ((long long)T + 7) >> 3;                      // bytes before stuffing
    const unsigned pad = (T & 7u) ? (0xFFu >> (T & 7u)) : 0u;         // 1-bits behind the last bit
    const uint4* src = reinterpret_cast<const uint4*>(raw + view * s.raw_words);
    unsigned char* dst = scan + view * (size_t)scan_stride;
    long long stuffed = 0;                                            // 0x00 bytes inserted before this round
    for (long long base = 0; base < n; base += (long long)JPEG_SCAN_BLOCK * 16) {
        const long long off = base + (long long)threadIdx.x * 16;
        const int m = (int)max(0ll, min(16ll, n - off));
        uint32_t w[4] = {0u, 0u, 0u, 0u};
        if (m > 0) { const uint4 q = src[off >> 4]; w[0] = q.x; w[1] = q.y; w[2] = q.z; w[3] = q.w; }
        if (m > 0 && off + m == n) w[(m - 1) >> 2] |= pad << (((m - 1) & 3) * 8);
        int ff = 0;
#pragma unroll
        for (int j = 0; j < 16; ++j) ff += (j < m && ((w[j >> 2] >> ((j & 3) * 8)) & 0xffu) == 0xffu) ? 1 : 0;
        int total;
        const int before = jpeg_block_exclusive_sum(ff, s_part, total);
        long long at = off + stuffed + before;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            if (j < m) {
                const unsigned byte = (w[j >> 2] >> ((j & 3) * 8)) & 0xffu;
                if (at < scan_stride) dst[at] = (unsigned char)byte;
                ++at;
                if (byte == 0xffu) { if (at < scan_stride) dst[at] = 0; ++at; }
            }
        }
        stuffed += total;
    }
    if (threadIdx.x == 0) {
        const long long need = n + stuffed;
        sizes[view] = need <= scan_stride ? (int)need : (int)-need;
    }
}

}  // namespace gsr
