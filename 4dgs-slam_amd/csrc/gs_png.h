// gs_png.h -- zlib (RFC 1950 / 1951) streams of the filtered scanlines of V pictures on the device: the bytes of a PNG file's IDAT chunk
// (include/video_io.h gsr_png_encode). gfx950 / wave64. The n = H * (W * D + 1) filtered bytes of a view (filter byte + W * D bytes per row,
// filter 0 = None or 2 = Up, formed from the pixels on the fly) are cut into segments of PNG_SEG bytes, each one deflate block of its own.
// Three launches:
//   png_segment_kernel  one workgroup per (segment, view): filters its bytes into LDS, marks the bytes that repeat at distance D (a thread
//                       owns 64 consecutive bytes = one word of the repeat mask; the runs' ends beyond a word come from two block scans),
//                       cuts the runs into matches, builds the histogram, the length-limited Huffman codes and the block header in LDS,
//                       scans the tokens' bit lengths, ORs their bits into LDS words and stores the block whole into the segment's staging
//                       slot; also the segment's two Adler-32 sums
//   png_offsets_kernel  one block per view: scans the segments' sizes to offsets, combines the Adler sums in segment order, writes the zlib
//                       header, the final block, the checksum and sizes[view]
//   png_gather_kernel   one workgroup per (segment, view): moves the segment to its offset (whole words between the unaligned ends)
// Tokens (the contract in video_io.h): byte q >= D of a segment repeats when b[q] == b[q - D]; a maximal run of repeating bytes is cut
// into pieces of 258 from its start; a piece of >= 3 bytes is one match (length, distance D), everything else is a literal.
// Huffman codes: the used symbols are ranked by (frequency, symbol); two-queue merge where a leaf goes before an internal node of the same
// weight; depths are clamped to the limit and the Kraft sum is repaired as zlib and miniz do (take one leaf from the deepest level, split the
// deepest shallower leaf) until it is exactly 1; the lengths go to the ranked symbols longest first; canonical codes by symbol order. All of
// it is integer work on a fixed order: the same input gives the same bytes. No float anywhere, no host read between the launches; the LDS
// atomics are integer adds (counts) and ORs of disjoint bits, both independent of their order.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gsr {

constexpr int PNG_SEG = 16384;                   // filtered bytes per segment (GSR_PNG_SEGMENT)
constexpr int PNG_BLOCK = 256;                   // segment / gather kernels: thread t owns bytes [64 t, 64 t + 64) of the segment
constexpr int PNG_SEG_EXTRA = 10;                // worst case of a segment beyond its bytes: stored header 5 + the empty stored block 5
constexpr int PNG_SLOT = PNG_SEG + 16;           // bytes of a segment's staging slot
constexpr int PNG_OUT_WORDS = PNG_SLOT / 4 + 2;  // LDS words of the block under construction (an OR may touch one word past its bits)
constexpr int PNG_SCAN_BLOCK = 1024;             // offsets kernel: one block per view
constexpr int PNG_HEAD = 2, PNG_TAIL = 9;        // 78 01 | final empty stored block 01 00 00 FF FF + Adler-32
constexpr uint32_t PNG_ADLER = 65521u;
constexpr int PNG_SYMBOLS = 286, PNG_CL_SYMBOLS = 19;
static_assert(PNG_SEG == 64 * PNG_BLOCK, "a thread's bytes are one 64-bit word of the repeat mask");
static_assert(PNG_SEG <= 65535, "a segment's stored form is one stored block");

struct PngShape { int W, H, D, kind, filter, row, n, nseg; };     // row = W * D + 1 bytes; n = H * row; nseg = ceil(n / PNG_SEG)

__device__ const unsigned char g_png_cl_order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

// LDS index of segment byte q: 4 bytes of padding per 64, so that the threads' 64-byte strides fall on different banks
__device__ __forceinline__ int png_at(int q) { return q + ((q >> 6) << 2); }

// ---- scans over the 256 threads of a segment's workgroup (part: 4 ints; two barriers each) ------------------------------------------------
__device__ __forceinline__ int png_exclusive_max(int v, int identity, int* part)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(v, d, 64);
        if (lane >= d) v = max(v, o);
    }
    __syncthreads();
    if (lane == 63) part[wave] = v;
    __syncthreads();
    int e = __shfl_up(v, 1, 64);
    if (lane == 0) e = identity;
    for (int w = 0; w < wave; ++w) e = max(e, part[w]);
    return e;
}

__device__ __forceinline__ int png_exclusive_min_behind(int v, int identity, int* part)     // over the threads AFTER this one
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_down(v, d, 64);
        if (lane + d < 64) v = min(v, o);
    }
    __syncthreads();
    if (lane == 0) part[wave] = v;
    __syncthreads();
    int e = __shfl_down(v, 1, 64);
    if (lane == 63) e = identity;
    for (int w = wave + 1; w < PNG_BLOCK / 64; ++w) e = min(e, part[w]);
    return e;
}

__device__ __forceinline__ int png_exclusive_sum(int v, int* part, int& total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(incl, d, 64);
        if (lane >= d) incl += o;
    }
    __syncthreads();
    if (lane == 63) part[wave] = incl;
    __syncthreads();
    int before = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < PNG_BLOCK / 64; ++w) {
        const int p = part[w];
        if (w < wave) before += p;
        total += p;
    }
    return before + incl - v;
}

// ---- tokens ----------------------------------------------------------------------------------------------------------------------------
// a thread's view of the runs: the bytes of its word that do NOT repeat (bits at and beyond the segment's end are set), and the nearest
// such byte before and behind its word
struct PngRuns { unsigned long long nonrep; int base, prev, next; };

// length 3 .. 258 -> symbol 257 .. 285 and its extra bits (RFC 1951 3.2.5)
__device__ __forceinline__ int png_length_symbol(int L, int& extra, int& ebits)
{
    const int l = L - 3;
    extra = 0;
    ebits = 0;
    if (l < 8) return 257 + l;
    if (L == 258) return 285;
    ebits = 29 - __clz(l);                                          // floor(log2 l) - 2: 1 .. 5
    extra = l & ((1 << ebits) - 1);
    return 261 + 4 * ebits + ((l >> ebits) & 3);
}

// The token that starts at byte j of the thread's word: a literal 0 .. 255, a length symbol (with its extra bits), or -1 for a byte that
// lies inside a match.
__device__ __forceinline__ int png_token(const PngRuns& r, const unsigned char* s_b, int j, int& extra, int& ebits)
{
    const int q = r.base + j;
    extra = 0;
    ebits = 0;
    if ((r.nonrep >> j) & 1ull) return s_b[png_at(q)];
    const unsigned long long below = r.nonrep & ((1ull << j) - 1ull);
    const int last = below ? r.base + 63 - __clzll((long long)below) : r.prev;
    const unsigned long long above = j < 63 ? r.nonrep & (~0ull << (j + 1)) : 0ull;
    const int next = above ? r.base + __ffsll((long long)above) - 1 : r.next;
    const int k = q - (last + 1), L = next - (last + 1);             // position in the run, the run's length
    const int piece = k / 258;
    const int plen = min(258, L - piece * 258);
    if (plen < 3) return s_b[png_at(q)];
    if (k != piece * 258) return -1;
    return png_length_symbol(plen, extra, ebits);
}

// ---- Huffman codes, by the whole workgroup --------------------------------------------------------------------------------------------
// freq[n] -> len[n] (0 for an unused symbol, at most maxbits) and code[n] = (the code, bit-reversed for deflate's bit order) | len << 16.
// scratch: 1760 words of LDS. Returns the number of used symbols; below 2 nothing else is valid. Ends with a barrier.
__device__ int png_build_code(const uint32_t* freq, int n, int maxbits, unsigned char* len, uint32_t* code, uint32_t* scratch, int* s_m)
{
    uint32_t* const key = scratch;                                   // (frequency << 9) | symbol; all ones for an unused symbol
    uint32_t* const sorted = key + 288;                              // rank -> symbol
    uint32_t* const lf = sorted + 288;                               // rank -> frequency: the leaves' queue
    uint32_t* const nf = lf + 288;                                   // the internal nodes' queue, in the order they are made
    uint32_t* const par = nf + 288;                                  // parent of leaf r (index r) and of internal node j (index m + j)
    uint32_t* const blc = par + 576;                                 // leaves per code length
    uint32_t* const nxt = blc + 16;                                  // first code per code length
    const int tid = threadIdx.x;
    if (tid < 16) blc[tid] = 0u;
    if (tid == 0) *s_m = 0;
    for (int i = tid; i < n; i += PNG_BLOCK) key[i] = freq[i] ? ((freq[i] << 9) | (uint32_t)i) : 0xffffffffu;
    __syncthreads();
    int used = 0;
    for (int i = tid; i < n; i += PNG_BLOCK) {
        const uint32_t k = key[i];
        len[i] = 0;
        code[i] = 0u;
        if (k == 0xffffffffu) continue;
        int r = 0;
        for (int j = 0; j < n; ++j) r += key[j] < k ? 1 : 0;
        sorted[r] = (uint32_t)i;
        lf[r] = k >> 9;
        ++used;
    }
    if (used) atomicAdd(s_m, used);
    __syncthreads();
    const int m = *s_m;
    __syncthreads();                                                 // (s_m may be written again by the next call)
    if (m < 2) return m;
    if (tid == 0) {                                                  // two queues: the two lightest of (next leaf, next internal node), a leaf first on a tie
        int li = 0, ni = 0, nn = 0;
        for (int k = 0; k < m - 1; ++k) {
            uint32_t f = 0u;
            for (int h = 0; h < 2; ++h) {
                if (li < m && (ni >= nn || lf[li] <= nf[ni])) { par[li] = (uint32_t)(m + nn); f += lf[li++]; }
                else { par[m + ni] = (uint32_t)(m + nn); f += nf[ni++]; }
            }
            nf[nn++] = f;
        }
    }
    __syncthreads();
    const uint32_t root = (uint32_t)(2 * m - 2);
    for (int r = tid; r < m; r += PNG_BLOCK) {
        int d = 0;
        for (uint32_t x = (uint32_t)r; x != root; x = par[x]) ++d;
        atomicAdd(&blc[min(d, maxbits)], 1u);
    }
    __syncthreads();
    if (tid == 0) {
        uint32_t total = 0u;                                         // Kraft sum in units of 2^-maxbits
        for (int l = 1; l <= maxbits; ++l) total += blc[l] << (maxbits - l);
        while (total > (1u << maxbits)) {                            // each round takes exactly one unit off
            blc[maxbits] -= 1u;
            for (int l = maxbits - 1; l > 0; --l)
                if (blc[l]) { blc[l] -= 1u; blc[l + 1] += 2u; break; }
            total -= 1u;
        }
        uint32_t c = 0u;
        blc[0] = 0u;
        for (int l = 1; l <= maxbits; ++l) { c = (c + blc[l - 1]) << 1; nxt[l] = c; }
    }
    __syncthreads();
    for (int r = tid; r < m; r += PNG_BLOCK) {                       // the rarest symbols get the longest codes
        int l = maxbits, seen = 0;
        for (; l > 1; --l) {
            seen += (int)blc[l];
            if (r < seen) break;
        }
        len[sorted[r]] = (unsigned char)l;
    }
    __syncthreads();
    for (int i = tid; i < n; i += PNG_BLOCK) {
        const int l = len[i];
        if (l == 0) continue;
        uint32_t c = nxt[l];
        for (int j = 0; j < i; ++j) c += len[j] == l ? 1u : 0u;
        code[i] = (__brev(c) >> (32 - l)) | ((uint32_t)l << 16);
    }
    __syncthreads();
    return m;
}

// ---- 1: one deflate block per segment ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(PNG_BLOCK) png_segment_kernel(PngShape s, const unsigned char* __restrict__ pixels, unsigned char* __restrict__ staging,
                                                                uint32_t* __restrict__ seg_bytes, uint32_t* __restrict__ seg_sums)
{
    __shared__ unsigned char s_b[PNG_SEG + PNG_SEG / 16];            // the filtered bytes (png_at)
    __shared__ uint32_t s_out[PNG_OUT_WORDS];                        // the block's bits; before that, png_build_code's scratch
    __shared__ uint32_t s_freq[288], s_code[288], s_clfreq[20], s_clcode[20];
    __shared__ unsigned char s_len[296], s_cllen[20];                // code lengths: literal/length symbols, then the distance symbols
    __shared__ unsigned short s_cl[296];                             // the run-coded lengths: code-length symbol | extra << 8
    __shared__ int s_part[4], s_i[8];
    __shared__ uint32_t s_sum[2];
    static_assert(PNG_OUT_WORDS >= 1760, "png_build_code's scratch lies in s_out");

    const int tid = threadIdx.x;
    const int seg = blockIdx.x;
    const size_t view = blockIdx.y;
    const int g0 = seg * PNG_SEG, len = min(PNG_SEG, s.n - g0);
    const int D = s.D, rowbytes = s.row - 1;
    const unsigned char* img = pixels + view * (size_t)rowbytes * s.H;

    // the filtered bytes: the filter type at the head of every row; 16-bit samples most significant byte first
    for (int q = tid; q < PNG_SEG; q += PNG_BLOCK) {
        unsigned v = 0u;
        if (q < len) {
            const int g = g0 + q, r = g / s.row, c = g - r * s.row;
            if (c == 0) v = (unsigned)s.filter;
            else {
                const int x = s.kind ? ((c - 1) ^ 1) : c - 1;
                v = img[(size_t)r * rowbytes + x];
                if (s.filter == 2 && r > 0) v -= img[(size_t)(r - 1) * rowbytes + x];
            }
        }
        s_b[png_at(q)] = (unsigned char)v;
    }
    for (int i = tid; i < 288; i += PNG_BLOCK) s_freq[i] = 0u;
    if (tid < 20) s_clfreq[tid] = 0u;
    if (tid < 2) s_sum[tid] = 0u;
    __syncthreads();

    // the repeat mask of this thread's 64 bytes and the Adler sums: s1 = sum b[q], s2 = sum (len - q) b[q]
    PngRuns runs;
    runs.base = tid * 64;
    const int cnt = max(0, min(64, len - runs.base));
    {
        unsigned long long rep = 0ull;
        uint32_t t1 = 0u, t2 = 0u;
        for (int j = 0; j < cnt; ++j) {
            const int q = runs.base + j;
            const uint32_t b = s_b[png_at(q)];
            t1 += b;
            t2 += (uint32_t)(len - q) * b;                           // at most 64 * 16384 * 255
            if (q >= D && b == s_b[png_at(q - D)]) rep |= 1ull << j;
        }
        runs.nonrep = ~rep;
        t2 %= PNG_ADLER;
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) { t1 += __shfl_xor(t1, d, 64); t2 += __shfl_xor(t2, d, 64); }
        if ((tid & 63) == 0) { atomicAdd(&s_sum[0], t1); atomicAdd(&s_sum[1], t2); }
    }
    const int last_in = runs.nonrep ? runs.base + 63 - __clzll((long long)runs.nonrep) : -1;
    const int first_in = runs.nonrep ? runs.base + __ffsll((long long)runs.nonrep) - 1 : len;
    runs.prev = png_exclusive_max(last_in, -1, s_part);
    runs.next = min(len, png_exclusive_min_behind(first_in, len, s_part));

    // histogram
    for (int j = 0; j < cnt; ++j) {
        int extra, ebits;
        const int sym = png_token(runs, s_b, j, extra, ebits);
        if (sym >= 0) atomicAdd(&s_freq[sym], 1u);
    }
    if (tid == 0) s_freq[256] = 1u;                                  // end of block
    __syncthreads();

    const int m = png_build_code(s_freq, PNG_SYMBOLS, 15, s_len, s_code, s_out, &s_i[0]);

    // the code lengths as one sequence (literal/length, then distance), run-coded with 16 / 17 / 18
    if (tid == 0) {
        int hlit = PNG_SYMBOLS;
        while (hlit > 257 && s_len[hlit - 1] == 0) --hlit;
        const bool match = hlit > 257;
        const int hdist = match ? D : 1;                             // distance D is symbol D - 1; without a match one code of zero bits
        for (int k = 0; k < hdist; ++k) s_len[hlit + k] = 0;
        if (match) s_len[hlit + hdist - 1] = 1;
        const int total = hlit + hdist;
        int ncl = 0;
        auto put = [&](int sym, int extra) { s_cl[ncl++] = (unsigned short)(sym | (extra << 8)); s_clfreq[sym] += 1u; };
        for (int i = 0; i < total;) {
            const int v = s_len[i];
            int r = 1;
            while (i + r < total && s_len[i + r] == v) ++r;
            i += r;
            if (v == 0) {
                while (r >= 11) { const int t = min(r, 138); put(18, t - 11); r -= t; }
                if (r >= 3) { put(17, r - 3); r = 0; }
                for (; r > 0; --r) put(0, 0);
            } else {
                put(v, 0);
                --r;
                while (r >= 3) { const int t = min(r, 6); put(16, t - 3); r -= t; }
                for (; r > 0; --r) put(v, 0);
            }
        }
        s_i[1] = hlit;
        s_i[2] = hdist;
        s_i[3] = ncl;
    }
    __syncthreads();

    const int mcl = png_build_code(s_clfreq, PNG_CL_SYMBOLS, 7, s_cllen, s_clcode, s_out, &s_i[0]);

    for (int i = tid; i < PNG_OUT_WORDS; i += PNG_BLOCK) s_out[i] = 0u;
    __syncthreads();

    // the block header, by one thread: BFINAL 0, BTYPE 2, HLIT, HDIST, HCLEN, the code-length code, the run-coded lengths
    if (tid == 0) {
        uint64_t acc = 0;
        int nb = 0, w = 0;
        auto put = [&](uint32_t v, int bits) {
            acc |= (uint64_t)v << nb;
            nb += bits;
            if (nb >= 32) { s_out[w++] = (uint32_t)acc; acc >>= 32; nb -= 32; }
        };
        const int hlit = s_i[1], hdist = s_i[2], ncl = s_i[3];
        put(0u, 1);
        put(2u, 2);
        put((uint32_t)(hlit - 257), 5);
        put((uint32_t)(hdist - 1), 5);
        int hclen = 19;
        while (hclen > 4 && s_cllen[g_png_cl_order[hclen - 1]] == 0) --hclen;
        put((uint32_t)(hclen - 4), 4);
        for (int k = 0; k < hclen; ++k) put(s_cllen[g_png_cl_order[k]], 3);
        for (int k = 0; k < ncl; ++k) {
            const int e = s_cl[k], sym = e & 0xff;
            const uint32_t c = s_clcode[sym];
            put(c & 0xffffu, (int)(c >> 16));
            if (sym == 16) put((uint32_t)(e >> 8), 2);
            else if (sym == 17) put((uint32_t)(e >> 8), 3);
            else if (sym == 18) put((uint32_t)(e >> 8), 7);
        }
        if (nb) s_out[w] = (uint32_t)acc;
        s_i[4] = 32 * w + nb;                                        // at most 17 + 57 + 289 * 14 bits
    }

    // the tokens' bit lengths -> bit offsets (the barriers inside the scan also publish the header's length)
    int bits = 0;
    for (int j = 0; j < cnt; ++j) {
        int extra, ebits;
        const int sym = png_token(runs, s_b, j, extra, ebits);
        if (sym >= 0) bits += (int)(s_code[sym] >> 16) + (sym > 256 ? ebits + 1 : 0);
    }
    int total;
    const int start = png_exclusive_sum(bits, s_part, total);
    const int header_bits = s_i[4];
    const uint32_t eob = s_code[256];
    const int end_bit = header_bits + total + (int)(eob >> 16);
    const int block_bytes = (end_bit + 3 + 7) >> 3;                  // ... + the empty stored block's 3 header bits, padded to a byte
    const bool dynamic = m >= 2 && mcl >= 2 && block_bytes + 4 <= len + PNG_SEG_EXTRA;

    unsigned char* slot = staging + (view * (size_t)s.nseg + seg) * PNG_SLOT;
    int bytes;
    if (dynamic) {
        int p = header_bits + start;
        for (int j = 0; j < cnt; ++j) {
            int extra, ebits;
            const int sym = png_token(runs, s_b, j, extra, ebits);
            if (sym < 0) continue;
            const uint32_t c = s_code[sym];
            uint32_t v = c & 0xffffu;
            int nb = (int)(c >> 16);
            if (sym > 256) { v |= (uint32_t)extra << nb; nb += ebits + 1; }       // + the one distance symbol: one 0 bit
            const uint64_t x = (uint64_t)v << (p & 31);
            atomicOr(&s_out[p >> 5], (uint32_t)x);
            if ((uint32_t)(x >> 32)) atomicOr(&s_out[(p >> 5) + 1], (uint32_t)(x >> 32));
            p += nb;
        }
        if (tid == 0) {
            const int p0 = header_bits + total;
            const uint64_t x = (uint64_t)(eob & 0xffffu) << (p0 & 31);
            atomicOr(&s_out[p0 >> 5], (uint32_t)x);
            if ((uint32_t)(x >> 32)) atomicOr(&s_out[(p0 >> 5) + 1], (uint32_t)(x >> 32));
        }
        __syncthreads();
        if (tid == 0) {                                              // 000 + padding are zero already; LEN 00 00, NLEN FF FF
            unsigned char* o = reinterpret_cast<unsigned char*>(s_out);
            o[block_bytes + 2] = 0xff;
            o[block_bytes + 3] = 0xff;
        }
        __syncthreads();
        bytes = block_bytes + 4;
        uint32_t* slot32 = reinterpret_cast<uint32_t*>(slot);
        for (int i = tid; i < (bytes + 3) >> 2; i += PNG_BLOCK) slot32[i] = s_out[i];
    } else {                                                         // stored: 00 | LEN | ~LEN | the bytes, then the empty stored block
        bytes = len + PNG_SEG_EXTRA;
        if (tid < 5) slot[tid] = (unsigned char)(tid == 0 ? 0 : tid == 1 ? len & 255 : tid == 2 ? len >> 8 : tid == 3 ? ~len & 255 : (~len >> 8) & 255);
        for (int q = tid; q < len; q += PNG_BLOCK) slot[5 + q] = s_b[png_at(q)];
        if (tid < 5) slot[5 + len + tid] = (unsigned char)(tid < 3 ? 0 : 0xff);
    }
    if (tid == 0) {
        const size_t at = view * (size_t)s.nseg + seg;
        seg_bytes[at] = (uint32_t)bytes;
        seg_sums[2 * at] = s_sum[0] % PNG_ADLER;
        seg_sums[2 * at + 1] = s_sum[1] % PNG_ADLER;
    }
}

// exclusive sum over the 1024 threads of a block; `total` gets the sum of all. s_part: 16 words. Two barriers.
__device__ __forceinline__ unsigned long long png_scan_exclusive_sum(unsigned long long v, unsigned long long* s_part, unsigned long long& total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned long long o = __shfl_up(incl, d, 64);
        if (lane >= d) incl += o;
    }
    __syncthreads();
    if (lane == 63) s_part[wave] = incl;
    __syncthreads();
    unsigned long long before = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < PNG_SCAN_BLOCK / 64; ++w) {
        const unsigned long long p = s_part[w];
        if (w < wave) before += p;
        total += p;
    }
    return before + incl - v;
}

// ---- 2: sizes -> offsets, the Adler-32 of the whole, the stream's head and tail; one block per view --------------------------------------
// Over a segment of len bytes with sums (s1, s2), Adler's pair goes (A, B) -> (A + s1, B + len * A + s2) mod 65521: B needs the A in front
// of every segment, which is an exclusive sum.
__global__ void __launch_bounds__(PNG_SCAN_BLOCK) png_offsets_kernel(PngShape s, const uint32_t* __restrict__ seg_bytes, const uint32_t* __restrict__ seg_sums,
                                                                     uint32_t* __restrict__ offsets, unsigned char* __restrict__ out, long long out_stride,
                                                                     int* __restrict__ sizes)
{
    __shared__ unsigned long long s_part[PNG_SCAN_BLOCK / 64];
    const size_t view = blockIdx.x;
    const uint32_t* sb = seg_bytes + view * (size_t)s.nseg;
    const uint32_t* ss = seg_sums + view * (size_t)s.nseg * 2;
    uint32_t* off = offsets + view * (size_t)s.nseg;
    unsigned long long at = PNG_HEAD, A = 1ull, B = 0ull;
    for (int base = 0; base < s.nseg; base += PNG_SCAN_BLOCK) {      // (uniform trip count: the barriers inside are reached by all)
        const int i = base + (int)threadIdx.x;
        const bool live = i < s.nseg;
        unsigned long long total;
        const unsigned long long before = png_scan_exclusive_sum(live ? sb[i] : 0u, s_part, total);
        if (live) off[i] = (uint32_t)(at + before);
        at += total;
        const unsigned long long a_before = png_scan_exclusive_sum(live ? ss[2 * i] : 0u, s_part, total);
        const unsigned long long a_total = total;
        unsigned long long term = 0ull;
        if (live) {
            const unsigned long long len = (unsigned long long)min(PNG_SEG, s.n - i * PNG_SEG);
            term = (len * ((A + a_before) % PNG_ADLER) + ss[2 * i + 1]) % PNG_ADLER;
        }
        png_scan_exclusive_sum(term, s_part, total);
        B = (B + total) % PNG_ADLER;
        A = (A + a_total) % PNG_ADLER;
    }
    if (threadIdx.x == 0) {
        unsigned char* o = out + view * (size_t)out_stride;
        o[0] = 0x78;
        o[1] = 0x01;
        unsigned char* t = o + at;
        t[0] = 0x01; t[1] = 0x00; t[2] = 0x00; t[3] = 0xff; t[4] = 0xff;
        t[5] = (unsigned char)(B >> 8); t[6] = (unsigned char)B; t[7] = (unsigned char)(A >> 8); t[8] = (unsigned char)A;
        sizes[view] = (int)(at + PNG_TAIL);
    }
}

// ---- 3: segments to their offsets ------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(PNG_BLOCK) png_gather_kernel(PngShape s, const unsigned char* __restrict__ staging, const uint32_t* __restrict__ seg_bytes,
                                                               const uint32_t* __restrict__ offsets, unsigned char* __restrict__ out, long long out_stride)
{
    const size_t view = blockIdx.y, at = view * (size_t)s.nseg + blockIdx.x;
    const unsigned char* src = staging + at * PNG_SLOT;
    unsigned char* dst = out + view * (size_t)out_stride + offsets[at];
    const int n = (int)seg_bytes[at];
    const int head = min(n, (int)((4u - (uint32_t)(reinterpret_cast<size_t>(dst) & 3u)) & 3u));      // bytes before dst's first whole word
    const int words = (n - head) >> 2;
    const int tid = threadIdx.x;
    if (tid < head) dst[tid] = src[tid];
    const uint32_t* src32 = reinterpret_cast<const uint32_t*>(src);  // src is 16-byte aligned: the word at byte head + 4 w spans two of its words
    uint32_t* dst32 = reinterpret_cast<uint32_t*>(dst + head);
    for (int w = tid; w < words; w += PNG_BLOCK) {
        const uint64_t two = (uint64_t)src32[w] | ((uint64_t)src32[w + 1] << 32);     // (src32[w + 1] lies inside the slot: n <= PNG_SLOT - 6)
        dst32[w] = (uint32_t)(two >> (8 * head));
    }
    const int done = head + 4 * words;
    if (tid < n - done) dst[done + tid] = src[done + tid];
}

}  // namespace gsr
