// gs_reloc.h -- the kernels of include/relocalisation.h: the randomised-fern code of a frame (gsr_reloc_encode), the block-wise Hamming
// search of a code in a database of codes (gsr_reloc_search) and the counts by which a rendering is judged against a frame
// (gsr_reloc_score). Everything that leaves a kernel is an integer.
//
// Encode, per call:  reloc_cells_kernel      one block per cell: the quantised colour / depth sums of its pixels, thread -> wave -> block ->
//                                            its six words of the workspace (no atomics, nothing to zero)
//                    reloc_ferns_kernel      (one block) one thread per code word: eight ferns, each four comparisons on its cell's sums
// Search, per call:  reloc_distance_kernel   2^k lanes per database row: xor, mask, the non-zero nibbles counted with popc
//                    reloc_select_kernel     (one block) per thread the topk smallest keys distance << 20 | index of its rows in its own LDS
//                                            column, then topk rounds of a block-wide minimum; the keys are distinct, so ties need no rule
// Score, per call:   reloc_score_kernel      five counters: thread -> wave -> block -> one integer atomic per block and counter
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gsr {

constexpr int RELOC_BLOCK = 256;
constexpr int RELOC_CELL_WORDS = 6;            // S_R, S_G, S_B, n, S_D, n_D
constexpr int RELOC_MAX_CELLS = 4096;
constexpr int RELOC_MAX_FERNS = 2048;          // 2048 << 20 is the largest key of the selection: it fits 32 bits
constexpr int RELOC_MAX_ROWS = 1 << 20;
constexpr int RELOC_MAX_TOPK = 16;
constexpr int RELOC_SELECT_BLOCK = 512;
constexpr int RELOC_SCORE_MAX_BLOCKS = 1024;
constexpr int RELOC_COUNTS = 8;
constexpr unsigned RELOC_NO_KEY = 0xFFFFFFFFu;

// q(v) of the header: float32 operation by operation (plain operators under contract(off): see gs_sweep.h); a NaN fails v > 0
__device__ __forceinline__ int reloc_quant(float v)
{
#pragma clang fp contract(off)
    float c = v > 0.f ? v : 0.f;
    c = c < 1.f ? c : 1.f;
    return (int)(c * 255.0f + 0.5f);
}

// dq of the header; 0 = not a valid depth
__device__ __forceinline__ int reloc_depth_quant(float d, float depth_scale)
{
#pragma clang fp contract(off)
    if (!(isfinite(d) && d > 0.f)) return 0;
    const float s = d * depth_scale;
    if (s >= 65535.f) return 65535;
    return (int)(s + 0.5f);
}

__device__ __forceinline__ unsigned reloc_wave_sum(unsigned v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

// grid: one block per cell
__global__ void __launch_bounds__(RELOC_BLOCK) reloc_cells_kernel(int W, int H, const float* __restrict__ image, const float* __restrict__ depth,
                                                                  const unsigned char* __restrict__ mask, int grid_w, int grid_h,
                                                                  float depth_scale, unsigned* __restrict__ cells)
{
    __shared__ unsigned part[RELOC_BLOCK / 64][RELOC_CELL_WORDS];
    const int cell = blockIdx.x, i = cell % grid_w, j = cell / grid_w;
    const int x0 = (int)((long long)i * W / grid_w), x1 = (int)((long long)(i + 1) * W / grid_w);
    const int y0 = (int)((long long)j * H / grid_h), y1 = (int)((long long)(j + 1) * H / grid_h);
    const int cw = x1 - x0, pixels = cw * (y1 - y0);           // cw >= 1: grid_w <= W
    const int n = W * H;                                       // below 2^23
    unsigned acc[RELOC_CELL_WORDS] = {0u, 0u, 0u, 0u, 0u, 0u};
    for (int k = threadIdx.x; k < pixels; k += RELOC_BLOCK) {
        const int p = (y0 + k / cw) * W + x0 + k % cw;
        if (mask && !mask[p]) continue;
        acc[0] += (unsigned)reloc_quant(image[p]);
        acc[1] += (unsigned)reloc_quant(image[n + p]);
        acc[2] += (unsigned)reloc_quant(image[2 * n + p]);
        acc[3] += 1u;
        const int dq = depth ? reloc_depth_quant(depth[p], depth_scale) : 0;
        if (dq > 0) {
            acc[4] += (unsigned)dq;
            acc[5] += 1u;
        }
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < RELOC_CELL_WORDS; ++k) {
        const unsigned s = reloc_wave_sum(acc[k]);
        if (lane == 0) part[wave][k] = s;
    }
    __syncthreads();
    if (threadIdx.x < RELOC_CELL_WORDS) {
        unsigned s = 0u;
        for (int wv = 0; wv < RELOC_BLOCK / 64; ++wv) s += part[wv][threadIdx.x];
        cells[(size_t)cell * RELOC_CELL_WORDS + threadIdx.x] = s;
    }
}

// S > t n in 32 bits: both sides modulo 2^32, compared as int32; an empty cell gives 0
__device__ __forceinline__ unsigned reloc_bit(unsigned S, int t, unsigned n)
{
    return (n != 0u && (int)S > (int)((unsigned)t * n)) ? 1u : 0u;
}

// one block; thread w writes word w (ferns / 8 <= RELOC_BLOCK words)
__global__ void __launch_bounds__(RELOC_BLOCK) reloc_ferns_kernel(int ferns, int cells_n, const int* __restrict__ table,
                                                                  const unsigned* __restrict__ cells, unsigned* __restrict__ code)
{
    const int word = threadIdx.x;
    if (word >= ferns / 8) return;
    unsigned out = 0u;
#pragma unroll
    for (int b = 0; b < 8; ++b) {
        const int* row = table + (size_t)(word * 8 + b) * 5;
        const unsigned* S = cells + (size_t)((unsigned)row[0] % (unsigned)cells_n) * RELOC_CELL_WORDS;
        const unsigned n = S[3], nD = S[5];
        const unsigned nibble = reloc_bit(S[0], row[1], n) | reloc_bit(S[1], row[2], n) << 1 | reloc_bit(S[2], row[3], n) << 2 |
                                reloc_bit(S[4], row[4], nD) << 3;
        out |= nibble << (4 * b);
    }
    code[word] = out;
}

// `lanes` (a power of two, at most 64) consecutive lanes share a row; a block holds RELOC_BLOCK / lanes rows
__global__ void __launch_bounds__(RELOC_BLOCK) reloc_distance_kernel(int rows, int words, int lanes, const unsigned* __restrict__ database,
                                                                     const unsigned* __restrict__ query, unsigned mask8, int* __restrict__ distance)
{
    const size_t t = (size_t)blockIdx.x * RELOC_BLOCK + threadIdx.x;
    const size_t row = t / lanes;
    const int lane = (int)(t % lanes);
    int count = 0;
    if (row < (size_t)rows) {
        const unsigned* r = database + row * words;
        for (int w = lane; w < words; w += lanes) {
            unsigned x = (r[w] ^ query[w]) & mask8;
            x = (x | x >> 1 | x >> 2 | x >> 3) & 0x11111111u;      // bit 0 of a nibble: the nibble differs
            count += __popc(x);
        }
    }
    for (int o = lanes >> 1; o > 0; o >>= 1) count += __shfl_xor(count, o, 64);     // every lane of the wave takes part
    if (lane == 0 && row < (size_t)rows) distance[row] = count;
}

// One block. best: [topk, 2] rows (index, distance); slots past `rows` hold (-1, ferns + 1).
__global__ void __launch_bounds__(RELOC_SELECT_BLOCK) reloc_select_kernel(int rows, int ferns, int topk, const int* __restrict__ distance,
                                                                          int* __restrict__ best)
{
    __shared__ unsigned list[RELOC_MAX_TOPK * RELOC_SELECT_BLOCK];      // list[s][thread]: the thread's keys, ascending in s
    __shared__ unsigned wave_min[RELOC_SELECT_BLOCK / 64];
    const int tid = threadIdx.x;
    unsigned* mine = list + tid;
    for (int s = 0; s < topk; ++s) mine[s * RELOC_SELECT_BLOCK] = RELOC_NO_KEY;
    for (int r = tid; r < rows; r += RELOC_SELECT_BLOCK) {
        const unsigned key = (unsigned)distance[r] << 20 | (unsigned)r;
        if (key >= mine[(topk - 1) * RELOC_SELECT_BLOCK]) continue;
        int s = topk - 1;
        for (; s > 0 && mine[(s - 1) * RELOC_SELECT_BLOCK] > key; --s) mine[s * RELOC_SELECT_BLOCK] = mine[(s - 1) * RELOC_SELECT_BLOCK];
        mine[s * RELOC_SELECT_BLOCK] = key;
    }
    int head = 0;
    for (int j = 0; j < topk; ++j) {
        const unsigned offer = head < topk ? mine[head * RELOC_SELECT_BLOCK] : RELOC_NO_KEY;
        unsigned m = offer;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m = min(m, (unsigned)__shfl_xor(m, o, 64));
        if ((tid & 63) == 0) wave_min[tid >> 6] = m;
        __syncthreads();
        m = wave_min[0];
#pragma unroll
        for (int wv = 1; wv < RELOC_SELECT_BLOCK / 64; ++wv) m = min(m, wave_min[wv]);
        __syncthreads();                                               // wave_min is written again in the next round
        if (offer == m && m != RELOC_NO_KEY) ++head;                   // one thread: the keys are distinct
        if (tid == 0) {
            best[2 * j] = m == RELOC_NO_KEY ? -1 : (int)(m & 0xFFFFFu);
            best[2 * j + 1] = m == RELOC_NO_KEY ? ferns + 1 : (int)(m >> 20);
        }
    }
}

// grid-stride over the pixels; counts was zeroed by a memset node
__global__ void __launch_bounds__(RELOC_BLOCK) reloc_score_kernel(size_t n, const float* __restrict__ render, const float* __restrict__ render_depth,
                                                                  const float* __restrict__ opacity, const float* __restrict__ image,
                                                                  const float* __restrict__ depth, const unsigned char* __restrict__ mask,
                                                                  int tau_colour, float tau_depth, int* counts)
{
#pragma clang fp contract(off)
    __shared__ unsigned part[RELOC_BLOCK / 64][5];
    unsigned acc[5] = {0u, 0u, 0u, 0u, 0u};
    for (size_t p = (size_t)blockIdx.x * RELOC_BLOCK + threadIdx.x; p < n; p += (size_t)gridDim.x * RELOC_BLOCK) {
        if (mask && !mask[p]) continue;
        acc[0] += 1u;
        if (!(opacity[p] > 0.5f)) continue;
        acc[1] += 1u;
        const int diff = abs(reloc_quant(render[p]) - reloc_quant(image[p])) + abs(reloc_quant(render[n + p]) - reloc_quant(image[n + p])) +
                         abs(reloc_quant(render[2 * n + p]) - reloc_quant(image[2 * n + p]));
        acc[2] += diff <= tau_colour ? 1u : 0u;
        if (!depth) continue;
        const float Df = depth[p];
        if (!(isfinite(Df) && Df > 0.f)) continue;
        acc[3] += 1u;
        const float Dr = render_depth[p];
        const float gap = fabsf(Dr - Df), bar = tau_depth * Df;
        acc[4] += gap <= bar ? 1u : 0u;
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const unsigned s = reloc_wave_sum(acc[k]);
        if (lane == 0) part[wave][k] = s;
    }
    __syncthreads();
    if (threadIdx.x < 5) {
        unsigned s = 0u;
        for (int wv = 0; wv < RELOC_BLOCK / 64; ++wv) s += part[wv][threadIdx.x];
        if (s) atomicAdd(counts + threadIdx.x, (int)s);
    }
}

}  // namespace gsr
