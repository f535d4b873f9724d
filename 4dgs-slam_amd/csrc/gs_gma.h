// gs_gma.h -- the GMA-specific hot path of the optical-flow estimator (include/optical_flow.h): the attention of GMA/gma.py Attention
// (one head, content only) over all N = h * w low-resolution pixels of image 1, and Aggregate's attn @ v with the gamma residual that
// every iteration of the update block runs. gfx950 / wave64. Both products follow raft_corr_kernel (gs_raft.h): a 64 x 64 tile per
// block, v_mfma_f32_16x16x4_f32 (exact f32 products, each element reduced over k in one order by one block), guarded edges. No atomics.
//
// attention: sim[i][j] = sum_c (scale q[c][i]) k[c][j], then per row in place: m = max_j, e_j = expf(sim_j - m), attn_j = e_j / sum e.
//            The row maximum and sum are reduced in a fixed order: thread t of 256 over j = t, t + 256, ... ascending, then a tree over t.
// aggregate: out[c][i] = x[c][i] + gamma * sum_j attn[i][j] v[c][j]: j in four interleaved partial sums (s_g over the j with
//            j / 32 mod 4 = g, ascending), added as (s0 + s1) + (s2 + s3): four wave groups of one block, and a quarter of the chain length.
// The batch index (one of the two directions of a pair) is blockIdx.z and only offsets the pointers: a batch-2 launch computes the bits
// of two batch-1 launches.
#pragma once
#include <hip/hip_runtime.h>

namespace gsr {

constexpr int GMA_TILE = 64;                      // a block's tile: four waves of 32 x 32 (2 x 2 MFMA 16 x 16 blocks each)
constexpr int GMA_BLOCK = 256;
constexpr int GMA_MAX_BATCH = 2;
constexpr int GMA_SIM_KC = 16;                    // sim: channel rows staged per step, [k][pixel] as raft_corr_kernel
constexpr int GMA_SIM_STRIDE = GMA_TILE + 16;
constexpr int GMA_AGG_KC = 32;                    // aggregate: j columns staged per step, [row][k]: both operands have k contiguous in memory
constexpr int GMA_AGG_STRIDE = GMA_AGG_KC + 1;
constexpr int GMA_AGG_SUMS = 4;                   // aggregate: interleaved partial sums over j per output element, one wave group each
constexpr int GMA_AGG_THREADS = GMA_AGG_SUMS * GMA_BLOCK;
static_assert(GMA_AGG_SUMS == 4 && GMA_AGG_KC == 32 && GMA_TILE == 64 && GMA_BLOCK == 256, "the epilogue adds four partial sums; the staging map");
static_assert((GMA_AGG_SUMS - 1) * 16 * GMA_BLOCK <= GMA_AGG_SUMS * 2 * GMA_TILE * GMA_AGG_STRIDE, "the parked sums fit the staging tiles");

typedef float gma_f32x4 __attribute__((ext_vector_type(4)));

// q, k: [batch, D, N]; sim: [batch, N, N], row i a pixel of q
__global__ void __launch_bounds__(GMA_BLOCK) gma_sim_kernel(int D, int N, const float* __restrict__ q, const float* __restrict__ k, float scale,
                                                            float* __restrict__ sim)
{
    __shared__ float sA[GMA_SIM_KC * GMA_SIM_STRIDE];
    __shared__ float sB[GMA_SIM_KC * GMA_SIM_STRIDE];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int i0 = blockIdx.y * GMA_TILE, j0 = blockIdx.x * GMA_TILE;
    const int wr = (wave >> 1) * 32, wc = (wave & 1) * 32;
    q += (size_t)blockIdx.z * D * N;
    k += (size_t)blockIdx.z * D * N;
    sim += (size_t)blockIdx.z * N * N;
    gma_f32x4 acc[2][2];
    for (int a = 0; a < 2; ++a)
        for (int b = 0; b < 2; ++b) acc[a][b] = gma_f32x4{0.f, 0.f, 0.f, 0.f};
    // staging: thread t loads channel row t / 16 of the chunk, pixels 4 (t % 16) .. +3 of both tiles (zero outside [0, N) and [0, D));
    // q is multiplied by the scale here, before the product, as the reference does
    const int lk = t >> 4, lc = (t & 15) * 4;
    for (int k0 = 0; k0 < D; k0 += GMA_SIM_KC) {
        const int c = k0 + lk;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int i = i0 + lc + e, j = j0 + lc + e;
            sA[lk * GMA_SIM_STRIDE + lc + e] = (c < D && i < N) ? __fmul_rn(scale, q[(size_t)c * N + i]) : 0.f;
            sB[lk * GMA_SIM_STRIDE + lc + e] = (c < D && j < N) ? k[(size_t)c * N + j] : 0.f;
        }
        __syncthreads();
        // 16x16x4 operand map: lane l holds A[row l & 15][k l >> 4] and B[k l >> 4][col l & 15]
#pragma unroll
        for (int s = 0; s < GMA_SIM_KC / 4; ++s) {
            const int kr = (4 * s + (lane >> 4)) * GMA_SIM_STRIDE;
            float a[2], b[2];
#pragma unroll
            for (int m = 0; m < 2; ++m) {
                a[m] = sA[kr + wr + 16 * m + (lane & 15)];
                b[m] = sB[kr + wc + 16 * m + (lane & 15)];
            }
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int n = 0; n < 2; ++n) acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[m], b[n], acc[m][n], 0, 0, 0);
        }
        __syncthreads();
    }
    // C/D map: col = lane & 15, row = 4 (lane >> 4) + r
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n) {
            const int j = j0 + wc + 16 * n + (lane & 15);
            const int ib = i0 + wr + 16 * m + 4 * (lane >> 4);
            if (j >= N) continue;
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (ib + r < N) sim[(size_t)(ib + r) * N + j] = acc[m][n][r];
        }
}

// softmax of every row of [batch, N, N] in place, one block per row
__global__ void __launch_bounds__(GMA_BLOCK) gma_softmax_kernel(int N, float* __restrict__ attn)
{
    __shared__ float red[GMA_BLOCK];
    const int t = threadIdx.x;
    float* row = attn + ((size_t)blockIdx.y * N + blockIdx.x) * N;
    float mx = -INFINITY;
    for (int j = t; j < N; j += GMA_BLOCK) mx = fmaxf(mx, row[j]);
    red[t] = mx;
    __syncthreads();
    for (int off = GMA_BLOCK / 2; off > 0; off >>= 1) {
        if (t < off) red[t] = fmaxf(red[t], red[t + off]);
        __syncthreads();
    }
    mx = red[0];
    __syncthreads();
    float sum = 0.f;
    for (int j = t; j < N; j += GMA_BLOCK) {
        const float e = expf(__fsub_rn(row[j], mx));
        row[j] = e;
        sum = __fadd_rn(sum, e);
    }
    red[t] = sum;
    __syncthreads();
    for (int off = GMA_BLOCK / 2; off > 0; off >>= 1) {
        if (t < off) red[t] = __fadd_rn(red[t], red[t + off]);
        __syncthreads();
    }
    sum = red[0];
    for (int j = t; j < N; j += GMA_BLOCK) row[j] = __fdiv_rn(row[j], sum);      // thread t rereads only what it wrote
}

// attn: [batch, N, N]; v, x, out: [batch, D, N]. The accumulator tile has the channel on its rows and the pixel i on its columns, so a
// 16-lane group stores 16 consecutive pixels of one channel. A block is four groups of four waves; every group owns the whole 64 x 64
// tile for its share of j -- group g the 32-column chunks g, g + 4, g + 8, ... -- with LDS tiles of its own, so a CU has four waves per
// SIMD and four chunks in flight although the output has only one tile per CU. A thread holds its next chunk in registers while the block
// multiplies the current one. At the end groups 1 to 3 park their sums in LDS and group 0 adds them as (s0 + s1) + (s2 + s3).
__global__ void __launch_bounds__(GMA_AGG_THREADS) gma_aggregate_kernel(int D, int N, const float* __restrict__ attn, const float* __restrict__ v,
                                                                        const float* __restrict__ x, float gamma, float* __restrict__ out)
{
    __shared__ float lds[GMA_AGG_SUMS * 2 * GMA_TILE * GMA_AGG_STRIDE];
    const int grp = threadIdx.x / GMA_BLOCK, t = threadIdx.x % GMA_BLOCK, lane = t & 63, wave = t >> 6;
    float* sV = lds + grp * 2 * GMA_TILE * GMA_AGG_STRIDE;
    float* sP = sV + GMA_TILE * GMA_AGG_STRIDE;
    const int c0 = blockIdx.y * GMA_TILE, i0 = blockIdx.x * GMA_TILE;
    const int wr = (wave >> 1) * 32, wc = (wave & 1) * 32;
    attn += (size_t)blockIdx.z * N * N;
    v += (size_t)blockIdx.z * D * N;
    x += (size_t)blockIdx.z * D * N;
    out += (size_t)blockIdx.z * D * N;
    gma_f32x4 acc[2][2];
    for (int a = 0; a < 2; ++a)
        for (int b = 0; b < 2; ++b) acc[a][b] = gma_f32x4{0.f, 0.f, 0.f, 0.f};
    // staging: thread t of a group loads column j = t % 32 of the group's chunk in rows t / 32, t / 32 + 8, ... of both tiles (a channel
    // of v, a pixel i of attn), so one load of a wave reads two rows of 128 contiguous bytes (zero outside [0, D), [0, N): a chunk past
    // the end of the row adds zeros). Nothing outside the tensors is dereferenced.
    const int lr = t >> 5, lj = t & 31;
    const float* vrow = v + (size_t)(c0 + lr) * N;
    const float* prow = attn + (size_t)(i0 + lr) * N;
    const size_t rstep = (size_t)8 * N;
    const int rounds = (N + GMA_AGG_SUMS * GMA_AGG_KC - 1) / (GMA_AGG_SUMS * GMA_AGG_KC);
    float rv[8], rp[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int j = grp * GMA_AGG_KC + lj;
        rv[e] = (c0 + lr + 8 * e < D && j < N) ? vrow[e * rstep + j] : 0.f;
        rp[e] = (i0 + lr + 8 * e < N && j < N) ? prow[e * rstep + j] : 0.f;
    }
    for (int n = 0; n < rounds; ++n) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            sV[(lr + 8 * e) * GMA_AGG_STRIDE + lj] = rv[e];
            sP[(lr + 8 * e) * GMA_AGG_STRIDE + lj] = rp[e];
        }
        __syncthreads();
        if (n + 1 < rounds) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int j = ((n + 1) * GMA_AGG_SUMS + grp) * GMA_AGG_KC + lj;
                rv[e] = (c0 + lr + 8 * e < D && j < N) ? vrow[e * rstep + j] : 0.f;
                rp[e] = (i0 + lr + 8 * e < N && j < N) ? prow[e * rstep + j] : 0.f;
            }
        }
        // 16x16x4 operand map: lane l holds A[row l & 15][k l >> 4] (v) and B[k l >> 4][col l & 15] (attn transposed)
#pragma unroll
        for (int s = 0; s < GMA_AGG_KC / 4; ++s) {
            const int kc = 4 * s + (lane >> 4);
            float a[2], b[2];
#pragma unroll
            for (int m = 0; m < 2; ++m) {
                a[m] = sV[(wr + 16 * m + (lane & 15)) * GMA_AGG_STRIDE + kc];
                b[m] = sP[(wc + 16 * m + (lane & 15)) * GMA_AGG_STRIDE + kc];
            }
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int q = 0; q < 2; ++q) acc[m][q] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[m], b[q], acc[m][q], 0, 0, 0);
        }
        __syncthreads();
    }
    // the staging tiles are free now: groups 1 to 3 park their 16 sums per thread at [group - 1][register][t]
    if (grp > 0) {
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int q = 0; q < 2; ++q)
#pragma unroll
                for (int r = 0; r < 4; ++r) lds[((grp - 1) * 16 + (m * 2 + q) * 4 + r) * GMA_BLOCK + t] = acc[m][q][r];
    }
    __syncthreads();
    if (grp > 0) return;
    // C/D map: col = lane & 15 (pixel), row = 4 (lane >> 4) + r (channel)
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int i = i0 + wc + 16 * q + (lane & 15);
            const int cb = c0 + wr + 16 * m + 4 * (lane >> 4);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int e = ((m * 2 + q) * 4 + r) * GMA_BLOCK + t;
                const float sum = __fadd_rn(__fadd_rn(acc[m][q][r], lds[e]), __fadd_rn(lds[16 * GMA_BLOCK + e], lds[32 * GMA_BLOCK + e]));
                if (i < N && cb + r < D) {
                    const size_t o = (size_t)(cb + r) * N + i;
                    out[o] = __fadd_rn(x[o], __fmul_rn(gamma, sum));
                }
            }
        }
}

}  // namespace gsr
