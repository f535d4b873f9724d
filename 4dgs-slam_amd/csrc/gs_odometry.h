// gs_odometry.h -- the kernels of include/visual_odometry.h: an intensity / depth pyramid of one frame (gsr_odometry_pyramid) and the dense
// photometric alignment of a previous pyramid (intensity and depth) against a current one (intensity) by a coarse-to-fine, Student-t
// weighted Gauss-Newton on SE(3) (gsr_odometry_align). gsr_odometry_align_rgbd's kernels, with an affine brightness and an inverse-depth
// term, follow at the end of the file under their own heading.
//
// Pyramid, per call:  odo_level0_kernel                     luma, the depth kept where it is usable, the count of kept depths (integer atomic)
//                     odo_down_kernel        per level      2 x 2 mean of the intensity, smallest non-zero depth
// Align, per call:    odo_init_kernel        (one wave)     T <- T_init or identity, sigma <- sigma_init
//   per pass:         odo_sums_kernel                       warp, sample, Jacobian, weight; the 30 sums in double: thread -> wave -> block ->
//                                                           its row of the slab
//                     odo_solve_kernel       (one block)    adds the slab in row order, Cholesky in double, T <- exp(xi) T, the next sigma
//   after the last:   odo_finish_kernel      (one wave)     the acceptance gate, T and stats
// The slab is written by one launch and read by the next: the kernel boundary is the only ordering between blocks. The slab sum, the solve
// and exp are gs_motion.h's. The only atomic is the integer count of the pyramid; every floating-point sum has one fixed order.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "gs_motion.h"

namespace gsr {

constexpr int ODO_BLOCK = MOTION_BLOCK;        // motion_slab_sum strides by it
constexpr int ODO_MAX_LEVELS = 6;
constexpr int ODO_MIN_COARSEST = 8;            // the coarsest level has at least this many pixels either way
constexpr int ODO_MAX_BLOCKS = MOTION_MAX_BLOCKS;
constexpr int ODO_SUMS = 30;                   // 21 of H (upper triangle, row-major), 6 of g, sum w, sum w r^2, pixels in
constexpr int ODO_MIN_IN = 6;                  // fewer pixels in: no step
constexpr float ODO_MIN_Z = 1e-3f;
constexpr int ODO_STATS = 8;

// the head of a pyramid buffer (zeroed by a memset node before the level-0 launch)
struct OdoPyramidHead { int valid0; int pad[3]; };

// what the launches of one alignment hand to each other (the head of the workspace; written in full by odo_init_kernel)
struct OdoHead {
    double T[16];
    double sigma, last_xi, n_last;
    int bad_init, pad;
};

struct OdoLevel {
    int w, h;
    float fx, fy, cx, cy;
    const float* P_I;      // previous frame: intensity and depth of this level
    const float* P_D;
    const float* C_I;      // current frame: intensity
};

__global__ void __launch_bounds__(ODO_BLOCK) odo_level0_kernel(int W, int H, const float* __restrict__ image, const float* __restrict__ depth,
                                                               const unsigned char* __restrict__ mask, float depth_min, float depth_max,
                                                               float* __restrict__ I, float* __restrict__ D, OdoPyramidHead* head)
{
    // contraction off: the luma rounds after every operation, as the header's float32 statement does (plain operators: see gs_sweep.h)
#pragma clang fp contract(off)
    const size_t n = (size_t)W * H;
    const size_t p = (size_t)blockIdx.x * ODO_BLOCK + threadIdx.x;
    bool valid = false;
    if (p < n) {
        const float r = image[p], g = image[n + p], b = image[2 * n + p];
        I[p] = (0.299f * r + 0.587f * g) + 0.114f * b;
        const float d = depth ? depth[p] : 0.f;
        valid = isfinite(d) && d > 0.f && d >= depth_min && d <= depth_max && (!mask || mask[p]);
        D[p] = valid ? d : 0.f;
    }
    motion_count(valid, &head->valid0);
}

// level l + 1 [h, w] from level l [.., sw]: an odd last row or column of the source is not read
__global__ void __launch_bounds__(ODO_BLOCK) odo_down_kernel(int w, int h, int sw, const float* __restrict__ Is, const float* __restrict__ Ds,
                                                             float* __restrict__ Id, float* __restrict__ Dd)
{
#pragma clang fp contract(off)
    const size_t p = (size_t)blockIdx.x * ODO_BLOCK + threadIdx.x;
    if (p >= (size_t)w * h) return;
    const int u = (int)(p % w), v = (int)(p / w);
    const size_t s = (size_t)(2 * v) * sw + 2 * u;
    Id[p] = ((Is[s] + Is[s + 1]) + (Is[s + sw] + Is[s + sw + 1])) * 0.25f;
    const float d[4] = {Ds[s], Ds[s + 1], Ds[s + sw], Ds[s + sw + 1]};
    float m = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (d[k] > 0.f && (m == 0.f || d[k] < m)) m = d[k];
    Dd[p] = m;
}

__global__ void __launch_bounds__(64) odo_init_kernel(const float* __restrict__ T_init, float sigma_init, OdoHead* head)
{
    const int k = threadIdx.x;
    const float v = (T_init && k < 12) ? T_init[k] : ((k % 5) == 0 ? 1.f : 0.f);        // the last row is 0 0 0 1 whatever T_init holds
    const bool bad = __ballot(k < 16 && !isfinite(v)) != 0ull;
    if (k < 16) head->T[k] = bad ? ((k % 5) == 0 ? 1.0 : 0.0) : (double)v;
    if (k == 0) {
        head->sigma = (double)sigma_init;
        head->last_xi = 0.0;
        head->n_last = 0.0;
        head->bad_init = bad ? 1 : 0;
        head->pad = 0;
    }
}

// grid: blocks of the level (a function of its size alone), grid-stride over the level's pixels in linear order
__global__ void __launch_bounds__(ODO_BLOCK) odo_sums_kernel(OdoLevel L, float nu, const OdoHead* __restrict__ head, double* __restrict__ slab)
{
    __shared__ double part[ODO_BLOCK / 64][ODO_SUMS];
    float R[9], t[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) R[3 * i + j] = (float)head->T[4 * i + j];
        t[i] = (float)head->T[4 * i + 3];
    }
    const float sigma = (float)head->sigma;
    const float xmax = (float)(L.w - 2), ymax = (float)(L.h - 2);
    double acc[ODO_SUMS];
#pragma unroll
    for (int k = 0; k < ODO_SUMS; ++k) acc[k] = 0.0;
    const size_t n = (size_t)L.w * L.h;
    for (size_t p = (size_t)blockIdx.x * ODO_BLOCK + threadIdx.x; p < n; p += (size_t)gridDim.x * ODO_BLOCK) {
        const float d = L.P_D[p];
        if (!(d > 0.f)) continue;
        const int u = (int)(p % L.w), v = (int)(p / L.w);
        const float X0 = ((float)u - L.cx) / L.fx * d, X1 = ((float)v - L.cy) / L.fy * d;
        const float Y0 = R[0] * X0 + R[1] * X1 + R[2] * d + t[0];
        const float Y1 = R[3] * X0 + R[4] * X1 + R[5] * d + t[1];
        const float Y2 = R[6] * X0 + R[7] * X1 + R[8] * d + t[2];
        if (!(Y2 > ODO_MIN_Z)) continue;
        const float iz = 1.f / Y2;
        const float x = L.fx * Y0 * iz + L.cx, y = L.fy * Y1 * iz + L.cy;
        if (!(x >= 1.f && x < xmax && y >= 1.f && y < ymax)) continue;      // the 4 x 4 patch below lies inside the level
        const int x0 = (int)floorf(x), y0 = (int)floorf(y);
        const float ax = x - (float)x0, ay = y - (float)y0;
        const float* c0 = L.C_I + (size_t)(y0 - 1) * L.w + (x0 - 1);
        const float* c1 = c0 + L.w;
        const float* c2 = c1 + L.w;
        const float* c3 = c2 + L.w;
        const float c01 = c0[1], c02 = c0[2];
        const float c10 = c1[0], c11 = c1[1], c12 = c1[2], c13 = c1[3];
        const float c20 = c2[0], c21 = c2[1], c22 = c2[2], c23 = c2[3];
        const float c31 = c3[1], c32 = c3[2];
        const float bx = 1.f - ax, by = 1.f - ay;
        const float Cs = by * (bx * c11 + ax * c12) + ay * (bx * c21 + ax * c22);
        // central differences at the four corners, sampled like the intensity
        const float gx = by * (bx * (0.5f * (c12 - c10)) + ax * (0.5f * (c13 - c11))) + ay * (bx * (0.5f * (c22 - c20)) + ax * (0.5f * (c23 - c21)));
        const float gy = by * (bx * (0.5f * (c21 - c01)) + ax * (0.5f * (c22 - c02))) + ay * (bx * (0.5f * (c31 - c11)) + ax * (0.5f * (c32 - c12)));
        const float r = Cs - L.P_I[p];
        const float q = r / sigma;
        const float w = (nu + 1.f) / (nu + q * q);
        // G d pi / d Y [I | -[Y]x]: the residual against a left perturbation xi = [rho | theta]
        const float a = gx * L.fx * iz, b = gy * L.fy * iz, xz = Y0 * iz, yz = Y1 * iz;
        float J[6];
        J[0] = a;
        J[1] = b;
        J[2] = -(a * xz + b * yz);
        J[3] = -a * xz * Y1 - b * (Y2 + yz * Y1);
        J[4] = a * (Y2 + xz * Y0) + b * yz * Y0;
        J[5] = -a * Y1 + b * Y0;
        int k = 0;
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
            for (int j = i; j < 6; ++j) acc[k++] += (double)(w * (J[i] * J[j]));
#pragma unroll
        for (int i = 0; i < 6; ++i) acc[21 + i] += (double)(w * (J[i] * r));
        acc[27] += (double)w;
        acc[28] += (double)(w * (r * r));
        acc[29] += 1.0;
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < ODO_SUMS; ++k) {
        const double s = motion_wave_sum(acc[k]);
        if (lane == 0) part[wave][k] = s;
    }
    __syncthreads();
    if (threadIdx.x < MOTION_ROW) {
        double s = 0.0;
        if (threadIdx.x < ODO_SUMS)
            for (int wv = 0; wv < ODO_BLOCK / 64; ++wv) s += part[wv][threadIdx.x];
        slab[(size_t)blockIdx.x * MOTION_ROW + threadIdx.x] = s;
    }
}

// One block. The pass's sums, its step, and the scale the next pass weighs with.
__global__ void __launch_bounds__(ODO_BLOCK) odo_solve_kernel(int rows, const double* __restrict__ slab, OdoHead* head, float sigma_min, int level,
                                                              double* __restrict__ trace_row)
{
    __shared__ double tile[MOTION_SLAB_TILE * MOTION_ROW];
    __shared__ double sums[MOTION_ROW];
    __shared__ MotionSolveLds S;
    const double s = motion_slab_sum(rows, slab, tile);
    if (threadIdx.x < MOTION_ROW) sums[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x != 0) return;
    sums[30] = head->sigma;                                     // the scale this pass used
    sums[31] = (double)level;
    if (trace_row)
        for (int k = 0; k < MOTION_ROW; ++k) trace_row[k] = sums[k];
    const double n = sums[29];
    head->n_last = n;
    double step = INFINITY;                                     // a pass without a step never passes the gate
    if (n >= (double)ODO_MIN_IN && motion_gauss_newton_step(sums, head->T, S)) {
        double q = 0.0;
        for (int i = 0; i < 6; ++i) q += S.xi[i] * S.xi[i];
        step = sqrt(q);
    }
    head->last_xi = step;
    if (n > 0.0) head->sigma = fmax((double)sigma_min, sqrt(sums[28] / n));
}

// One wave; thread 0 decides. T_out is the aligned motion when accepted, identity otherwise.
__global__ void __launch_bounds__(64) odo_finish_kernel(const OdoHead* __restrict__ head, const OdoPyramidHead* __restrict__ prev, float min_share,
                                                        float max_last_step, float max_translation, float max_rotation,
                                                        float* __restrict__ T_out, double* __restrict__ stats)
{
    if (threadIdx.x != 0) return;
    const double* T = head->T;
    const int valid0 = prev->valid0;
    const double share = valid0 > 0 ? head->n_last / (double)valid0 : 0.0;
    const double tn = sqrt(T[3] * T[3] + T[7] * T[7] + T[11] * T[11]);
    const double sx = T[9] - T[6], sy = T[2] - T[8], sz = T[4] - T[1];
    const double angle = atan2(0.5 * sqrt(sx * sx + sy * sy + sz * sz), 0.5 * (T[0] + T[5] + T[10] - 1.0));
    bool finite = true;
    for (int k = 0; k < 12; ++k) finite = finite && isfinite(T[k]);
    const bool accepted = !head->bad_init && finite && share >= (double)min_share && head->last_xi <= (double)max_last_step &&
                          tn <= (double)max_translation && angle <= (double)max_rotation;
    for (int k = 0; k < 16; ++k) T_out[k] = accepted ? (float)T[k] : ((k % 5) == 0 ? 1.f : 0.f);
    stats[0] = accepted ? 1.0 : 0.0;
    stats[1] = share;
    stats[2] = head->sigma;
    stats[3] = head->last_xi;
    stats[4] = head->n_last;
    stats[5] = tn;
    stats[6] = angle;
    stats[7] = (double)valid0;
}

// ---- gsr_odometry_align_rgbd: the photometric term with an affine brightness (alpha, beta) and an inverse-depth term ---------------------
// Align, per call:    odo_rgbd_init_kernel   (one wave)     T <- T_init or identity, both sigmas, alpha = beta = 0
//   per pass:         odo_rgbd_sums_kernel<AFFINE, DEPTH>   both terms of a pixel in float32; the NH + N + 6 sums in double (N = 6 or 8 unknowns,
//                                                           NH = N (N + 1) / 2): thread -> wave -> block -> its row of the slab
//                     odo_rgbd_solve_kernel<N> (one block)  adds the slab in row order, Cholesky in double, T <- exp(xi) T, alpha, beta, the sigmas
//   after the last:   odo_rgbd_finish_kernel (one wave)     the gate, T and stats
// AFFINE = false carries no sum of the two brightness columns and DEPTH = false reads no depth of the current frame.
constexpr int ODO_RGBD_ROW = 64;               // doubles per slab row and per trace row
constexpr int ODO_RGBD_TAIL = 6;               // sum w_I, sum w_I r_I^2, n_I, sum w_D, sum w_D r_D^2, n_D
constexpr int ODO_RGBD_STATS = 12;
constexpr int ODO_RGBD_SLAB_TILE = 64;         // rows staged in LDS at a time

struct OdoRgbdHead {
    double T[16];
    double sigma_i, sigma_d, last_xi, n_last, nd_last, alpha, beta;
    int bad_init, pad;
};

struct OdoRgbdLevel {
    int w, h;
    float fx, fy, cx, cy;
    const float* P_I;      // previous frame: intensity and depth of this level
    const float* P_D;
    const float* C_I;      // current frame: intensity and depth
    const float* C_D;
};

__global__ void __launch_bounds__(64) odo_rgbd_init_kernel(const float* __restrict__ T_init, float sigma_init, float sigma_depth_init, OdoRgbdHead* head)
{
    const int k = threadIdx.x;
    const float v = (T_init && k < 12) ? T_init[k] : ((k % 5) == 0 ? 1.f : 0.f);        // the last row is 0 0 0 1 whatever T_init holds
    const bool bad = __ballot(k < 16 && !isfinite(v)) != 0ull;
    if (k < 16) head->T[k] = bad ? ((k % 5) == 0 ? 1.0 : 0.0) : (double)v;
    if (k == 0) {
        head->sigma_i = (double)sigma_init;
        head->sigma_d = (double)sigma_depth_init;
        head->last_xi = 0.0;
        head->n_last = 0.0;
        head->nd_last = 0.0;
        head->alpha = 0.0;
        head->beta = 0.0;
        head->bad_init = bad ? 1 : 0;
        head->pad = 0;
    }
}

// grid: blocks of the level (a function of its size alone), grid-stride over the level's pixels in linear order. A pixel adds its photometric
// term to a sum first, then its depth term: one fixed order.
template <bool AFFINE, bool DEPTH>
__global__ void __launch_bounds__(ODO_BLOCK) odo_rgbd_sums_kernel(OdoRgbdLevel L, float nu, float lambda, float edge_ratio,
                                                                  const OdoRgbdHead* __restrict__ head, double* __restrict__ slab)
{
    constexpr int N = AFFINE ? 8 : 6, NH = N * (N + 1) / 2, NS = NH + N + ODO_RGBD_TAIL;
    static_assert(NS <= ODO_RGBD_ROW, "a slab row holds the sums");
    __shared__ double part[ODO_BLOCK / 64][NS];
    float R[9], t[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) R[3 * i + j] = (float)head->T[4 * i + j];
        t[i] = (float)head->T[4 * i + 3];
    }
    const float sigma_i = (float)head->sigma_i, sigma_d = (float)head->sigma_d;
    const float gain = 1.f + (float)head->alpha, offset = (float)head->beta;
    const float scale_i = 1.f / (sigma_i * sigma_i), scale_d = lambda / (sigma_d * sigma_d);
    const float xmax = (float)(L.w - 2), ymax = (float)(L.h - 2);
    double acc[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) acc[k] = 0.0;
    const size_t n = (size_t)L.w * L.h;
    for (size_t p = (size_t)blockIdx.x * ODO_BLOCK + threadIdx.x; p < n; p += (size_t)gridDim.x * ODO_BLOCK) {
        const float d = L.P_D[p];
        if (!(d > 0.f)) continue;
        const int u = (int)(p % L.w), v = (int)(p / L.w);
        const float X0 = ((float)u - L.cx) / L.fx * d, X1 = ((float)v - L.cy) / L.fy * d;
        const float Y0 = R[0] * X0 + R[1] * X1 + R[2] * d + t[0];
        const float Y1 = R[3] * X0 + R[4] * X1 + R[5] * d + t[1];
        const float Y2 = R[6] * X0 + R[7] * X1 + R[8] * d + t[2];
        if (!(Y2 > ODO_MIN_Z)) continue;
        const float iz = 1.f / Y2;
        const float x = L.fx * Y0 * iz + L.cx, y = L.fy * Y1 * iz + L.cy;
        if (!(x >= 1.f && x < xmax && y >= 1.f && y < ymax)) continue;      // the 4 x 4 patch below lies inside the level
        const int x0 = (int)floorf(x), y0 = (int)floorf(y);
        const float ax = x - (float)x0, ay = y - (float)y0;
        const float bx = 1.f - ax, by = 1.f - ay;
        const float xz = Y0 * iz, yz = Y1 * iz;
        {
            const float* c0 = L.C_I + (size_t)(y0 - 1) * L.w + (x0 - 1);
            const float* c1 = c0 + L.w;
            const float* c2 = c1 + L.w;
            const float* c3 = c2 + L.w;
            const float c01 = c0[1], c02 = c0[2];
            const float c10 = c1[0], c11 = c1[1], c12 = c1[2], c13 = c1[3];
            const float c20 = c2[0], c21 = c2[1], c22 = c2[2], c23 = c2[3];
            const float c31 = c3[1], c32 = c3[2];
            const float Cs = by * (bx * c11 + ax * c12) + ay * (bx * c21 + ax * c22);
            const float gx = by * (bx * (0.5f * (c12 - c10)) + ax * (0.5f * (c13 - c11))) + ay * (bx * (0.5f * (c22 - c20)) + ax * (0.5f * (c23 - c21)));
            const float gy = by * (bx * (0.5f * (c21 - c01)) + ax * (0.5f * (c22 - c02))) + ay * (bx * (0.5f * (c31 - c11)) + ax * (0.5f * (c32 - c12)));
            const float Pv = L.P_I[p];
            const float r = AFFINE ? (Cs - gain * Pv) - offset : Cs - Pv;
            const float q = r / sigma_i;
            const float w = (nu + 1.f) / (nu + q * q);
            const float wh = w * scale_i;
            const float a = gx * L.fx * iz, b = gy * L.fy * iz;
            float J[N];
            J[0] = a;
            J[1] = b;
            J[2] = -(a * xz + b * yz);
            J[3] = -a * xz * Y1 - b * (Y2 + yz * Y1);
            J[4] = a * (Y2 + xz * Y0) + b * yz * Y0;
            J[5] = -a * Y1 + b * Y0;
            if (AFFINE) { J[N - 2] = -Pv; J[N - 1] = -1.f; }
            int k = 0;
#pragma unroll
            for (int i = 0; i < N; ++i)
#pragma unroll
                for (int j = i; j < N; ++j) acc[k++] += (double)(wh * (J[i] * J[j]));
#pragma unroll
            for (int i = 0; i < N; ++i) acc[NH + i] += (double)(wh * (J[i] * r));
            acc[NH + N + 0] += (double)w;
            acc[NH + N + 1] += (double)(w * (r * r));
            acc[NH + N + 2] += 1.0;
        }
        if (DEPTH) {
            const float* d0 = L.C_D + (size_t)y0 * L.w + x0;
            const float D00 = d0[0], D01 = d0[1], D10 = d0[L.w], D11 = d0[L.w + 1];
            const float lo = fminf(fminf(D00, D01), fminf(D10, D11)), hi = fmaxf(fmaxf(D00, D01), fmaxf(D10, D11));
            if (!(D00 > 0.f && D01 > 0.f && D10 > 0.f && D11 > 0.f) || !(hi - lo <= edge_ratio * lo)) continue;
            const float W00 = 1.f / D00, W01 = 1.f / D01, W10 = 1.f / D10, W11 = 1.f / D11;
            const float Ws = by * (bx * W00 + ax * W01) + ay * (bx * W10 + ax * W11);
            const float gx = by * (W01 - W00) + ay * (W11 - W10), gy = bx * (W10 - W00) + ax * (W11 - W01);
            const float r = Ws - iz;
            const float q = r / sigma_d;
            const float w = (nu + 1.f) / (nu + q * q);
            const float wh = w * scale_d;
            const float a = gx * L.fx * iz, b = gy * L.fy * iz, iz2 = iz * iz;
            float J[6];
            J[0] = a;
            J[1] = b;
            J[2] = -(a * xz + b * yz) + iz2;
            J[3] = -a * xz * Y1 - b * (Y2 + yz * Y1) + iz2 * Y1;
            J[4] = a * (Y2 + xz * Y0) + b * yz * Y0 - iz2 * Y0;
            J[5] = -a * Y1 + b * Y0;
            int k = 0;
#pragma unroll
            for (int i = 0; i < 6; ++i) {
#pragma unroll
                for (int j = i; j < 6; ++j) acc[k++] += (double)(wh * (J[i] * J[j]));
                k += N - 6;                                                  // past the two brightness columns of this row
            }
#pragma unroll
            for (int i = 0; i < 6; ++i) acc[NH + i] += (double)(wh * (J[i] * r));
            acc[NH + N + 3] += (double)w;
            acc[NH + N + 4] += (double)(w * (r * r));
            acc[NH + N + 5] += 1.0;
        }
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < NS; ++k) {
        const double s = motion_wave_sum(acc[k]);
        if (lane == 0) part[wave][k] = s;
    }
    __syncthreads();
    if (threadIdx.x < ODO_RGBD_ROW) {
        double s = 0.0;
        if (threadIdx.x < NS)
            for (int wv = 0; wv < ODO_BLOCK / 64; ++wv) s += part[wv][threadIdx.x];
        slab[(size_t)blockIdx.x * ODO_RGBD_ROW + threadIdx.x] = s;
    }
}

template <int N> struct OdoRgbdSolveLds { double A[N][N], g[N], xi[N], E[16], Tn[16]; };     // thread 0's own, as MotionSolveLds

constexpr double ODO_RGBD_MIN_PIVOT = 1e-6;   // of the pivot's diagonal entry: below it two columns count as collinear

// One thread. sums: the NH entries of H (upper triangle, row-major), then the N of g. Solves (H + 1e-9 tr(H) / N I) xi = -g by Cholesky;
// false where the matrix is not positive definite (a pivot not above ODO_RGBD_MIN_PIVOT of its diagonal entry) or xi is not finite.
template <int N>
__device__ inline bool odo_rgbd_solve(const double* sums, OdoRgbdSolveLds<N>& L)
{
    constexpr int NH = N * (N + 1) / 2;
    int k = 0;
    for (int i = 0; i < N; ++i)
        for (int j = i; j < N; ++j) { L.A[i][j] = sums[k]; L.A[j][i] = sums[k]; ++k; }
    double tr = 0.0;
    for (int i = 0; i < N; ++i) { tr += L.A[i][i]; L.g[i] = -sums[NH + i]; }
    for (int i = 0; i < N; ++i) L.A[i][i] += 1e-9 * tr / (double)N;
    for (int j = 0; j < N; ++j) {                              // A = L L^T, L in the lower triangle
        const double diagonal = L.A[j][j];
        double d = diagonal;
        for (int m = 0; m < j; ++m) d -= L.A[j][m] * L.A[j][m];
        if (!(d > 0.0) || !(d > ODO_RGBD_MIN_PIVOT * diagonal)) return false;
        L.A[j][j] = sqrt(d);
        for (int i = j + 1; i < N; ++i) {
            double s = L.A[i][j];
            for (int m = 0; m < j; ++m) s -= L.A[i][m] * L.A[j][m];
            L.A[i][j] = s / L.A[j][j];
        }
    }
    for (int i = 0; i < N; ++i) {
        double s = L.g[i];
        for (int m = 0; m < i; ++m) s -= L.A[i][m] * L.xi[m];
        L.xi[i] = s / L.A[i][i];
    }
    for (int i = N - 1; i >= 0; --i) {
        double s = L.xi[i];
        for (int m = i + 1; m < N; ++m) s -= L.A[m][i] * L.xi[m];
        L.xi[i] = s / L.A[i][i];
    }
    for (int i = 0; i < N; ++i)
        if (!isfinite(L.xi[i])) return false;
    return true;
}

// One block. The pass's sums, its step, and the scales the next pass weighs with.
template <int N>
__global__ void __launch_bounds__(ODO_BLOCK) odo_rgbd_solve_kernel(int rows, const double* __restrict__ slab, OdoRgbdHead* head, float sigma_min,
                                                                   float sigma_depth_min, int level, double* __restrict__ trace_row)
{
    constexpr int NH = N * (N + 1) / 2, TAIL = NH + N;
    __shared__ double tile[ODO_RGBD_SLAB_TILE * ODO_RGBD_ROW];
    __shared__ double sums[ODO_RGBD_ROW];
    __shared__ OdoRgbdSolveLds<N> S;
    double s = 0.0;                                             // column k by thread k, the rows in index order
    for (int r0 = 0; r0 < rows; r0 += ODO_RGBD_SLAB_TILE) {
        const int count = min(ODO_RGBD_SLAB_TILE, rows - r0) * ODO_RGBD_ROW;
        for (int k = threadIdx.x; k < count; k += ODO_BLOCK) tile[k] = slab[(size_t)r0 * ODO_RGBD_ROW + k];
        __syncthreads();
        if (threadIdx.x < ODO_RGBD_ROW)
            for (int k = threadIdx.x; k < count; k += ODO_RGBD_ROW) s += tile[k];
        __syncthreads();
    }
    if (threadIdx.x < ODO_RGBD_ROW) sums[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x != 0) return;
    sums[TAIL + 6] = head->sigma_i;                             // what this pass used
    sums[TAIL + 7] = head->sigma_d;
    sums[TAIL + 8] = head->alpha;
    sums[TAIL + 9] = head->beta;
    sums[TAIL + 10] = (double)level;
    if (trace_row)
        for (int k = 0; k < ODO_RGBD_ROW; ++k) trace_row[k] = sums[k];
    const double n_i = sums[TAIL + 2], n_d = sums[TAIL + 5];
    head->n_last = n_i;
    head->nd_last = n_d;
    double step = INFINITY;                                     // a pass without a step never passes the gate
    if (n_i >= (double)N && odo_rgbd_solve<N>(sums, S)) {
        motion_se3_exp(S.xi, S.E);
        for (int i = 0; i < 4; ++i)
            for (int j = 0; j < 4; ++j) {
                double a = 0.0;
                for (int m = 0; m < 4; ++m) a += S.E[4 * i + m] * head->T[4 * m + j];
                S.Tn[4 * i + j] = a;
            }
        for (int i = 0; i < 16; ++i) head->T[i] = S.Tn[i];
        if (N == 8) { head->alpha += S.xi[N - 2]; head->beta += S.xi[N - 1]; }
        double q = 0.0;
        for (int i = 0; i < N; ++i) q += S.xi[i] * S.xi[i];
        step = sqrt(q);
    }
    head->last_xi = step;
    if (n_i > 0.0) head->sigma_i = fmax((double)sigma_min, sqrt(sums[TAIL + 1] / n_i));
    if (n_d > 0.0) head->sigma_d = fmax((double)sigma_depth_min, sqrt(sums[TAIL + 4] / n_d));
}

// One wave; thread 0 decides. T_out is the aligned motion when accepted, identity otherwise.
__global__ void __launch_bounds__(64) odo_rgbd_finish_kernel(const OdoRgbdHead* __restrict__ head, const OdoPyramidHead* __restrict__ prev, int affine,
                                                             float min_share, float max_last_step, float max_translation, float max_rotation,
                                                             float max_gain, float max_offset, float* __restrict__ T_out, double* __restrict__ stats)
{
    if (threadIdx.x != 0) return;
    const double* T = head->T;
    const int valid0 = prev->valid0;
    const double share = valid0 > 0 ? head->n_last / (double)valid0 : 0.0;
    const double tn = sqrt(T[3] * T[3] + T[7] * T[7] + T[11] * T[11]);
    const double sx = T[9] - T[6], sy = T[2] - T[8], sz = T[4] - T[1];
    const double angle = atan2(0.5 * sqrt(sx * sx + sy * sy + sz * sz), 0.5 * (T[0] + T[5] + T[10] - 1.0));
    bool finite = true;
    for (int k = 0; k < 12; ++k) finite = finite && isfinite(T[k]);
    bool accepted = !head->bad_init && finite && share >= (double)min_share && head->last_xi <= (double)max_last_step &&
                    tn <= (double)max_translation && angle <= (double)max_rotation;
    if (affine)                                                 // a comparison with a NaN is false: not finite, not accepted
        accepted = accepted && fabs(head->alpha) <= (double)max_gain && fabs(head->beta) <= (double)max_offset;
    for (int k = 0; k < 16; ++k) T_out[k] = accepted ? (float)T[k] : ((k % 5) == 0 ? 1.f : 0.f);
    stats[0] = accepted ? 1.0 : 0.0;
    stats[1] = share;
    stats[2] = head->sigma_i;
    stats[3] = head->last_xi;
    stats[4] = head->n_last;
    stats[5] = tn;
    stats[6] = angle;
    stats[7] = (double)valid0;
    stats[8] = head->alpha;
    stats[9] = head->beta;
    stats[10] = head->sigma_d;
    stats[11] = head->nd_last;
}

}  // namespace gsr
