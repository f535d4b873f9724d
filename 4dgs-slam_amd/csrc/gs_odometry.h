// gs_odometry.h -- the kernels of include/visual_odometry.h: an intensity / depth pyramid of one frame (gsr_odometry_pyramid) and the dense
// photometric alignment of a previous pyramid (intensity and depth) against a current one (intensity) by a coarse-to-fine, Student-t
// weighted Gauss-Newton on SE(3) (gsr_odometry_align).
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

}  // namespace gsr
