// gs_motion.h -- the kernels of include/motion_segmentation.h: a robust rigid fit of one camera motion to a flow field with depth
// (gsr_flow_rigid_fit) and the cleaning of a candidate mask into a few solid regions (gsr_motion_mask_clean).
//
// Fit, per call:      motion_prep_kernel                      usable / fit-set flags, their counts, T <- T_init
//   per iteration:    motion_residual_kernel                  e = |pi(T X) - t| of the fit set into an integer histogram (LDS, then global)
//                     motion_normal_kernel                    every block reads the histogram -> median bin -> cutoff c of THIS pass; Tukey
//                                                             weights, the 30 sums in double: thread -> wave -> block -> its row of the slab
//                     motion_solve_kernel   (one block)       adds the slab in row order, Cholesky in double, T <- exp(xi) T, trace row
//   after the last:   motion_residual_kernel (writes residual), motion_finish_kernel (c under the final T, stats, candidate)
// The slab is written by one launch and read by the next: the kernel boundary is the only ordering between blocks. Integer atomics only;
// every floating-point sum has one fixed order, so the same input gives the same bytes.
//
// Clean:  erode, dilate (the opening) -> init -> merge -> flatten -> count -> filter -> grow. The labelling is a union-find over the pixel
// grid: init hangs every set pixel under the first pixel of its horizontal run inside its wave's 64 indices, merge joins what that leaves
// apart. A root is linked under a smaller root with atomicMin, so parent[x] <= x always holds, no cycle can form, and the root that survives
// is the component's smallest linear index whatever the schedule was. parent[] is read with agent-scope atomic loads while other blocks
// link (a plain load may be served from a stale line); each later stage is a launch of its own and reads what the earlier launch finished.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gsr {

constexpr int MOTION_BLOCK = 256;
constexpr int MOTION_BINS = 1024;              // of 1/16 px; the last one is open
constexpr float MOTION_BINS_PER_PX = 16.f;
constexpr int MOTION_MAX_BLOCKS = 256;         // rows of the slab: the grid of the per-iteration kernels, a function of the size alone
constexpr int MOTION_SUMS = 30;                // 21 of H (upper triangle, row-major), 6 of g, sum w, sum w e^2, pixels with w > 0
constexpr int MOTION_ROW = 32;                 // doubles per slab row and per trace row
constexpr float MOTION_MIN_Z = 1e-3f;
constexpr float MOTION_BEHIND = 3.0e38f;       // the residual of a usable pixel that the pose puts at Y_z <= MOTION_MIN_Z

enum { MOTION_USABLE = 1, MOTION_FIT = 2 };

struct MotionCam { int W, H; float fx, fy, cx, cy; };

// what the launches of one fit hand to each other (the head of the workspace; zeroed by a memset node before the first launch)
struct MotionHead {
    double T[16];
    double sum_w;
    float c;
    int bin, usable, fit;
    int hist[MOTION_BINS];
};

__device__ __forceinline__ double motion_wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

__device__ __forceinline__ void motion_count(bool flag, int* counter)        // one integer atomic per wave
{
    const unsigned long long b = __ballot(flag);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(counter, __popcll(b));
}

__device__ __forceinline__ bool motion_bilinear(const MotionCam& cam, const float2* __restrict__ f, float x, float y, float& ox, float& oy)
{
    const int x0 = (int)floorf(x), y0 = (int)floorf(y);
    const int x1 = min(x0 + 1, cam.W - 1), y1 = min(y0 + 1, cam.H - 1);
    const float ax = x - (float)x0, ay = y - (float)y0;
    const float2 a = f[(size_t)y0 * cam.W + x0], b = f[(size_t)y0 * cam.W + x1], c = f[(size_t)y1 * cam.W + x0], d = f[(size_t)y1 * cam.W + x1];
    ox = (1.f - ay) * ((1.f - ax) * a.x + ax * b.x) + ay * ((1.f - ax) * c.x + ax * d.x);
    oy = (1.f - ay) * ((1.f - ax) * a.y + ax * b.y) + ay * ((1.f - ax) * c.y + ax * d.y);
    return isfinite(ox) && isfinite(oy);
}

__global__ void __launch_bounds__(MOTION_BLOCK) motion_prep_kernel(MotionCam cam, const float2* __restrict__ flow_ij, const float* __restrict__ depth,
                                                                   const float2* __restrict__ flow_ji, const unsigned char* __restrict__ fit_mask,
                                                                   const float* __restrict__ T_init, float occlusion_px,
                                                                   unsigned char* __restrict__ flags, MotionHead* head)
{
    if (blockIdx.x == 0 && threadIdx.x < 16)
        head->T[threadIdx.x] = T_init ? (double)T_init[threadIdx.x] : ((threadIdx.x % 5) == 0 ? 1.0 : 0.0);
    const size_t n = (size_t)cam.W * cam.H;
    const size_t p = (size_t)blockIdx.x * MOTION_BLOCK + threadIdx.x;
    bool usable = false, fit = false;
    if (p < n) {
        const int u = (int)(p % cam.W), v = (int)(p / cam.W);
        const float d = depth[p];
        const float2 f = flow_ij[p];
        const float px = f.x * (0.5f * cam.W), py = f.y * (0.5f * cam.H);
        const float tx = (float)u + px, ty = (float)v + py;
        usable = d > 0.f && isfinite(d) && isfinite(f.x) && isfinite(f.y) && tx >= 0.f && tx <= (float)(cam.W - 1) && ty >= 0.f &&
                 ty <= (float)(cam.H - 1);
        if (usable && flow_ji) {
            float bx, by;
            usable = motion_bilinear(cam, flow_ji, tx, ty, bx, by);
            const float sx = px + bx * (0.5f * cam.W), sy = py + by * (0.5f * cam.H);
            usable = usable && sqrtf(sx * sx + sy * sy) <= occlusion_px;
        }
        fit = usable && (!fit_mask || fit_mask[p]);
        flags[p] = (unsigned char)((usable ? MOTION_USABLE : 0) | (fit ? MOTION_FIT : 0));
    }
    motion_count(usable, &head->usable);
    motion_count(fit, &head->fit);
}

// the pose as floats: rows of R, then t
struct MotionPose { float r[9], t[3]; };
__device__ __forceinline__ MotionPose motion_load_pose(const MotionHead* head)
{
    MotionPose P;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) P.r[3 * i + j] = (float)head->T[4 * i + j];
        P.t[i] = (float)head->T[4 * i + 3];
    }
    return P;
}

// Y = R X + t0, r = pi(Y) - t, e = |r| for pixel p; false where Y_z <= MOTION_MIN_Z
__device__ __forceinline__ bool motion_residual(const MotionCam& cam, const MotionPose& P, const float2* __restrict__ flow_ij,
                                                const float* __restrict__ depth, size_t p, float Y[3], float& rx, float& ry, float& e)
{
    const int u = (int)(p % cam.W), v = (int)(p / cam.W);
    const float d = depth[p];
    const float2 f = flow_ij[p];
    const float X0 = ((float)u - cam.cx) / cam.fx * d, X1 = ((float)v - cam.cy) / cam.fy * d;
    Y[0] = P.r[0] * X0 + P.r[1] * X1 + P.r[2] * d + P.t[0];
    Y[1] = P.r[3] * X0 + P.r[4] * X1 + P.r[5] * d + P.t[1];
    Y[2] = P.r[6] * X0 + P.r[7] * X1 + P.r[8] * d + P.t[2];
    if (!(Y[2] > MOTION_MIN_Z)) { rx = ry = 0.f; e = MOTION_BEHIND; return false; }
    const float iz = 1.f / Y[2];
    rx = cam.fx * Y[0] * iz + cam.cx - ((float)u + f.x * (0.5f * cam.W));
    ry = cam.fy * Y[1] * iz + cam.cy - ((float)v + f.y * (0.5f * cam.H));
    e = sqrtf(rx * rx + ry * ry);
    if (!isfinite(e)) e = MOTION_BEHIND;
    return true;
}

__device__ __forceinline__ int motion_bin(float e)
{
    const float b = e * MOTION_BINS_PER_PX;
    return b >= (float)(MOTION_BINS - 1) ? MOTION_BINS - 1 : (int)b;
}

// grid: motion_blocks(n) blocks, grid-stride. The histogram must be zero on entry (the memset node, later motion_solve_kernel).
__global__ void __launch_bounds__(MOTION_BLOCK) motion_residual_kernel(MotionCam cam, const float2* __restrict__ flow_ij, const float* __restrict__ depth,
                                                                       const unsigned char* __restrict__ flags, MotionHead* head,
                                                                       float* __restrict__ residual)
{
    __shared__ int hist[MOTION_BINS];
    for (int k = threadIdx.x; k < MOTION_BINS; k += MOTION_BLOCK) hist[k] = 0;
    __syncthreads();
    const MotionPose P = motion_load_pose(head);
    const size_t n = (size_t)cam.W * cam.H;
    for (size_t p = (size_t)blockIdx.x * MOTION_BLOCK + threadIdx.x; p < n; p += (size_t)gridDim.x * MOTION_BLOCK) {
        const int fl = flags[p];
        float e = -1.f;
        if (fl & MOTION_USABLE) {
            float Y[3], rx, ry;
            motion_residual(cam, P, flow_ij, depth, p, Y, rx, ry, e);
            if (fl & MOTION_FIT) atomicAdd(&hist[motion_bin(e)], 1);
        }
        if (residual) residual[p] = e;
    }
    __syncthreads();
    for (int k = threadIdx.x; k < MOTION_BINS; k += MOTION_BLOCK)
        if (hist[k]) atomicAdd(&head->hist[k], hist[k]);
}

// The first bin whose cumulative count reaches (n + 1) / 2 (0 for an empty histogram); every thread of the block gets it.
// lds: MOTION_BINS + 1 ints.
__device__ __forceinline__ int motion_median_bin(const int* hist, int* lds)
{
    for (int k = threadIdx.x; k < MOTION_BINS; k += MOTION_BLOCK) lds[k] = hist[k];
    if (threadIdx.x == 0) lds[MOTION_BINS] = 0;
    __syncthreads();
    if (threadIdx.x < 64) {
        constexpr int PER = MOTION_BINS / 64;
        const int lane = threadIdx.x;
        int s = 0;
        for (int k = 0; k < PER; ++k) s += lds[lane * PER + k];
        int cum = s;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int other = __shfl_up(cum, o, 64);
            if (lane >= o) cum += other;
        }
        const int n = __shfl(cum, 63, 64);
        const int target = (n + 1) / 2;
        int before = cum - s;
        if (n > 0 && before < target && cum >= target) {
            int b = lane * PER;
            for (;; ++b) {
                before += lds[b];
                if (before >= target) break;
            }
            lds[MOTION_BINS] = b;
        }
    }
    __syncthreads();
    const int b = lds[MOTION_BINS];
    __syncthreads();
    return b;
}

__device__ __forceinline__ float motion_cutoff(int bin, float scale_multiplier, float c_min, float c_max)
{
    const float med = (float)(bin + 1) / MOTION_BINS_PER_PX;
    return fminf(fmaxf(scale_multiplier * 1.4826f * med, c_min), c_max);
}

__global__ void __launch_bounds__(MOTION_BLOCK) motion_normal_kernel(MotionCam cam, const float2* __restrict__ flow_ij, const float* __restrict__ depth,
                                                                     const unsigned char* __restrict__ flags, MotionHead* head,
                                                                     float scale_multiplier, float c_min, float c_max, double* __restrict__ slab)
{
    __shared__ int lds[MOTION_BINS + 1];
    __shared__ double part[MOTION_BLOCK / 64][MOTION_SUMS];
    const int bin = motion_median_bin(head->hist, lds);
    const float c = motion_cutoff(bin, scale_multiplier, c_min, c_max);
    if (blockIdx.x == 0 && threadIdx.x == 0) { head->bin = bin; head->c = c; }
    const MotionPose P = motion_load_pose(head);
    const float ic2 = 1.f / (c * c);
    double acc[MOTION_SUMS];
#pragma unroll
    for (int k = 0; k < MOTION_SUMS; ++k) acc[k] = 0.0;
    const size_t n = (size_t)cam.W * cam.H;
    for (size_t p = (size_t)blockIdx.x * MOTION_BLOCK + threadIdx.x; p < n; p += (size_t)gridDim.x * MOTION_BLOCK) {
        if (!(flags[p] & MOTION_FIT)) continue;
        float Y[3], r[2], e;
        if (!motion_residual(cam, P, flow_ij, depth, p, Y, r[0], r[1], e) || !(e < c)) continue;
        const float q = 1.f - e * e * ic2;
        const float w = q * q;
        if (!(w > 0.f)) continue;
        // d pi / d Y times [I | -[Y]x]: the residual against a left perturbation xi = [rho | theta]
        const float iz = 1.f / Y[2];
        const float a = cam.fx * iz, b = cam.fy * iz, xz = Y[0] * iz, yz = Y[1] * iz;
        float J[2][6];
        J[0][0] = a;   J[0][1] = 0.f; J[0][2] = -a * xz; J[0][3] = -a * xz * Y[1];            J[0][4] = a * (Y[2] + xz * Y[0]); J[0][5] = -a * Y[1];
        J[1][0] = 0.f; J[1][1] = b;   J[1][2] = -b * yz; J[1][3] = -b * (Y[2] + yz * Y[1]);   J[1][4] = b * yz * Y[0];          J[1][5] = b * Y[0];
        int k = 0;
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
            for (int j = i; j < 6; ++j) acc[k++] += (double)(w * (J[0][i] * J[0][j] + J[1][i] * J[1][j]));
#pragma unroll
        for (int i = 0; i < 6; ++i) acc[21 + i] += (double)(w * (J[0][i] * r[0] + J[1][i] * r[1]));
        acc[27] += (double)w;
        acc[28] += (double)(w * e * e);
        acc[29] += 1.0;
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < MOTION_SUMS; ++k) {
        const double s = motion_wave_sum(acc[k]);
        if (lane == 0) part[wave][k] = s;
    }
    __syncthreads();
    if (threadIdx.x < MOTION_ROW) {
        double s = 0.0;
        if (threadIdx.x < MOTION_SUMS)
            for (int wv = 0; wv < MOTION_BLOCK / 64; ++wv) s += part[wv][threadIdx.x];
        slab[(size_t)blockIdx.x * MOTION_ROW + threadIdx.x] = s;
    }
}

// exp of xi = [rho | theta] as a 4x4 (the closed forms of slam/camera.py SE3_exp, in double)
__device__ inline void motion_se3_exp(const double xi[6], double E[16])
{
    const double wx = xi[3], wy = xi[4], wz = xi[5];
    const double K[9] = {0, -wz, wy, wz, 0, -wx, -wy, wx, 0};
    double K2[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) K2[3 * i + j] = K[3 * i] * K[j] + K[3 * i + 1] * K[3 + j] + K[3 * i + 2] * K[6 + j];
    const double th = sqrt(wx * wx + wy * wy + wz * wz);
    double A = 1.0, B = 0.5, C = 1.0 / 6.0;
    if (th >= 1e-5) { A = sin(th) / th; B = (1.0 - cos(th)) / (th * th); C = (th - sin(th)) / (th * th * th); }
    for (int i = 0; i < 3; ++i) {
        double t = 0.0;
        for (int j = 0; j < 3; ++j) {
            const double I = i == j ? 1.0 : 0.0;
            E[4 * i + j] = I + A * K[3 * i + j] + B * K2[3 * i + j];
            t += (I + B * K[3 * i + j] + C * K2[3 * i + j]) * xi[j];
        }
        E[4 * i + 3] = t;
    }
    E[12] = E[13] = E[14] = 0.0;
    E[15] = 1.0;
}

// Shared with gs_odometry.h: the slab sum, the regularised 6 x 6 solve and the pose update of one Gauss-Newton pass.
constexpr int MOTION_SLAB_TILE = 128;                           // rows staged in LDS at a time: the loads run in parallel, the adds in row order
struct MotionSolveLds { double A[6][6], g[6], xi[6], E[16], Tn[16]; };     // thread 0's own: indexed by loop variables, and LDS is nearer than scratch

// Every thread of the block calls it. Adds the slab's rows in index order, column k by thread k; threads k < MOTION_ROW return column k's sum.
// tile: MOTION_SLAB_TILE * MOTION_ROW doubles of LDS.
__device__ __forceinline__ double motion_slab_sum(int rows, const double* __restrict__ slab, double* tile)
{
    double s = 0.0;
    for (int r0 = 0; r0 < rows; r0 += MOTION_SLAB_TILE) {
        const int count = min(MOTION_SLAB_TILE, rows - r0) * MOTION_ROW;
        for (int k = threadIdx.x; k < count; k += MOTION_BLOCK) tile[k] = slab[(size_t)r0 * MOTION_ROW + k];
        __syncthreads();
        if (threadIdx.x < MOTION_ROW)
            for (int k = threadIdx.x; k < count; k += MOTION_ROW) s += tile[k];
        __syncthreads();
    }
    return s;
}

// One thread. sums: the 21 entries of H (upper triangle, row-major), then the 6 of g. Solves (H + 1e-9 tr(H) / 6 I) xi = -g by Cholesky and
// sets T <- exp(xi) T; xi stays in L.xi. False, and T as it was, where the matrix is not positive definite or xi is not finite.
__device__ inline bool motion_gauss_newton_step(const double* sums, double* T, MotionSolveLds& L)
{
    int k = 0;
    for (int i = 0; i < 6; ++i)
        for (int j = i; j < 6; ++j) { L.A[i][j] = sums[k]; L.A[j][i] = sums[k]; ++k; }
    double tr = 0.0;
    for (int i = 0; i < 6; ++i) { tr += L.A[i][i]; L.g[i] = -sums[21 + i]; }
    for (int i = 0; i < 6; ++i) L.A[i][i] += 1e-9 * tr / 6.0;
    bool ok = true;                                             // A = L L^T, L in the lower triangle
    for (int j = 0; j < 6 && ok; ++j) {
        double d = L.A[j][j];
        for (int m = 0; m < j; ++m) d -= L.A[j][m] * L.A[j][m];
        if (!(d > 0.0)) { ok = false; break; }
        L.A[j][j] = sqrt(d);
        for (int i = j + 1; i < 6; ++i) {
            double s = L.A[i][j];
            for (int m = 0; m < j; ++m) s -= L.A[i][m] * L.A[j][m];
            L.A[i][j] = s / L.A[j][j];
        }
    }
    if (!ok) return false;
    for (int i = 0; i < 6; ++i) {
        double s = L.g[i];
        for (int m = 0; m < i; ++m) s -= L.A[i][m] * L.xi[m];
        L.xi[i] = s / L.A[i][i];
    }
    for (int i = 5; i >= 0; --i) {
        double s = L.xi[i];
        for (int m = i + 1; m < 6; ++m) s -= L.A[m][i] * L.xi[m];
        L.xi[i] = s / L.A[i][i];
    }
    for (int i = 0; i < 6; ++i)
        if (!isfinite(L.xi[i])) return false;
    motion_se3_exp(L.xi, L.E);
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            double s = 0.0;
            for (int m = 0; m < 4; ++m) s += L.E[4 * i + m] * T[4 * m + j];
            L.Tn[4 * i + j] = s;
        }
    for (int i = 0; i < 16; ++i) T[i] = L.Tn[i];
    return true;
}

// One block. Adds the slab's rows in index order (column k by thread k), solves (H + 1e-9 tr(H) / 6 I) xi = -g by Cholesky, T <- exp(xi) T;
// a matrix that is not positive definite (an empty fit set) leaves T as it is. Zeroes the histogram for the next pass.
__global__ void __launch_bounds__(MOTION_BLOCK) motion_solve_kernel(int rows, const double* __restrict__ slab, MotionHead* head, double* __restrict__ trace_row)
{
    __shared__ double tile[MOTION_SLAB_TILE * MOTION_ROW];
    __shared__ double sums[MOTION_ROW];
    __shared__ MotionSolveLds L;
    const double s = motion_slab_sum(rows, slab, tile);
    if (threadIdx.x < MOTION_ROW) sums[threadIdx.x] = s;
    for (int k = threadIdx.x; k < MOTION_BINS; k += MOTION_BLOCK) head->hist[k] = 0;
    __syncthreads();
    if (threadIdx.x != 0) return;
    sums[30] = (double)head->bin;
    sums[31] = (double)head->c;
    if (trace_row)
        for (int k = 0; k < MOTION_ROW; ++k) trace_row[k] = sums[k];
    head->sum_w = sums[27];
    motion_gauss_newton_step(sums, head->T, L);
}

// After the residual pass under the final T: c from its histogram, the outputs T and stats, and candidate = usable and residual > max(residual_px, c).
__global__ void __launch_bounds__(MOTION_BLOCK) motion_finish_kernel(long long n, MotionHead* head, float scale_multiplier, float c_min, float c_max,
                                                                     float residual_px, const unsigned char* __restrict__ flags,
                                                                     const float* __restrict__ residual, float* __restrict__ T_out,
                                                                     double* __restrict__ stats, unsigned char* __restrict__ candidate)
{
    __shared__ int lds[MOTION_BINS + 1];
    const int bin = motion_median_bin(head->hist, lds);
    const float c = motion_cutoff(bin, scale_multiplier, c_min, c_max);
    if (blockIdx.x == 0) {
        if (threadIdx.x < 16) T_out[threadIdx.x] = (float)head->T[threadIdx.x];
        if (threadIdx.x == 0) {
            stats[0] = (double)c;
            stats[1] = (double)head->usable;
            stats[2] = (double)head->fit;
            stats[3] = head->sum_w;
        }
    }
    if (!candidate) return;
    const float bar = fmaxf(residual_px, c);
    const long long p = (long long)blockIdx.x * MOTION_BLOCK + threadIdx.x;
    if (p < n) candidate[p] = (unsigned char)((flags[p] & MOTION_USABLE) && residual[p] > bar);
}

// ---- cleaning -------------------------------------------------------------------------------------------------------------------------
// erode != 0: 1 where every pixel of the (2r+1)^2 square is set and inside the image; else 1 where any pixel of the square is set.
// motion (optional, with the dilation): motion[p] &= ~out[p]. counter (optional): the number of set output pixels.
__global__ void __launch_bounds__(MOTION_BLOCK) motion_morph_kernel(int W, int H, int r, int erode, const unsigned char* __restrict__ in,
                                                                    unsigned char* __restrict__ out, unsigned char* __restrict__ motion, int* counter)
{
    const long long n = (long long)W * H;
    const long long p = (long long)blockIdx.x * MOTION_BLOCK + threadIdx.x;
    bool set = false;
    if (p < n) {
        const int u = (int)(p % W), v = (int)(p / W);
        if (erode) {
            set = u - r >= 0 && u + r < W && v - r >= 0 && v + r < H;
            for (int y = v - r; set && y <= v + r; ++y)
                for (int x = u - r; x <= u + r; ++x)
                    if (!in[(long long)y * W + x]) { set = false; break; }
        } else {
            const int y0 = max(v - r, 0), y1 = min(v + r, H - 1), x0 = max(u - r, 0), x1 = min(u + r, W - 1);
            for (int y = y0; !set && y <= y1; ++y)
                for (int x = x0; x <= x1; ++x)
                    if (in[(long long)y * W + x]) { set = true; break; }
        }
        out[p] = (unsigned char)set;
        if (motion && set) motion[p] = 0;
    }
    if (counter) motion_count(set, counter);
}

__device__ __forceinline__ int motion_parent(const int* parent, int x)
{
    return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ int motion_find(int* parent, int x)
{
    const int start = x;
    int p = motion_parent(parent, x);
    while (p != x) { x = p; p = motion_parent(parent, x); }
    if (x != start) atomicMin(parent + start, x);       // shorten the chain: x is an ancestor of start, and <= parent[start]
    return x;
}

__device__ __forceinline__ void motion_union(int* parent, int a, int b)
{
    for (;;) {
        a = motion_find(parent, a);
        b = motion_find(parent, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(parent + a, b);          // a > b
        if (old == a) return;                               // a was still a root and now hangs under b
        a = old;                                            // a had been linked meanwhile: its former parent and b remain to be joined
    }
}

// A wave holds 64 consecutive linear indices. A set pixel starts as a child of the first pixel of its horizontal run inside the wave's
// span (runs end at a row's end), found from two ballots: most west links exist before the merge launch, and without one union.
__global__ void __launch_bounds__(MOTION_BLOCK) motion_label_init_kernel(int W, long long n, const unsigned char* __restrict__ mask,
                                                                         int* __restrict__ parent, int* __restrict__ area, int* __restrict__ counts)
{
    const long long p = (long long)blockIdx.x * MOTION_BLOCK + threadIdx.x;
    if (blockIdx.x == 0 && threadIdx.x < 4) counts[threadIdx.x] = 0;
    const bool set = p < n && mask[p];
    const unsigned long long b = __ballot(set), row_start = __ballot(p < n && p % W == 0);
    const unsigned long long starts = b & (~(b << 1) | row_start | 1ull);
    if (p >= n) return;
    int par = -1;
    if (set) {
        const int lane = threadIdx.x & 63;
        const unsigned long long upto = starts & (lane == 63 ? ~0ull : ((2ull << lane) - 1ull));      // this lane's run is set from its start on
        par = (int)p - (lane - (63 - __clzll((long long)upto)));
    }
    parent[p] = par;
    area[p] = 0;
}

// Joins what the runs of the init launch left apart, each 8-connected pair through at least one chain of unions and few of them twice:
// the west link across a wave's span; the north link unless the west pixel makes it through its own (west and north-west both set);
// where north is clear, north-west unless west makes it (west's north), and north-east unless east makes it (east's north).
__global__ void __launch_bounds__(MOTION_BLOCK) motion_label_merge_kernel(int W, int H, const unsigned char* __restrict__ mask, int* parent)
{
    const long long n = (long long)W * H;
    const long long p = (long long)blockIdx.x * MOTION_BLOCK + threadIdx.x;
    if (p >= n || !mask[p]) return;
    const int u = (int)(p % W), v = (int)(p / W);
    const bool west = u > 0 && mask[p - 1];
    if (west && (p & 63) == 0) motion_union(parent, (int)p, (int)p - 1);
    if (v == 0) return;
    const bool north_west = u > 0 && mask[p - W - 1];
    if (mask[p - W]) {
        if (!(west && north_west)) motion_union(parent, (int)p, (int)p - W);
    } else {
        if (north_west && !west) motion_union(parent, (int)p, (int)p - W - 1);
        if (u + 1 < W && mask[p - W + 1] && !mask[p + 1]) motion_union(parent, (int)p, (int)p - W + 1);
    }
}

__global__ void __launch_bounds__(MOTION_BLOCK) motion_label_flatten_kernel(long long n, int* parent, int* __restrict__ labels)
{
    const long long p = (long long)blockIdx.x * MOTION_BLOCK + threadIdx.x;
    if (p >= n) return;
    int x = motion_parent(parent, (int)p);
    if (x >= 0) {                                           // no link is made in this launch: walk up, nothing is written to parent
        int q = motion_parent(parent, x);
        while (q != x) { x = q; q = motion_parent(parent, x); }
    }
    labels[p] = x;
}

__global__ void __launch_bounds__(MOTION_BLOCK) motion_label_count_kernel(long long n, const int* __restrict__ labels, int* area, int* counts)
{
    const long long p = (long long)blockIdx.x * MOTION_BLOCK + threadIdx.x;
    const int l = p < n ? labels[p] : -1;
    // one add per wave and label, not per pixel: a large component would otherwise queue all its pixels on one address
    const int lane = threadIdx.x & 63;
    bool todo = l >= 0;
    for (unsigned long long remaining = __ballot(todo); remaining;) {
        const int leader = __ffsll((long long)remaining) - 1;
        const int label = __shfl(l, leader, 64);
        const unsigned long long same = __ballot(todo && l == label);
        if (lane == leader) atomicAdd(area + label, __popcll(same));
        if (l == label) todo = false;
        remaining &= ~same;
    }
    motion_count(l >= 0 && l == (int)p, counts + 0);
}

__global__ void __launch_bounds__(MOTION_BLOCK) motion_label_filter_kernel(long long n, int min_area, const int* __restrict__ area, int* __restrict__ labels,
                                                                           unsigned char* __restrict__ kept, int* counts)
{
    const long long p = (long long)blockIdx.x * MOTION_BLOCK + threadIdx.x;
    int l = p < n ? labels[p] : -1;
    if (l >= 0 && area[l] < min_area) l = -1;
    if (p < n) { labels[p] = l; kept[p] = (unsigned char)(l >= 0); }
    motion_count(l >= 0 && l == (int)p, counts + 1);
    motion_count(l >= 0, counts + 2);
}

}  // namespace gsr
