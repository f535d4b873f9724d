// gs_loop.h -- the kernels of include/loop_closure.h: the pose-graph solve (gsr_pose_graph_solve) and the correction of the map
// (gsr_map_correct). The header has the rules; this file has the launch shapes.
//
// Solve, per call:    pose_graph_kernel     ONE workgroup of 256 threads does everything: checks the edges, sorts the keys (node, 2 edge + end)
//                                           into per-node edge lists (bitonic, in the workspace), and runs the outer Gauss-Newton loop with
//                                           its conjugate gradients inside. Vectors and per-edge Jacobians live in the workspace (a graph of
//                                           4096 nodes and 65536 edges needs ~45 MB, far beyond LDS); LDS holds the reduction tree. Phases
//                                           are separated by __syncthreads() alone: one workgroup's global writes are visible to it after one.
// Correct, per call:  map_quat_kernel       one thread per node: the unit quaternion of D's rotation, fp64, rounded once
//                     map_correct_kernel    four Gaussians per thread: int4 of ids, 3 float4 of positions, 4 float4 of quaternions; a thread
//                                           whose four ids all miss writes nothing
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

namespace gsr {

constexpr int PG_BLOCK = 256;
constexpr int PG_MAX_NODES = 4096;
constexpr int PG_MAX_EDGES = 65536;
constexpr int PG_KEY_SHIFT = 17;                    // 2 * PG_MAX_EDGES incidences fit 17 bits, PG_MAX_NODES nodes the 12 above them
constexpr unsigned PG_NO_KEY = 0xFFFFFFFFu;
constexpr int PG_EDGE_DOUBLES = 36;                 // P_i, Q_i, P_j, Q_j: A = [[P, Q], [0, P]]
constexpr int MAPC_BLOCK = 256;

struct PoseGraphWs {
    double *x_old, *edge_r, *edge_A, *con, *vx, *vr, *vz, *vp, *vq, *hd, *chol;
    unsigned* keys;
    int *start, *end, *active;
    unsigned char* valid;
    size_t bytes;
};

// ---- 3x3 helpers on row-major double[9]; every loop has constant bounds and unrolls, so the arrays stay in registers ------------------
__device__ __forceinline__ void m3_mul(const double* a, const double* b, double* c)
{
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int k = 0; k < 3; k++) c[r * 3 + k] = a[r * 3] * b[k] + a[r * 3 + 1] * b[3 + k] + a[r * 3 + 2] * b[6 + k];
}
__device__ __forceinline__ void m3_mul_tn(const double* a, const double* b, double* c)      // a^T b
{
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int k = 0; k < 3; k++) c[r * 3 + k] = a[r] * b[k] + a[3 + r] * b[3 + k] + a[6 + r] * b[6 + k];
}
__device__ __forceinline__ void m3_mul_nt(const double* a, const double* b, double* c)      // a b^T
{
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int k = 0; k < 3; k++) c[r * 3 + k] = a[r * 3] * b[k * 3] + a[r * 3 + 1] * b[k * 3 + 1] + a[r * 3 + 2] * b[k * 3 + 2];
}
__device__ __forceinline__ void m3_vec(const double* a, const double* v, double* o)
{
#pragma unroll
    for (int r = 0; r < 3; r++) o[r] = a[r * 3] * v[0] + a[r * 3 + 1] * v[1] + a[r * 3 + 2] * v[2];
}
__device__ __forceinline__ void m3_tvec(const double* a, const double* v, double* o)       // a^T v
{
#pragma unroll
    for (int r = 0; r < 3; r++) o[r] = a[r] * v[0] + a[3 + r] * v[1] + a[6 + r] * v[2];
}
__device__ __forceinline__ void m3_skew(const double* v, double* w)
{
    w[0] = 0.0; w[1] = -v[2]; w[2] = v[1];
    w[3] = v[2]; w[4] = 0.0; w[5] = -v[0];
    w[6] = -v[1]; w[7] = v[0]; w[8] = 0.0;
}

// Log of the header: [R | t] -> (rho | theta)
__device__ inline void pg_log(const double* R, const double* t, double* tau)
{
    const double ax[3] = {R[7] - R[5], R[2] - R[6], R[3] - R[1]};
    double c = 0.5 * (R[0] + R[4] + R[8] - 1.0);
    c = c < -1.0 ? -1.0 : (c > 1.0 ? 1.0 : c);
    const double s = 0.5 * sqrt(ax[0] * ax[0] + ax[1] * ax[1] + ax[2] * ax[2]);
    const double a = atan2(s, c);
    double th[3];
    if (a < 1e-5) {
        th[0] = 0.5 * ax[0]; th[1] = 0.5 * ax[1]; th[2] = 0.5 * ax[2];
    } else if (c > -0.99) {
        const double f = a / (2.0 * s);
        th[0] = f * ax[0]; th[1] = f * ax[1]; th[2] = f * ax[2];
    } else {
        double v[3];
        if (R[0] >= R[4] && R[0] >= R[8]) { v[0] = R[0] - c; v[1] = 0.5 * (R[3] + R[1]); v[2] = 0.5 * (R[6] + R[2]); }
        else if (R[4] >= R[8]) { v[0] = 0.5 * (R[1] + R[3]); v[1] = R[4] - c; v[2] = 0.5 * (R[7] + R[5]); }
        else { v[0] = 0.5 * (R[2] + R[6]); v[1] = 0.5 * (R[5] + R[7]); v[2] = R[8] - c; }
        double n = a / sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
        if (v[0] * ax[0] + v[1] * ax[1] + v[2] * ax[2] < 0.0) n = -n;
        th[0] = n * v[0]; th[1] = n * v[1]; th[2] = n * v[2];
    }
    double G = 1.0 / 12.0;
    if (a >= 1e-5) G = (1.0 - 0.5 * a * cos(0.5 * a) / sin(0.5 * a)) / (a * a);
    double W[9], W2[9], wt[3], w2t[3];
    m3_skew(th, W);
    m3_mul(W, W, W2);
    m3_vec(W, t, wt);
    m3_vec(W2, t, w2t);
#pragma unroll
    for (int k = 0; k < 3; k++) { tau[k] = t[k] - 0.5 * wt[k] + G * w2t[k]; tau[3 + k] = th[k]; }
}

// Exp of the header: (rho | theta) -> [R | t]
__device__ inline void pg_exp(const double* tau, double* R, double* t)
{
    const double* th = tau + 3;
    const double a = sqrt(th[0] * th[0] + th[1] * th[1] + th[2] * th[2]);
    double A = 1.0, B = 0.5, C = 1.0 / 6.0;
    if (a >= 1e-5) { A = sin(a) / a; B = (1.0 - cos(a)) / (a * a); C = (a - sin(a)) / (a * a * a); }
    double W[9], W2[9], wr[3], w2r[3];
    m3_skew(th, W);
    m3_mul(W, W, W2);
#pragma unroll
    for (int k = 0; k < 9; k++) R[k] = ((k % 4) == 0 ? 1.0 : 0.0) + A * W[k] + B * W2[k];
    m3_vec(W, tau, wr);
    m3_vec(W2, tau, w2r);
#pragma unroll
    for (int k = 0; k < 3; k++) t[k] = tau[k] + B * wr[k] + C * w2r[k];
}

__device__ __forceinline__ void pg_load_pose(const double* __restrict__ X, double* R, double* t)
{
#pragma unroll
    for (int r = 0; r < 3; r++) {
        R[r * 3] = X[r * 4]; R[r * 3 + 1] = X[r * 4 + 1]; R[r * 3 + 2] = X[r * 4 + 2]; t[r] = X[r * 4 + 3];
    }
}

// the sum of `mine` over the block: the fixed tree of the header; every thread gets the result
__device__ __forceinline__ double pg_block_sum(double mine, double* red)
{
    const int t = threadIdx.x;
    __syncthreads();                                      // the previous result has been read by everyone
    red[t] = mine;
    __syncthreads();
#pragma unroll
    for (int s = PG_BLOCK / 2; s > 0; s >>= 1) {
        if (t < s) red[t] = red[t] + red[t + s];
        __syncthreads();
    }
    return red[0];
}
__device__ __forceinline__ double pg_block_max(double mine, double* red)
{
    const int t = threadIdx.x;
    __syncthreads();
    red[t] = mine;
    __syncthreads();
#pragma unroll
    for (int s = PG_BLOCK / 2; s > 0; s >>= 1) {
        if (t < s) red[t] = fmax(red[t], red[t + s]);
        __syncthreads();
    }
    return red[0];
}
__device__ __forceinline__ double pg_dot(const double* __restrict__ a, const double* __restrict__ b, int nodes, double* red)
{
    double s = 0.0;
    for (int k = threadIdx.x; k < nodes; k += PG_BLOCK) {
        double term = 0.0;
#pragma unroll
        for (int c = 0; c < 6; c++) term += a[k * 6 + c] * b[k * 6 + c];
        s += term;
    }
    return pg_block_sum(s, red);
}

// r = Log(Z^-1 X_j X_i^-1) of one edge and, with STORE, its Jacobian blocks into A[36]
template <bool STORE>
__device__ inline void pg_linearise(const double* __restrict__ Xi, const double* __restrict__ Xj, const double* __restrict__ Z, double* r,
                                    double* __restrict__ A)
{
    double Ri[9], ti[3], Rj[9], tj[3], Rz[9], tz[3], Rm[9], tm[3], Re[9], te[3], tmp[3];
    pg_load_pose(Xi, Ri, ti);
    pg_load_pose(Xj, Rj, tj);
    pg_load_pose(Z, Rz, tz);
    m3_mul_nt(Rj, Ri, Rm);                                 // M = X_j X_i^-1
    m3_vec(Rm, ti, tmp);
#pragma unroll
    for (int k = 0; k < 3; k++) tm[k] = tj[k] - tmp[k] - tz[k];
    m3_mul_tn(Rz, Rm, Re);                                 // E = Z^-1 M
    m3_tvec(Rz, tm, te);
    pg_log(Re, te, r);
    if (!STORE) return;
    double Th[9], Rh[9], Th2[9], Th4[9], Cm[9], K[9], t1[9], t2[9];
    m3_skew(r + 3, Th);
    m3_skew(r, Rh);
    m3_mul(Th, Th, Th2);
    m3_mul(Th2, Th2, Th4);
    m3_mul(Th, Rh, t1);
    m3_mul(Rh, Th, t2);
#pragma unroll
    for (int k = 0; k < 9; k++) Cm[k] = t1[k] + t2[k];
    m3_mul(Th2, Cm, t1);
    m3_mul(Cm, Th2, t2);
#pragma unroll
    for (int k = 0; k < 9; k++) K[k] = t1[k] + t2[k];
    double Ja[9], Jb[9];                                   // Jinv(r) = [[Ja, Jb], [0, Ja]]
#pragma unroll
    for (int k = 0; k < 9; k++) {
        const double even_a = ((k % 4) == 0 ? 1.0 : 0.0) + Th2[k] * (1.0 / 12.0) - Th4[k] * (1.0 / 720.0);
        const double even_b = Cm[k] * (1.0 / 12.0) - K[k] * (1.0 / 720.0);
        Ja[k] = even_a - 0.5 * Th[k];
        Jb[k] = even_b - 0.5 * Rh[k];
        A[k] = -(even_a + 0.5 * Th[k]);                    // P_i = -Ja(-r)
        A[9 + k] = -(even_b + 0.5 * Rh[k]);                // Q_i = -Jb(-r)
    }
    double RzT[9], tp[3], Tp[9], TR[9];
#pragma unroll
    for (int r_ = 0; r_ < 3; r_++)
#pragma unroll
        for (int k = 0; k < 3; k++) RzT[r_ * 3 + k] = Rz[k * 3 + r_];
    m3_tvec(Rz, tz, tp);
#pragma unroll
    for (int k = 0; k < 3; k++) tp[k] = -tp[k];            // Z^-1 = [Rz^T | -Rz^T tz]
    m3_skew(tp, Tp);
    m3_mul(Tp, RzT, TR);
    m3_mul(Ja, RzT, t1);                                   // P_j
    m3_mul(Ja, TR, t2);
    m3_mul(Jb, RzT, K);
#pragma unroll
    for (int k = 0; k < 9; k++) { A[18 + k] = t1[k]; A[27 + k] = t2[k] + K[k]; }
}

// A^T v of one end of an edge: (P^T v_rho, Q^T v_rho + P^T v_theta)
__device__ __forceinline__ void pg_at_vec(const double* __restrict__ PQ, const double* v, double* o)
{
    double P[9], Q[9], a[3], b[3], c[3];
#pragma unroll
    for (int k = 0; k < 9; k++) { P[k] = PQ[k]; Q[k] = PQ[9 + k]; }
    m3_tvec(P, v, a);
    m3_tvec(Q, v, b);
    m3_tvec(P, v + 3, c);
#pragma unroll
    for (int k = 0; k < 3; k++) { o[k] = a[k]; o[3 + k] = b[k] + c[k]; }
}

__global__ void __launch_bounds__(PG_BLOCK)
pose_graph_kernel(int nodes, int edges, int n_keys, double* __restrict__ poses, const int* __restrict__ fixed, const int* __restrict__ edge_nodes,
                  const double* __restrict__ edge_Z, const double* __restrict__ edge_w, int outer_iters, int cg_iters, double lambda,
                  double step_tol, float* __restrict__ D, double* __restrict__ stats, PoseGraphWs ws)
{
    __shared__ double red[PG_BLOCK];
    const int tid = threadIdx.x;

    // ---- the edges: which are used; the keys of their two ends -----------------------------------------------------------------------
    double used = 0.0;
    for (int e = tid; e < edges; e += PG_BLOCK) {
        const int i = edge_nodes[2 * e], j = edge_nodes[2 * e + 1];
        bool ok = i >= 0 && i < nodes && j >= 0 && j < nodes && i != j;
        for (int k = 0; k < 12; k++) ok = ok && isfinite(edge_Z[(size_t)e * 12 + k]);
        const double wt = edge_w[2 * e], wr = edge_w[2 * e + 1];
        ok = ok && isfinite(wt) && isfinite(wr) && wt >= 0.0 && wr >= 0.0;
        ws.valid[e] = ok ? 1 : 0;
        ws.keys[2 * e] = ok ? ((unsigned)i << PG_KEY_SHIFT) | (unsigned)(2 * e) : PG_NO_KEY;
        ws.keys[2 * e + 1] = ok ? ((unsigned)j << PG_KEY_SHIFT) | (unsigned)(2 * e + 1) : PG_NO_KEY;
        used += ok ? 1.0 : 0.0;
    }
    for (int p = 2 * edges + tid; p < n_keys; p += PG_BLOCK) ws.keys[p] = PG_NO_KEY;
    for (int k = tid; k < nodes; k += PG_BLOCK) {
        ws.start[k] = 0;
        ws.end[k] = 0;
        for (int c = 0; c < 12; c++) ws.x_old[k * 12 + c] = poses[k * 12 + c];
    }
    used = pg_block_sum(used, red);                        // (counts below 2^53: exact in any order)

    // ---- bitonic sort of the keys, ascending: n_keys is a power of two ---------------------------------------------------------------
    for (int k = 2; k <= n_keys; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < (n_keys >> 1); t += PG_BLOCK) {
                const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;
                const unsigned a = ws.keys[lo], b = ws.keys[hi];
                const bool up = (lo & k) == 0;
                if ((a > b) == up) { ws.keys[lo] = b; ws.keys[hi] = a; }
            }
            __syncthreads();
        }
    }
    for (int p = tid; p < 2 * edges; p += PG_BLOCK) {
        const unsigned key = ws.keys[p];
        if (key == PG_NO_KEY) continue;
        const int node = (int)(key >> PG_KEY_SHIFT);
        if (p == 0 || (int)(ws.keys[p - 1] >> PG_KEY_SHIFT) != node) ws.start[node] = p;
        if (p == 2 * edges - 1 || ws.keys[p + 1] == PG_NO_KEY || (int)(ws.keys[p + 1] >> PG_KEY_SHIFT) != node) ws.end[node] = p + 1;
    }
    __syncthreads();
    double n_active = 0.0;
    for (int k = tid; k < nodes; k += PG_BLOCK) {
        bool act = false;
        if (fixed[k] == 0)
            for (int p = ws.start[k]; p < ws.end[k]; p++) {
                const int e = (int)(ws.keys[p] & ((1u << PG_KEY_SHIFT) - 1)) >> 1;
                act = act || (edge_w[2 * e] > 0.0 && edge_w[2 * e + 1] > 0.0);
            }
        ws.active[k] = act ? 1 : 0;
        n_active += act ? 1.0 : 0.0;
    }
    n_active = pg_block_sum(n_active, red);

    double cost0 = 0.0, cost1 = 0.0, last_step = 0.0;
    int outer_used = 0;
    const int outer = n_active > 0.0 ? outer_iters : 0;
    for (int it = 0; it <= outer; it++) {
        const bool last = it == outer;                     // the pass after the last update only takes the cost
        // ---- per edge: residual, Jacobian blocks ---------------------------------------------------------------------------------------
        for (int e = tid; e < edges; e += PG_BLOCK) {
            if (!ws.valid[e]) continue;
            const int i = edge_nodes[2 * e], j = edge_nodes[2 * e + 1];
            double r[6];
            if (last) pg_linearise<false>(poses + i * 12, poses + j * 12, edge_Z + (size_t)e * 12, r, nullptr);
            else pg_linearise<true>(poses + i * 12, poses + j * 12, edge_Z + (size_t)e * 12, r, ws.edge_A + (size_t)e * PG_EDGE_DOUBLES);
#pragma unroll
            for (int c = 0; c < 6; c++) ws.edge_r[(size_t)e * 6 + c] = r[c];
        }
        __syncthreads();
        // ---- per node: the cost of the edges that end in it; for an active node b, the damped diagonal block and its Cholesky factor --------
        double cost = 0.0;
        for (int k = tid; k < nodes; k += PG_BLOCK) {
            const bool act = ws.active[k] != 0 && !last;
            double H11[9], H12[9], H22[9], b[6], node_cost = 0.0;
#pragma unroll
            for (int c = 0; c < 9; c++) H11[c] = H12[c] = H22[c] = 0.0;
#pragma unroll
            for (int c = 0; c < 6; c++) b[c] = 0.0;
            for (int p = ws.start[k]; p < ws.end[k]; p++) {
                const int inc = (int)(ws.keys[p] & ((1u << PG_KEY_SHIFT) - 1)), e = inc >> 1, side = inc & 1;
                const double wt = edge_w[2 * e], wr = edge_w[2 * e + 1];
                double r[6];
#pragma unroll
                for (int c = 0; c < 6; c++) r[c] = ws.edge_r[(size_t)e * 6 + c];
                if (side) node_cost += wt * (r[0] * r[0] + r[1] * r[1] + r[2] * r[2]) + wr * (r[3] * r[3] + r[4] * r[4] + r[5] * r[5]);
                if (!act) continue;
                const double* PQ = ws.edge_A + (size_t)e * PG_EDGE_DOUBLES + side * 18;
                double v[6], g[6], P[9], Q[9], pp[9], pq[9], qq[9];
#pragma unroll
                for (int c = 0; c < 3; c++) { v[c] = wt * r[c]; v[3 + c] = wr * r[3 + c]; }
                pg_at_vec(PQ, v, g);
#pragma unroll
                for (int c = 0; c < 6; c++) b[c] -= g[c];
#pragma unroll
                for (int c = 0; c < 9; c++) { P[c] = PQ[c]; Q[c] = PQ[9 + c]; }
                m3_mul_tn(P, P, pp);
                m3_mul_tn(P, Q, pq);
                m3_mul_tn(Q, Q, qq);
#pragma unroll
                for (int c = 0; c < 9; c++) { H11[c] += wt * pp[c]; H12[c] += wt * pq[c]; H22[c] += wt * qq[c] + wr * pp[c]; }
            }
            cost += node_cost;
#pragma unroll
            for (int c = 0; c < 6; c++) {
                ws.vx[k * 6 + c] = 0.0; ws.vq[k * 6 + c] = 0.0;
                ws.vr[k * 6 + c] = b[c];                  // the start is delta = 0: the first residual is b
            }
            if (!act) {
#pragma unroll
                for (int c = 0; c < 6; c++) { ws.vz[k * 6 + c] = 0.0; ws.vp[k * 6 + c] = 0.0; ws.hd[k * 6 + c] = 0.0; }
                continue;
            }
            double Hm[6][6], L[6][6];
#pragma unroll
            for (int r_ = 0; r_ < 3; r_++)
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    Hm[r_][c] = H11[r_ * 3 + c]; Hm[r_][3 + c] = H12[r_ * 3 + c];
                    Hm[3 + r_][c] = H12[c * 3 + r_]; Hm[3 + r_][3 + c] = H22[r_ * 3 + c];
                }
#pragma unroll
            for (int c = 0; c < 6; c++) { ws.hd[k * 6 + c] = lambda * Hm[c][c]; Hm[c][c] += lambda * Hm[c][c]; }
#pragma unroll
            for (int r_ = 0; r_ < 6; r_++)
#pragma unroll
                for (int c = 0; c < 6; c++) L[r_][c] = 0.0;
#pragma unroll
            for (int c = 0; c < 6; c++) {
                double d = Hm[c][c];
#pragma unroll
                for (int m = 0; m < c; m++) d -= L[c][m] * L[c][m];
                d = sqrt(d);
                L[c][c] = d;
#pragma unroll
                for (int r_ = c + 1; r_ < 6; r_++) {
                    double s = Hm[r_][c];
#pragma unroll
                    for (int m = 0; m < c; m++) s -= L[r_][m] * L[c][m];
                    L[r_][c] = s / d;
                }
            }
#pragma unroll
            for (int r_ = 0; r_ < 6; r_++)
#pragma unroll
                for (int c = 0; c < 6; c++) ws.chol[k * 36 + r_ * 6 + c] = L[r_][c];
        }
        cost = pg_block_sum(cost, red);
        if (it == 0) cost0 = cost;
        cost1 = cost;
        if (last) break;

        // ---- conjugate gradients on (H + lambda diag H) x = b, block-Jacobi preconditioned ----------------------------------------------
        auto precondition = [&]() {                          // z = M^-1 r, p = z where `first`
            for (int k = tid; k < nodes; k += PG_BLOCK) {
                if (!ws.active[k]) continue;
                double L[6][6], y[6];
#pragma unroll
                for (int r_ = 0; r_ < 6; r_++)
#pragma unroll
                    for (int c = 0; c < 6; c++) L[r_][c] = ws.chol[k * 36 + r_ * 6 + c];
#pragma unroll
                for (int c = 0; c < 6; c++) {
                    double s = ws.vr[k * 6 + c];
#pragma unroll
                    for (int m = 0; m < c; m++) s -= L[c][m] * y[m];
                    y[c] = s / L[c][c];
                }
#pragma unroll
                for (int c = 5; c >= 0; c--) {
                    double s = y[c];
#pragma unroll
                    for (int m = c + 1; m < 6; m++) s -= L[m][c] * y[m];
                    y[c] = s / L[c][c];
                }
#pragma unroll
                for (int c = 0; c < 6; c++) ws.vz[k * 6 + c] = y[c];
            }
            __syncthreads();
        };
        precondition();
        for (int k = tid; k < nodes; k += PG_BLOCK)
#pragma unroll
            for (int c = 0; c < 6; c++) ws.vp[k * 6 + c] = ws.vz[k * 6 + c];
        __syncthreads();
        double rz = pg_dot(ws.vr, ws.vz, nodes, red);
        const double rz_first = rz;
        for (int pass = 0; pass < cg_iters; pass++) {
            if (!(rz > 0.0) || !(rz > 1e-32 * rz_first)) break;       // uniform: every thread holds the same rz
            for (int e = tid; e < edges; e += PG_BLOCK) {     // q = H p, first the two ends of every edge
                if (!ws.valid[e]) continue;
                const int i = edge_nodes[2 * e], j = edge_nodes[2 * e + 1];
                const double* A = ws.edge_A + (size_t)e * PG_EDGE_DOUBLES;
                const double wt = edge_w[2 * e], wr = edge_w[2 * e + 1];
                double pi[6], pj[6], u[6], a[3], o[6];
#pragma unroll
                for (int c = 0; c < 6; c++) { pi[c] = ws.vp[i * 6 + c]; pj[c] = ws.vp[j * 6 + c]; u[c] = 0.0; }
#pragma unroll
                for (int side = 0; side < 2; side++) {
                    const double* PQ = A + side * 18;
                    const double* pv = side ? pj : pi;
                    double P[9], Q[9];
#pragma unroll
                    for (int c = 0; c < 9; c++) { P[c] = PQ[c]; Q[c] = PQ[9 + c]; }
                    m3_vec(P, pv, a);
                    u[0] += a[0]; u[1] += a[1]; u[2] += a[2];
                    m3_vec(Q, pv + 3, a);
                    u[0] += a[0]; u[1] += a[1]; u[2] += a[2];
                    m3_vec(P, pv + 3, a);
                    u[3] += a[0]; u[4] += a[1]; u[5] += a[2];
                }
#pragma unroll
                for (int c = 0; c < 3; c++) { u[c] *= wt; u[3 + c] *= wr; }
                pg_at_vec(A, u, o);
#pragma unroll
                for (int c = 0; c < 6; c++) ws.con[(size_t)(2 * e) * 6 + c] = o[c];
                pg_at_vec(A + 18, u, o);
#pragma unroll
                for (int c = 0; c < 6; c++) ws.con[(size_t)(2 * e + 1) * 6 + c] = o[c];
            }
            __syncthreads();
            for (int k = tid; k < nodes; k += PG_BLOCK) {    // ... then every active node gathers its list, in order
                if (!ws.active[k]) continue;
                double q[6];
#pragma unroll
                for (int c = 0; c < 6; c++) q[c] = 0.0;
                for (int p = ws.start[k]; p < ws.end[k]; p++) {
                    const size_t inc = ws.keys[p] & ((1u << PG_KEY_SHIFT) - 1);
#pragma unroll
                    for (int c = 0; c < 6; c++) q[c] += ws.con[inc * 6 + c];
                }
#pragma unroll
                for (int c = 0; c < 6; c++) ws.vq[k * 6 + c] = q[c] + ws.hd[k * 6 + c] * ws.vp[k * 6 + c];
            }
            __syncthreads();
            const double pq = pg_dot(ws.vp, ws.vq, nodes, red);
            if (!(pq > 0.0)) break;
            const double alpha = rz / pq;
            for (int k = tid; k < nodes; k += PG_BLOCK)
#pragma unroll
                for (int c = 0; c < 6; c++) {
                    ws.vx[k * 6 + c] += alpha * ws.vp[k * 6 + c];
                    ws.vr[k * 6 + c] -= alpha * ws.vq[k * 6 + c];
                }
            __syncthreads();
            precondition();
            const double rz_new = pg_dot(ws.vr, ws.vz, nodes, red);
            const double beta = rz_new / rz;
            rz = rz_new;
            for (int k = tid; k < nodes; k += PG_BLOCK)
#pragma unroll
                for (int c = 0; c < 6; c++) ws.vp[k * 6 + c] = ws.vz[k * 6 + c] + beta * ws.vp[k * 6 + c];
            __syncthreads();
        }
        // ---- X_k <- Exp(delta_k) X_k ---------------------------------------------------------------------------------------------------
        const double step2 = pg_dot(ws.vx, ws.vx, nodes, red);
        for (int k = tid; k < nodes; k += PG_BLOCK) {
            if (!ws.active[k]) continue;
            double tau[6], Rd[9], td[3], R[9], t[3], Rn[9], tn[3];
            bool moved = false;
#pragma unroll
            for (int c = 0; c < 6; c++) { tau[c] = ws.vx[k * 6 + c]; moved = moved || tau[c] != 0.0; }
            if (!moved) continue;
            pg_exp(tau, Rd, td);
            pg_load_pose(poses + k * 12, R, t);
            m3_mul(Rd, R, Rn);
            m3_vec(Rd, t, tn);
#pragma unroll
            for (int r_ = 0; r_ < 3; r_++) {
                poses[k * 12 + r_ * 4] = Rn[r_ * 3]; poses[k * 12 + r_ * 4 + 1] = Rn[r_ * 3 + 1]; poses[k * 12 + r_ * 4 + 2] = Rn[r_ * 3 + 2];
                poses[k * 12 + r_ * 4 + 3] = tn[r_] + td[r_];
            }
        }
        __syncthreads();
        last_step = sqrt(step2);
        outer_used = it + 1;
        if (last_step <= step_tol && it + 1 < outer) it = outer - 1;     // the next pass is the cost pass
    }

    // ---- D_k = X_new^-1 X_old; the largest correction -----------------------------------------------------------------------------------
    double max_t = 0.0, max_a = 0.0;
    for (int k = tid; k < nodes; k += PG_BLOCK) {
        bool same = true;
        for (int c = 0; c < 12; c++) same = same && poses[k * 12 + c] == ws.x_old[k * 12 + c];
        double Rd[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0}, td[3] = {0.0, 0.0, 0.0};
        if (!same) {
            double Rn[9], tn[3], Ro[9], to[3], dt[3];
            pg_load_pose(poses + k * 12, Rn, tn);
            pg_load_pose(ws.x_old + k * 12, Ro, to);
            m3_mul_tn(Rn, Ro, Rd);
#pragma unroll
            for (int c = 0; c < 3; c++) dt[c] = to[c] - tn[c];
            m3_tvec(Rn, dt, td);
            const double ax[3] = {Rd[7] - Rd[5], Rd[2] - Rd[6], Rd[3] - Rd[1]};
            double c_ = 0.5 * (Rd[0] + Rd[4] + Rd[8] - 1.0);
            c_ = c_ < -1.0 ? -1.0 : (c_ > 1.0 ? 1.0 : c_);
            max_a = fmax(max_a, atan2(0.5 * sqrt(ax[0] * ax[0] + ax[1] * ax[1] + ax[2] * ax[2]), c_));
            max_t = fmax(max_t, sqrt(td[0] * td[0] + td[1] * td[1] + td[2] * td[2]));
        }
#pragma unroll
        for (int r_ = 0; r_ < 3; r_++) {
            D[k * 12 + r_ * 4] = (float)Rd[r_ * 3]; D[k * 12 + r_ * 4 + 1] = (float)Rd[r_ * 3 + 1]; D[k * 12 + r_ * 4 + 2] = (float)Rd[r_ * 3 + 2];
            D[k * 12 + r_ * 4 + 3] = (float)td[r_];
        }
    }
    max_t = pg_block_max(max_t, red);
    max_a = pg_block_max(max_a, red);
    if (tid == 0) {
        stats[0] = cost0; stats[1] = cost1; stats[2] = (double)outer_used; stats[3] = last_step;
        stats[4] = used; stats[5] = (double)edges - used; stats[6] = max_t; stats[7] = max_a;
    }
}

// ---- gsr_map_correct -----------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(MAPC_BLOCK) map_quat_kernel(int nodes, const float* __restrict__ D, float* __restrict__ quat)
{
    const int k = blockIdx.x * MAPC_BLOCK + threadIdx.x;
    if (k >= nodes) return;
    double R[9];
#pragma unroll
    for (int r = 0; r < 3; r++) { R[r * 3] = D[k * 12 + r * 4]; R[r * 3 + 1] = D[k * 12 + r * 4 + 1]; R[r * 3 + 2] = D[k * 12 + r * 4 + 2]; }
    double w, x, y, z;
    const double T = R[0] + R[4] + R[8];
    if (T > 0.0) {
        const double s = 2.0 * sqrt(1.0 + T);
        w = 0.25 * s; x = (R[7] - R[5]) / s; y = (R[2] - R[6]) / s; z = (R[3] - R[1]) / s;
    } else if (R[0] >= R[4] && R[0] >= R[8]) {
        const double s = 2.0 * sqrt(1.0 + R[0] - R[4] - R[8]);
        w = (R[7] - R[5]) / s; x = 0.25 * s; y = (R[1] + R[3]) / s; z = (R[2] + R[6]) / s;
    } else if (R[4] >= R[8]) {
        const double s = 2.0 * sqrt(1.0 + R[4] - R[0] - R[8]);
        w = (R[2] - R[6]) / s; x = (R[1] + R[3]) / s; y = 0.25 * s; z = (R[5] + R[7]) / s;
    } else {
        const double s = 2.0 * sqrt(1.0 + R[8] - R[0] - R[4]);
        w = (R[3] - R[1]) / s; x = (R[2] + R[6]) / s; y = (R[5] + R[7]) / s; z = 0.25 * s;
    }
    double n = 1.0 / sqrt(w * w + x * x + y * y + z * z);
    if (w < 0.0) n = -n;
    reinterpret_cast<float4*>(quat)[k] = make_float4((float)(w * n), (float)(x * n), (float)(y * n), (float)(z * n));
}

__device__ __forceinline__ int mapc_slot(int id, int frames, int nodes, const int* __restrict__ slot_of_frame)
{
    if (id < 0 || id >= frames) return -1;
    const int s = slot_of_frame[id];
    return (s < 0 || s >= nodes) ? -1 : s;
}

// x <- R x + t and q <- q_D (x) q of one Gaussian, the header's operation order
__device__ __forceinline__ void mapc_move(const float* __restrict__ Dk, const float4 a, float* x, float4& q)
{
    const float x0 = x[0], x1 = x[1], x2 = x[2];
#pragma unroll
    for (int r = 0; r < 3; r++) x[r] = __fmaf_rn(Dk[r * 4 + 2], x2, __fmaf_rn(Dk[r * 4 + 1], x1, __fmaf_rn(Dk[r * 4], x0, Dk[r * 4 + 3])));
    const float w = q.x, qx = q.y, qy = q.z, qz = q.w;                    // the model's order: (w, x, y, z)
    q.x = __fmaf_rn(-a.w, qz, __fmaf_rn(-a.z, qy, __fmaf_rn(-a.y, qx, __fmul_rn(a.x, w))));
    q.y = __fmaf_rn(-a.w, qy, __fmaf_rn(a.z, qz, __fmaf_rn(a.y, w, __fmul_rn(a.x, qx))));
    q.z = __fmaf_rn(a.w, qx, __fmaf_rn(a.z, w, __fmaf_rn(-a.y, qz, __fmul_rn(a.x, qy))));
    q.w = __fmaf_rn(a.w, w, __fmaf_rn(-a.z, qx, __fmaf_rn(a.y, qy, __fmul_rn(a.x, qz))));
}

__global__ void __launch_bounds__(MAPC_BLOCK)
map_correct_kernel(int P, float* __restrict__ xyz, float* __restrict__ rotation, const int* __restrict__ kf_id, int frames,
                   const int* __restrict__ slot_of_frame, int nodes, const float* __restrict__ D, const float* __restrict__ quat)
{
    const int64_t g = (int64_t)blockIdx.x * MAPC_BLOCK + threadIdx.x;      // the group of four Gaussians 4 g .. 4 g + 3
    const int64_t first = 4 * g;
    if (first >= P) return;
    if (first + 4 <= P) {
        const int4 ids = reinterpret_cast<const int4*>(kf_id)[g];
        const int s[4] = {mapc_slot(ids.x, frames, nodes, slot_of_frame), mapc_slot(ids.y, frames, nodes, slot_of_frame),
                          mapc_slot(ids.z, frames, nodes, slot_of_frame), mapc_slot(ids.w, frames, nodes, slot_of_frame)};
        if ((s[0] & s[1] & s[2] & s[3]) < 0) return;       // all four miss: nothing is read or written
        float4* xp = reinterpret_cast<float4*>(xyz) + 3 * g;
        float4* qp = reinterpret_cast<float4*>(rotation) + 4 * g;
        const float4 v0 = xp[0], v1 = xp[1], v2 = xp[2];
        float x[12] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w, v2.x, v2.y, v2.z, v2.w};
        float4 q[4] = {qp[0], qp[1], qp[2], qp[3]};
#pragma unroll
        for (int m = 0; m < 4; m++)
            if (s[m] >= 0) mapc_move(D + s[m] * 12, reinterpret_cast<const float4*>(quat)[s[m]], x + 3 * m, q[m]);
        xp[0] = make_float4(x[0], x[1], x[2], x[3]);
        xp[1] = make_float4(x[4], x[5], x[6], x[7]);
        xp[2] = make_float4(x[8], x[9], x[10], x[11]);
#pragma unroll
        for (int m = 0; m < 4; m++) qp[m] = q[m];
        return;
    }
    for (int64_t n = first; n < P; n++) {                  // the last P % 4
        const int s = mapc_slot(kf_id[n], frames, nodes, slot_of_frame);
        if (s < 0) continue;
        float x[3] = {xyz[n * 3], xyz[n * 3 + 1], xyz[n * 3 + 2]};
        float4 q = reinterpret_cast<float4*>(rotation)[n];
        mapc_move(D + s * 12, reinterpret_cast<const float4*>(quat)[s], x, q);
        xyz[n * 3] = x[0]; xyz[n * 3 + 1] = x[1]; xyz[n * 3 + 2] = x[2];
        reinterpret_cast<float4*>(rotation)[n] = q;
    }
}

}  // namespace gsr
