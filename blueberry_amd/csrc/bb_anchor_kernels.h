// bb_anchor_kernels.h -- the landmark constraints of docs/SPEC.md 2.5.5: L' kept rows of
// geodesics, resident in the run's dtype as A[a][v] (n_pad values per row, 0 = no term), add
//     lambda * sum_a sum_v A_av^-q (|x_{s_a} - x_v|_eps - A_av)^2
// to the stress and its gradient to the exchange buffer [g * 2 * bin_scale | stress hi | lo] the
// reduce has left (bb_solver_device.h: kReduceExchange).  Three launches, no floating-point
// atomics, every sum in an order fixed by (n_bins, L') alone:
//   anchor_node_kernel      a thread owns node v: the landmarks' coordinates in LDS, a ascending
//                           over the coalesced A[a][v], g_v and the stress share in registers
//                           (float64 sums of terms formed in the run's dtype), ONE
//                           read-modify-write of exch[3v..] with the bin's step factor applied as
//                           gradient_element applies it; the workgroup's stress to its own slot
//   anchor_landmark_kernel  workgroup (chunk c, landmark a): -sum_v f_av over the chunk's
//                           kAnchorChunk nodes, re-reading the row, to slot (a, c)
//   anchor_fold_kernel      a workgroup per landmark: its slots added in a fixed order into
//                           exch[3 s_a ..]; the first one folds the stress slots into hi / lo
// and the conversion of the float64 rows of a bb_paths into A (through bb_wish.h's flush: the
// one value rule), gfx950 only.  (The two kernels behind bb_solver_anchor_sums are compiled with
// the reduce, in bb_solver_kernels.h: see there.)  Included by
// bb_solver_anchors.hip and by nothing else; the fold modes (AnchorFold), which the callers of
// launch_anchors name, are in bb_solver_device.h.
#pragma once

#include "bb_solver_device.h"

namespace {

constexpr int kAnchorMaxRows = 1024;    // BB_PATHS_MAX_SOURCES: what the LDS stage holds
constexpr int kAnchorChunk = 1024;      // nodes of one workgroup of the landmark side

// One term (a, v) with delta = A_av > 0 and (dx, dy, dz) = x_v - x_{s_a}, in the run's dtype:
// st = lambda w (d - delta)^2 and coef = lambda w (d - delta) / d, w = delta^-Q; the factor 2 of
// the gradient is applied where the sum leaves the kernel, as in the reduce.
template <typename T, int Q>
__device__ __forceinline__ void anchor_term(T delta, T lam, T dx, T dy, T dz, T &coef, T &st) {
    const T d2 = fma(dx, dx, fma(dy, dy, fma(dz, dz, Traits<T>::eps2())));  // SPEC 2.2
    const T dist = sqrt(d2);
    const T res = dist - delta;
    T w = lam;
    if constexpr (Q >= 1) w = w / delta;
    if constexpr (Q == 2) w = w / delta;
    const T wr = w * res;
    st = wr * res;
    coef = wr / dist;
}

// exch[o] += the gradient element whose partial sum is tot, scaled as gradient_element scales
template <typename T>
__device__ __forceinline__ void anchor_add(T *__restrict__ exch, const T *__restrict__ bin_scale,
                                           int64_t v, int c, double tot) {
    const T t = (T)tot;
    const T g = bin_scale ? bin_scale[v] * (T(2) * t) : T(2) * t;
    exch[3 * v + c] = exch[3 * v + c] + g;
}

// The sums of a 256-thread workgroup's values, in a fixed order: the DPP tree of each wave, then the
// four waves in wave order through LDS.  Called by every thread; the totals are valid in thread 0.
template <int N>
__device__ __forceinline__ void anchor_block_sum(double (&v)[N], double (*sh)[4], int tid) {
#pragma unroll
    for (int k = 0; k < N; ++k) {
        v[k] = wave_sum_hi(v[k]);
        if ((tid & 63) == 63) sh[k][tid >> 6] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] = ((sh[k][0] + sh[k][1]) + sh[k][2]) + sh[k][3];
}

template <typename T, int Q>
__global__ __launch_bounds__(256) void anchor_node_kernel(
    const T *__restrict__ A, int64_t n_pad, int64_t n_bins, int n_rows, const int *__restrict__ nodes,
    const T *__restrict__ X, T *__restrict__ exch, const T *__restrict__ bin_scale, T lam,
    double *__restrict__ stress_part) {
    __shared__ T lx[kAnchorMaxRows * 3];
    __shared__ double sh[1][4];
    const int tid = threadIdx.x;
    for (int q = tid; q < n_rows * 3; q += 256) lx[q] = X[3 * (int64_t)nodes[q / 3] + q % 3];
    __syncthreads();
    const int64_t v = (int64_t)blockIdx.x * 256 + tid;
    double gx = 0.0, gy = 0.0, gz = 0.0, st = 0.0;
    bool any = false;
    if (v < n_bins) {
        const T xv = X[3 * v], yv = X[3 * v + 1], zv = X[3 * v + 2];
        for (int a0 = 0; a0 < n_rows; a0 += 8) {
            T d[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) d[q] = a0 + q < n_rows ? A[(int64_t)(a0 + q) * n_pad + v] : T(0);
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                if (d[q] > T(0)) {
                    const int a = a0 + q;
                    const T dx = xv - lx[3 * a], dy = yv - lx[3 * a + 1], dz = zv - lx[3 * a + 2];
                    T coef, t;
                    anchor_term<T, Q>(d[q], lam, dx, dy, dz, coef, t);
                    gx += (double)(coef * dx); gy += (double)(coef * dy); gz += (double)(coef * dz);
                    st += (double)t;
                    any = true;
                }
            }
        }
    }
    if (any && exch != nullptr) {
        anchor_add(exch, bin_scale, v, 0, gx);
        anchor_add(exch, bin_scale, v, 1, gy);
        anchor_add(exch, bin_scale, v, 2, gz);
    }
    double tot[1] = {st};
    anchor_block_sum(tot, sh, tid);
    if (tid == 0) stress_part[blockIdx.x] = tot[0];
}

template <typename T, int Q>
__global__ __launch_bounds__(256) void anchor_landmark_kernel(
    const T *__restrict__ A, int64_t n_pad, int64_t n_bins, const int *__restrict__ nodes,
    const T *__restrict__ X, T lam, double *__restrict__ lm_part) {
    __shared__ double sh[3][4];
    const int tid = threadIdx.x;
    const int a = blockIdx.y;
    const int64_t s = nodes[a];
    const T xs = X[3 * s], ys = X[3 * s + 1], zs = X[3 * s + 2];
    const T *__restrict__ row = A + (int64_t)a * n_pad;
    double gx = 0.0, gy = 0.0, gz = 0.0;
    T d[kAnchorChunk / 256];
    int64_t v[kAnchorChunk / 256];
#pragma unroll
    for (int k = 0; k < kAnchorChunk / 256; ++k) {
        v[k] = (int64_t)blockIdx.x * kAnchorChunk + k * 256 + tid;
        d[k] = v[k] < n_bins ? row[v[k]] : T(0);
    }
#pragma unroll
    for (int k = 0; k < kAnchorChunk / 256; ++k) {
        if (d[k] > T(0)) {
            const T dx = X[3 * v[k]] - xs, dy = X[3 * v[k] + 1] - ys, dz = X[3 * v[k] + 2] - zs;
            T coef, t;
            anchor_term<T, Q>(d[k], lam, dx, dy, dz, coef, t);
            gx -= (double)(coef * dx); gy -= (double)(coef * dy); gz -= (double)(coef * dz);
        }
    }
    double g[3] = {gx, gy, gz};
    anchor_block_sum(g, sh, tid);
    if (tid == 0) {
        double *out = lm_part + ((int64_t)a * gridDim.x + blockIdx.x) * 3;
        out[0] = g[0]; out[1] = g[1]; out[2] = g[2];
    }
}

// Workgroup a (exchange mode: one per kept landmark; else one in all): landmark a's slots added --
// thread t the chunks t, t + 256, ... in order, then anchor_block_sum -- into exch[3 s_a ..]; the
// first workgroup also folds the stress slots the same way.
template <typename T>
__global__ __launch_bounds__(256) void anchor_fold_kernel(
    int mode, const double *__restrict__ stress_part, int n_node_blocks,
    const double *__restrict__ lm_part, int n_chunks, const int *__restrict__ nodes,
    T *__restrict__ exch, const T *__restrict__ bin_scale, int64_t n_pad,
    double *__restrict__ anchor_stress, double *__restrict__ stress_out) {
    __shared__ double sh[3][4];
    const int tid = threadIdx.x;
    if (blockIdx.x == 0) {
        double part[1] = {0.0};
        for (int i = tid; i < n_node_blocks; i += 256) part[0] += stress_part[i];
        anchor_block_sum(part, sh, tid);
        if (tid == 0) {
            const double Sa = part[0];
            anchor_stress[0] = Sa;
            if (mode == kAnchorFoldExchange) {
                const int64_t n3 = 3 * n_pad;
                T hi, lo;
                split_hi_lo((double)exch[n3] + (double)exch[n3 + 1] + Sa, hi, lo);
                exch[n3] = hi;
                exch[n3 + 1] = lo;
            } else if (mode == kAnchorFoldStress) {
                stress_out[0] += Sa;
            }
        }
        __syncthreads();                                   // (sh is used again below)
    }
    if (mode != kAnchorFoldExchange) return;
    // (the kept landmarks are distinct nodes: nobody else writes these three elements)
    const int a = blockIdx.x;
    double g[3] = {0.0, 0.0, 0.0};
    for (int c = tid; c < n_chunks; c += 256)
#pragma unroll
        for (int k = 0; k < 3; ++k) g[k] += lm_part[((int64_t)a * n_chunks + c) * 3 + k];
    anchor_block_sum(g, sh, tid);
    if (tid == 0) {
        const int64_t s = nodes[a];
#pragma unroll
        for (int k = 0; k < 3; ++k) anchor_add(exch, bin_scale, s, k, g[k]);
    }
}

// ---- A from the float64 rows of a bb_paths: D is (n_nodes, ld), node-major, +inf = no path ----
// A[a][v] = flush_wish<T>(D[v][col[a]]) (+inf and the 0 of a landmark's own node flush to 0),
// 0 in the padding; 64 x 64 tiles through LDS so that both sides are coalesced.  terms[0] += the
// values kept (an integer sum).
template <typename T>
__global__ __launch_bounds__(256) void anchor_rows_kernel(const double *__restrict__ D, int64_t ld,
                                                          int64_t n_nodes, int64_t n_pad,
                                                          const int *__restrict__ col, int n_rows,
                                                          T *__restrict__ A,
                                                          unsigned long long *__restrict__ terms) {
    __shared__ double tile[64][65];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t v0 = (int64_t)blockIdx.x * 64;
    const int a0 = (int)blockIdx.y * 64;
    for (int r = w; r < 64; r += 4) {
        const int64_t v = v0 + r;
        const int a = a0 + lane;
        tile[r][lane] = (v < n_nodes && a < n_rows) ? D[v * ld + col[a]] : 0.0;
    }
    __syncthreads();
    int kept = 0;
    for (int j = w; j < 64; j += 4) {
        const int a = a0 + j;
        const int64_t v = v0 + lane;
        if (a < n_rows && v < n_pad) {
            const T val = flush_wish<T>(tile[lane][j]);
            A[(int64_t)a * n_pad + v] = val;
            kept += val > T(0) ? 1 : 0;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) kept += __shfl_down(kept, off, 64);
    if (lane == 0 && kept > 0) atomicAdd(terms, (unsigned long long)kept);
}

}  // namespace
