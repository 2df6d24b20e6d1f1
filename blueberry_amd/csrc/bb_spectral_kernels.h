// bb_spectral_kernels.h -- device code of the spectral start of the 3D-structure solver
// (gfx950 only).  Included by bb_solver_spectral.hip and by nothing else.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bb_device_sums.h"

namespace {

// --------------------------------------------------------------------------
// spectral start on the device (bb_solver_spectral_init): the N x 3 side of the block
// power iteration.  All of it is O(N): one workgroup, fixed-order sums.
// --------------------------------------------------------------------------
// out[0..8] = A^T B (3 x 3) and out[9..11] = column sums of A, over n rows of (n,3) arrays
template <typename TA, typename TB>
__global__ __launch_bounds__(1024) void gram3_kernel(const TA *__restrict__ A,
                                                     const TB *__restrict__ B, int64_t n,
                                                     double *__restrict__ out) {
    __shared__ double sh[12][16];
    double acc[12];
#pragma unroll
    for (int q = 0; q < 12; ++q) acc[q] = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += 1024) {
        const double a0 = (double)A[3 * i], a1 = (double)A[3 * i + 1], a2 = (double)A[3 * i + 2];
        const double b0 = (double)B[3 * i], b1 = (double)B[3 * i + 1], b2 = (double)B[3 * i + 2];
        acc[0] = fma(a0, b0, acc[0]); acc[1] = fma(a0, b1, acc[1]); acc[2] = fma(a0, b2, acc[2]);
        acc[3] = fma(a1, b0, acc[3]); acc[4] = fma(a1, b1, acc[4]); acc[5] = fma(a1, b2, acc[5]);
        acc[6] = fma(a2, b0, acc[6]); acc[7] = fma(a2, b1, acc[7]); acc[8] = fma(a2, b2, acc[8]);
        acc[9] += a0; acc[10] += a1; acc[11] += a2;
    }
    bb::wave_sums_to_lds(acc, sh);
    if (threadIdx.x < 12) out[threadIdx.x] = bb::lds_wave_total(sh[threadIdx.x]);
}

// out_i = scale * ((in_i - mean) M), rows i < n_bins; M is 3 x 3 row-major; rows beyond
// n_bins (padding) are written as 0.  The 12 numbers travel as kernel arguments.
struct Affine3 {
    double mean[3], m[9], scale;
};
template <typename TI, typename TO>
__global__ __launch_bounds__(256) void affine3_kernel(const TI *__restrict__ in, TO *__restrict__ out,
                                                      int64_t n_bins, int64_t n_pad, Affine3 a) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_pad) return;
    double o0 = 0.0, o1 = 0.0, o2 = 0.0;
    if (i < n_bins) {
        const double x0 = (double)in[3 * i] - a.mean[0], x1 = (double)in[3 * i + 1] - a.mean[1],
                     x2 = (double)in[3 * i + 2] - a.mean[2];
        o0 = a.scale * (x0 * a.m[0] + x1 * a.m[3] + x2 * a.m[6]);
        o1 = a.scale * (x0 * a.m[1] + x1 * a.m[4] + x2 * a.m[7]);
        o2 = a.scale * (x0 * a.m[2] + x1 * a.m[5] + x2 * a.m[8]);
    }
    out[3 * i] = (TO)o0; out[3 * i + 1] = (TO)o1; out[3 * i + 2] = (TO)o2;
}

// ---- the same N x 3 algebra WITHOUT a host round trip (round 4) -------------------------
// bb_solver_spectral_init used to read 12 sums back four times per product (centre, centre,
// two Cholesky-QR passes): four stream synchronisations around a sweep that takes 0.1 ms on a
// 1/8 share.  Now the 3 x 3 work stays on the device: every pass over an (n,3) array is ONE
// kernel that leaves the 12 sums of its OUTPUT (Gram matrix + column sums) as per-workgroup
// partials, and the NEXT pass adds them in a fixed order and does the 3 x 3 step (mean, or
// Cholesky factor and its inverse) in its own prologue.  A factor that is not positive definite
// (the iterate lost rank) raises a flag the host reads once, at the end.  Sums are in double,
// fixed order: bitwise reproducible, and identical on every rank of a multi-rank start.
constexpr int kSpWG = 256;          // threads per workgroup of the passes
constexpr int kSpMaxGroups = 256;   // partials per pass

// rows [r0, r1) of workgroup g of G over n_pad rows
__device__ __forceinline__ void sp_rows(int64_t n_pad, int64_t &r0, int64_t &r1) {
    const int64_t per = (n_pad + gridDim.x - 1) / gridDim.x;
    r0 = (int64_t)blockIdx.x * per;
    r1 = r0 + per < n_pad ? r0 + per : n_pad;
}
// the workgroup's 12 sums -> partial[blockIdx.x * 12 ..]
__device__ __forceinline__ void sp_store_partial(double (&acc)[12], double *__restrict__ partial) {
    __shared__ double sh[12][kSpWG / 64];
    bb::wave_sums_to_lds(acc, sh);
    if (threadIdx.x < 12) partial[(int64_t)blockIdx.x * 12 + threadIdx.x] = bb::lds_wave_total(sh[threadIdx.x]);
}
__device__ __forceinline__ void sp_accumulate(double (&acc)[12], double a0, double a1, double a2) {
    acc[0] = fma(a0, a0, acc[0]); acc[1] = fma(a0, a1, acc[1]); acc[2] = fma(a0, a2, acc[2]);
    acc[3] = fma(a1, a0, acc[3]); acc[4] = fma(a1, a1, acc[4]); acc[5] = fma(a1, a2, acc[5]);
    acc[6] = fma(a2, a0, acc[6]); acc[7] = fma(a2, a1, acc[7]); acc[8] = fma(a2, a2, acc[8]);
    acc[9] += a0; acc[10] += a1; acc[11] += a2;
}

// partial sums of in^T in and of in's columns (rows < n_bins)
template <typename TI>
__global__ __launch_bounds__(kSpWG) void sp_stats_kernel(const TI *__restrict__ in, int64_t n_bins,
                                                         int64_t n_pad, double *__restrict__ partial) {
    int64_t r0, r1;
    sp_rows(n_pad, r0, r1);
    double acc[12];
#pragma unroll
    for (int q = 0; q < 12; ++q) acc[q] = 0.0;
    for (int64_t i = r0 + threadIdx.x; i < r1 && i < n_bins; i += kSpWG)
        sp_accumulate(acc, (double)in[3 * i], (double)in[3 * i + 1], (double)in[3 * i + 2]);
    sp_store_partial(acc, partial);
}

// the 12 sums themselves (groups added in order), for the stopping rule's one small read-back
__global__ __launch_bounds__(64) void sp_fold_partials_kernel(const double *__restrict__ partial,
                                                              int groups, double *__restrict__ out) {
    if (threadIdx.x >= 12) return;
    double v = 0.0;
    for (int g = 0; g < groups; ++g) v += partial[(int64_t)g * 12 + threadIdx.x];
    out[threadIdx.x] = v;
}

// g = R^T R (R upper) -> R^-1 (upper), 3 x 3 row-major.  False if g is not positive definite.
__host__ __device__ inline bool sp_chol3_inv_upper(const double *g, double *rinv) {
    double r[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int j = 0; j < 3; ++j) {
        double d = g[j * 3 + j];
        for (int k = 0; k < j; ++k) d -= r[k * 3 + j] * r[k * 3 + j];
        if (!(d > 0.0)) return false;
        r[j * 3 + j] = sqrt(d);
        for (int c = j + 1; c < 3; ++c) {
            double v = g[j * 3 + c];
            for (int k = 0; k < j; ++k) v -= r[k * 3 + j] * r[k * 3 + c];
            r[j * 3 + c] = v / r[j * 3 + j];
        }
    }
    for (int q = 0; q < 9; ++q) rinv[q] = 0.0;
    for (int j = 0; j < 3; ++j) {
        rinv[j * 3 + j] = 1.0 / r[j * 3 + j];
        for (int i = j - 1; i >= 0; --i) {
            double v = 0.0;
            for (int k = i + 1; k <= j; ++k) v -= r[i * 3 + k] * rinv[k * 3 + j];
            rinv[i * 3 + j] = v / r[i * 3 + i];
        }
    }
    return true;
}

// The 3 x 3 step BETWEEN two passes, done by every workgroup of the consuming pass for itself
// (round 4, second version: as a kernel of its own it cost what every tiny kernel costs here,
// 4.7 us by the kernel trace, three times per product).  The producer left `groups` partial
// sums of 12 values; 12 x 16 threads add them in a fixed order (thread (q, l) takes the groups
// l, l + 16, ... of value q, then a 16-lane tree), thread 0 does the 3 x 3 step, LDS hands the
// map to everybody.  Every workgroup -- and every rank -- computes the same bits.
//   kSpMean     A = { mean = column sums / n, M = I, scale }           (centring)
//   kSpChol     A = { 0, R^-1, 1 } with R^T R = the Gram matrix        (Cholesky-QR pass)
//   kSpCholMean the same, and B.mean = (column sums / n) R^-1: the mean of what the map is
//               about to produce (sp_affine_centre_kernel)
// A Gram matrix that is not positive definite sets *flag and leaves the identity.
enum { kSpMean = 0, kSpChol = 1, kSpCholMean = 2 };
__device__ __forceinline__ void sp_map_from_partials(const double *__restrict__ partial, int groups,
                                                     int64_t n_bins, int mode, double scale,
                                                     int *__restrict__ flag, Affine3 &A, Affine3 &B) {
    __shared__ double tot[12];
    __shared__ Affine3 maps[2];
    const int t = threadIdx.x;
    if (t < 192) {
        const int q = t >> 4, l = t & 15;
        double v = 0.0;
        for (int g = l; g < groups; g += 16) v += partial[(int64_t)g * 12 + q];
#pragma unroll
        for (int off = 8; off > 0; off >>= 1) v += __shfl_xor(v, off, 16);
        if (l == 0) tot[q] = v;
    }
    __syncthreads();
    if (t == 0) {
        Affine3 a, b;
        for (int k = 0; k < 3; ++k) a.mean[k] = 0.0;
        for (int k = 0; k < 9; ++k) a.m[k] = (k % 4 == 0) ? 1.0 : 0.0;
        a.scale = 1.0;
        b = a;
        if (mode == kSpMean) {
            for (int k = 0; k < 3; ++k) a.mean[k] = tot[9 + k] / (double)n_bins;
            a.scale = scale;
        } else {
            double rinv[9];
            if (!sp_chol3_inv_upper(tot, rinv)) {
                *flag = 1;                       // (every workgroup writes the same 1)
            } else {
                for (int k = 0; k < 9; ++k) a.m[k] = rinv[k];
                b = a;
                const double m0 = tot[9] / (double)n_bins, m1 = tot[10] / (double)n_bins,
                             m2 = tot[11] / (double)n_bins;
                b.mean[0] = m0 * rinv[0] + m1 * rinv[3] + m2 * rinv[6];
                b.mean[1] = m0 * rinv[1] + m1 * rinv[4] + m2 * rinv[7];
                b.mean[2] = m0 * rinv[2] + m1 * rinv[5] + m2 * rinv[8];
            }
        }
        maps[0] = a;
        maps[1] = b;
    }
    __syncthreads();
    A = maps[0];
    B = maps[1];
}

// out_i = A.scale * ((in_i - A.mean) A.m) for rows < n_bins (0 beyond), A = the 3 x 3 step
// `mode` on the producer's partial sums, + the partial sums of the OUTPUT.  In place
// (in == out) is fine: a thread reads its row before it writes it.
template <typename TI>
__global__ __launch_bounds__(kSpWG) void sp_affine_stats_kernel(const TI *in, double *out,
                                                                int64_t n_bins, int64_t n_pad,
                                                                const double *__restrict__ partial_in,
                                                                int groups, int mode, double scale,
                                                                int *__restrict__ flag,
                                                                double *__restrict__ partial) {
    Affine3 A, unused;
    sp_map_from_partials(partial_in, groups, n_bins, mode, scale, flag, A, unused);
    int64_t r0, r1;
    sp_rows(n_pad, r0, r1);
    double acc[12];
#pragma unroll
    for (int q = 0; q < 12; ++q) acc[q] = 0.0;
    for (int64_t i = r0 + threadIdx.x; i < r1; i += kSpWG) {
        double o0 = 0.0, o1 = 0.0, o2 = 0.0;
        if (i < n_bins) {
            const double x0 = (double)in[3 * i] - A.mean[0], x1 = (double)in[3 * i + 1] - A.mean[1],
                         x2 = (double)in[3 * i + 2] - A.mean[2];
            o0 = A.scale * (x0 * A.m[0] + x1 * A.m[3] + x2 * A.m[6]);
            o1 = A.scale * (x0 * A.m[1] + x1 * A.m[4] + x2 * A.m[7]);
            o2 = A.scale * (x0 * A.m[2] + x1 * A.m[5] + x2 * A.m[8]);
            sp_accumulate(acc, o0, o1, o2);
        }
        out[3 * i] = o0; out[3 * i + 1] = o1; out[3 * i + 2] = o2;
    }
    sp_store_partial(acc, partial);
}

// The last pass of an orthonormalisation: V = V' R^-1, written as double, and the sweep's
// right-hand sides mv = (T)(V - mean V) -- V centred, in the solver's type -- in one go; R^-1 and
// the mean from the producer's partial sums (kSpCholMean).
template <typename T>
__global__ __launch_bounds__(kSpWG) void sp_affine_centre_kernel(const double *in, double *out_v,
                                                                 T *__restrict__ out_mv,
                                                                 int64_t n_bins, int64_t n_pad,
                                                                 const double *__restrict__ partial_in,
                                                                 int groups, int *__restrict__ flag) {
    Affine3 A, B;
    sp_map_from_partials(partial_in, groups, n_bins, kSpCholMean, 1.0, flag, A, B);
    const int64_t i = (int64_t)blockIdx.x * kSpWG + threadIdx.x;
    if (i >= n_pad) return;
    double o0 = 0.0, o1 = 0.0, o2 = 0.0, c0 = 0.0, c1 = 0.0, c2 = 0.0;
    if (i < n_bins) {
        const double x0 = in[3 * i], x1 = in[3 * i + 1], x2 = in[3 * i + 2];
        o0 = x0 * A.m[0] + x1 * A.m[3] + x2 * A.m[6];
        o1 = x0 * A.m[1] + x1 * A.m[4] + x2 * A.m[7];
        o2 = x0 * A.m[2] + x1 * A.m[5] + x2 * A.m[8];
        c0 = o0 - B.mean[0]; c1 = o1 - B.mean[1]; c2 = o2 - B.mean[2];
    }
    out_v[3 * i] = o0; out_v[3 * i + 1] = o1; out_v[3 * i + 2] = o2;
    out_mv[3 * i] = (T)c0; out_mv[3 * i + 1] = (T)c1; out_mv[3 * i + 2] = (T)c2;
}

}  // namespace
