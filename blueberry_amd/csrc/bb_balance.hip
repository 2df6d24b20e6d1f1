// bb_balance.hip -- from raw counts to a balanced map on the device (docs/SPEC.md 2.5.2): the
// bias vector of iterative correction (Imakaev et al. 2012) and the distance-decay expected of
// the balanced map, both over the leading n x n block (n = n_bins = d - 1) of the resident
// (d, d) float64 matrix.  Row and column n_bins are never read.  Like symv, only the UPPER
// triangle is read (8 B per pair) and the matrix is taken to be symmetric.
//
//   band_symv_kernel   y = A x, A_ij = M_ij for |i - j| >= ignore_diags: the product's one body
//                      (bb::symv_item, bb_cm_internal.h) over the leading n x n block, row
//                      stride d, the band's edge as the offsets from which a cell counts.  Every
//                      sum is a sum of non-negative terms.  Three cell rules: the value (the
//                      iteration, the mask's fixed point), "is not 0" (min_nnz), "is negative
//                      or not finite" (the input check).  bb::symv_reduce_kernel adds the partials.
//   balance_*_kernel   the mask, and one step of the loop (s, mean, var, the stopping rule,
//                      b and x) in ONE workgroup: every sum in a fixed order, the loop's state
//                      on the device.  A stopped loop turns later launches into no-ops, so the
//                      host enqueues a batch of iterations per scalar read-back.
//   bb::balance_loop   the whole of 2.5.2 around a product it is GIVEN (bb_balance_loop.h):
//                      bb_cm_balance passes the banded product, bb_triples_balance.hip the
//                      product over its index of resident triples (SPEC 2.5.3).
//   diag_sums_kernel   sum_k and cnt_k of every diagonal in one read of the upper triangle:
//                      row r of a wave loads its 64-element chunk r columns later, so that a
//                      lane holds ONE diagonal for all 16 rows and adds them into one register
//                      (no cross-lane traffic); the 4 waves meet in LDS; one partial per (row
//                      block, diagonal).  diag_reduce_kernel adds a diagonal's partials in
//                      list order, in 8 slices.
// No floating-point atomics anywhere: the same bits on every run (SPEC 2.7).  Traffic, and why
// the product has two entry points and no runtime flag: DESIGN.md 4.15.
#include <float.h>
#include <math.h>

#include <algorithm>
#include <string>
#include <vector>

#include "bb_balance_loop.h"
#include "bb_cm_internal.h"
#include "bb_common.h"

namespace {

using bb::kCellBad;
using bb::kCellNonzero;
using bb::kCellValue;
using bb::kSvGroup;
using bb::kSvRows;
using bb::kSvSeg;
using bb::lds_barrier;

// ---- the banded product -----------------------------------------------------------------------
// `stop` (may be NULL): the loop's "stopped" word; a launch enqueued behind the stop returns.
// A cell (row, c) counts on the row side from c = row + ignore on; on the column side the
// diagonal never counts either.
template <int MODE>
__global__ __launch_bounds__(256, 2) void band_symv_kernel(const double *__restrict__ m, int64_t ld,
                                                           int64_t n, int64_t ignore,
                                                           const double *__restrict__ x,
                                                           const int2 *__restrict__ items,
                                                           double *__restrict__ rowpart,
                                                           double *__restrict__ colpart,
                                                           const int *__restrict__ stop) {
    if (stop != nullptr && *stop != 0) return;
    bb::symv_item<MODE>(m, ld, n, ignore, std::max<int64_t>(ignore, 1), x, items, rowpart, colpart);
}

// ---- the loop's vectors and state --------------------------------------------------------------
struct BalanceState {
    int stopped;          // the loop has ended: later launches of the batch do nothing
    int changed;          // bins the last mask round killed
    long long it;         // updates made
    long long n_live;
    double mean, var;     // of the last evaluated iteration
    double mean0;         // of iteration 0
};

__global__ __launch_bounds__(256) void fill_kernel(double *__restrict__ v, double value, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) v[i] = value;
}

// b = 1; bin i starts live unless its count of non-zero counted cells is below min_nnz
// (nnz == NULL: no such rule); x = the 0/1 indicator of the live bins
__global__ __launch_bounds__(256) void balance_start_kernel(const double *__restrict__ nnz, double min_nnz,
                                                            int64_t n, unsigned char *__restrict__ live,
                                                            double *__restrict__ x, double *__restrict__ b) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const bool on = nnz == nullptr || nnz[i] >= min_nnz;
    live[i] = on ? 1 : 0;
    x[i] = on ? 1.0 : 0.0;
    b[i] = 1.0;
}

// One round of the mask's fixed point: y = A x for the indicator x; a live bin whose marginal
// over the live bins is 0 dies.  (A sum of non-negative terms is 0 exactly when every term is.)
__global__ __launch_bounds__(1024) void balance_mask_kernel(const double *__restrict__ y, int64_t n,
                                                            unsigned char *__restrict__ live,
                                                            double *__restrict__ x,
                                                            BalanceState *__restrict__ st) {
    __shared__ long long sh[1024];
    long long killed = 0, alive = 0;
    for (int64_t i = threadIdx.x; i < n; i += 1024) {
        const bool was = live[i] != 0, now = was && y[i] > 0.0;
        killed += was && !now;
        alive += now;
        live[i] = now ? 1 : 0;
        x[i] = now ? 1.0 : 0.0;
    }
    killed = bb::block_sum<1024>(killed, sh);
    __syncthreads();                              // sh[0] has been read: sh is free again
    alive = bb::block_sum<1024>(alive, sh);
    if (threadIdx.x == 0) {
        st->changed = (int)std::min<long long>(killed, 1);
        st->n_live = alive;
    }
}

// One pass of the loop (SPEC 2.5.2) on y = A x:  s_i = x_i y_i over the live bins, their mean,
// the variance of s / mean, the stopping rule, and -- unless it stops -- b_i *= s_i / mean,
// x_i = 1 / b_i.  One workgroup: thread t adds bins t, t + 1024, ... in order, then the tree.
__global__ __launch_bounds__(1024) void balance_step_kernel(const double *__restrict__ y, int64_t n,
                                                            const unsigned char *__restrict__ live,
                                                            double *__restrict__ x, double *__restrict__ b,
                                                            double tol, long long max_iter,
                                                            BalanceState *__restrict__ st) {
    __shared__ double sh[1024];
    if (st->stopped != 0) return;                 // (uniform: written by this kernel alone)
    const long long it = st->it;
    const double n_live = (double)st->n_live;
    double acc = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += 1024)
        if (live[i]) acc += x[i] * y[i];
    const double mean = bb::block_sum<1024>(acc, sh) / n_live;
    acc = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += 1024)
        if (live[i]) {
            const double t = x[i] * y[i] / mean - 1.0;
            acc += t * t;
        }
    __syncthreads();                              // sh[0] has been read: sh is free again
    const double var = bb::block_sum<1024>(acc, sh) / n_live;
    const bool stop = var < tol || it == max_iter;
    if (!stop)
        for (int64_t i = threadIdx.x; i < n; i += 1024)
            if (live[i]) {
                const double bi = b[i] * (x[i] * y[i] / mean);
                b[i] = bi;
                x[i] = 1.0 / bi;
            }
    __syncthreads();                              // every thread has read st->it
    if (threadIdx.x == 0) {
        st->mean = mean;
        st->var = var;
        if (it == 0) st->mean0 = mean;
        if (stop) st->stopped = 1; else st->it = it + 1;
    }
}

// ---- the distance-decay expected ----------------------------------------------------------------
// x = 1 / bias, 0 where the bias is NaN
__global__ __launch_bounds__(256) void inverse_bias_kernel(const double *__restrict__ bias,
                                                           double *__restrict__ x, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double bi = bias[i];
    x[i] = bi != bi ? 0.0 : 1.0 / bi;
}

// Work item (I, S): rows 64 I .. 64 I + 63, diagonals S kSvSeg .. (S + 1) kSvSeg of the ones the
// row block has (k < n - 64 I).  Lane l of a wave holds diagonal k0 + l: its cell in row i is
// column i + k0 + l, so the wave's load for row i is the 512 contiguous bytes from column
// i + k0 on.  HAS_X = false: all weights are 1 (no bias vector is read).
// A pair with x_i x_j == 0 is not counted and not added (selected out: its cell may hold anything).
template <bool HAS_X>
__global__ __launch_bounds__(256, 2) void diag_sums_kernel(const double *__restrict__ m, int64_t ld,
                                                           int64_t n, const double *__restrict__ x,
                                                           const int2 *__restrict__ items,
                                                           double *__restrict__ sumpart,
                                                           int *__restrict__ cntpart) {
    __shared__ double meet[4][kSvGroup][64];
    __shared__ int meetc[4][kSvGroup][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int2 it = items[blockIdx.x];
    const int64_t I = it.x, S = it.y;
    const int64_t row0 = I * kSvRows + wave * 16;
    const int64_t k_begin = S * kSvSeg;
    const int64_t k_end = std::min<int64_t>(n - I * kSvRows, (S + 1) * (int64_t)kSvSeg);
    double xr[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) xr[r] = HAS_X ? (row0 + r < n ? x[row0 + r] : 0.0) : 1.0;
    for (int64_t kg = k_begin; kg < k_end; kg += 64 * kSvGroup) {
        double acc[kSvGroup];
        int cnt[kSvGroup];
#pragma unroll
        for (int g = 0; g < kSvGroup; ++g) {
            acc[g] = 0.0;
            cnt[g] = 0;
            const int64_t k0 = kg + 64 * g;              // first diagonal of the chunk (uniform)
            if (k0 >= k_end) continue;
            const int64_t k = k0 + lane;
            double a[16], p[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int64_t i = row0 + r, c = i + k;
                const bool in = k < k_end && c < n;       // (c < n implies i < n)
                a[r] = in ? m[i * ld + c] : 0.0;
                p[r] = in ? (HAS_X ? xr[r] * x[c] : 1.0) : 0.0;
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const bool on = p[r] != 0.0;
                acc[g] = on ? fma(a[r], p[r], acc[g]) : acc[g];
                cnt[g] += on ? 1 : 0;
            }
        }
#pragma unroll
        for (int g = 0; g < kSvGroup; ++g) {
            meet[wave][g][lane] = acc[g];
            meetc[wave][g][lane] = cnt[g];
        }
        lds_barrier();   // (LDS only: nobody reads the global cells stored here)
        for (int j = threadIdx.x; j < 64 * kSvGroup; j += 256) {
            const int g = j >> 6, l = j & 63;
            const int64_t k = kg + j;
            if (k < k_end) {
                sumpart[I * n + k] = ((meet[0][g][l] + meet[1][g][l]) + meet[2][g][l]) + meet[3][g][l];
                cntpart[I * n + k] = meetc[0][g][l] + meetc[1][g][l] + meetc[2][g][l] + meetc[3][g][l];
            }
        }
        lds_barrier();
    }
}

// sums[k], counts[k] = diagonal k's partials of the row blocks 0 .. (n - 1 - k) / 64, in order,
// cut into 8 slices that are added in slice order (as symv_reduce_kernel)
__global__ __launch_bounds__(1024) void diag_reduce_kernel(const double *__restrict__ sumpart,
                                                           const int *__restrict__ cntpart, int64_t n,
                                                           double *__restrict__ sums,
                                                           long long *__restrict__ counts) {
    __shared__ double meet[8][128];
    __shared__ long long meetc[8][128];
    const int el = threadIdx.x & 127, sl = threadIdx.x >> 7;
    const int64_t k = (int64_t)blockIdx.x * 128 + el;
    double acc = 0.0;
    long long cnt = 0;
    if (k < n) {
        const int64_t nb = (n - 1 - k) / kSvRows + 1;
        const int64_t per = (nb + 7) / 8, b0 = sl * per, b1 = std::min<int64_t>(nb, b0 + per);
        for (int64_t b = b0; b < b1; b += 8) {
            double v[8];
            int c[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const bool in = b + q < b1;
                v[q] = in ? sumpart[(b + q) * n + k] : 0.0;
                c[q] = in ? cntpart[(b + q) * n + k] : 0;
            }
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                acc += v[q];
                cnt += c[q];
            }
        }
    }
    meet[sl][el] = acc;
    meetc[sl][el] = cnt;
    __syncthreads();
    if (sl == 0 && k < n) {
        double t = meet[0][el];
        long long tc = meetc[0][el];
#pragma unroll
        for (int q = 1; q < 8; ++q) {
            t += meet[q][el];
            tc += meetc[q][el];
        }
        sums[k] = t;
        counts[k] = tc;
    }
}

// ---- host side ---------------------------------------------------------------------------------
// y = A x under cell rule MODE over the handle's prepared scratch, enqueued on its stream
template <int MODE>
hipError_t band_symv_enqueue(bb_cm *cm, int64_t ignore, const double *dx, double *dy, const int *stop) {
    return bb::product_enqueue(cm->bal, cm->stream, dy,
                               [&](dim3 grid, const int2 *items, double *rowpart, double *colpart) {
                                   return bb::launch(band_symv_kernel<MODE>, grid, dim3(256), 0, cm->stream,
                                                     (const double *)cm->m, cm->d, cm->bal.n, ignore, dx,
                                                     items, rowpart, colpart, stop);
                               });
}

// iterations enqueued per read-back of the loop's state: a launch behind the stop costs a few
// microseconds, a read-back a synchronisation
constexpr int kBalanceBatch = 16;

}  // namespace

namespace bb {

hipError_t inverse_bias_enqueue(const double *bias, double *x, int64_t n, hipStream_t st) {
    return launch(inverse_bias_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, bias, x, n);
}

int balance_loop(const char *who_, int64_t n, hipStream_t st, const BalanceProduct &product,
                 int64_t min_nnz, double tol, int64_t max_iter, double row_sum, double *bias,
                 uint8_t *masked, int64_t *iterations, double *variance) {
    const std::string who(who_);
    DevBuf bx, bbias, by, blive, bst;
    hipError_t e = bx.alloc((size_t)n * 8);
    if (e == hipSuccess) e = bbias.alloc((size_t)n * 8);
    if (e == hipSuccess) e = by.alloc((size_t)n * 8);
    if (e == hipSuccess) e = blive.alloc((size_t)n);
    if (e == hipSuccess) e = bst.alloc(sizeof(BalanceState));
    BB_TRY(hip_status(who_, e, BB_ERR_NOMEM));
    double *x = (double *)bx.p, *b = (double *)bbias.p, *y = (double *)by.p;
    unsigned char *live = (unsigned char *)blive.p;
    BalanceState *dst = (BalanceState *)bst.p;
    const dim3 gvec((unsigned)((n + 255) / 256)), b256(256);
    std::vector<double> host((size_t)n);

    // 1. the input check: one pass over the counted upper triangle
    e = hipMemsetAsync(dst, 0, sizeof(BalanceState), st);
    if (e == hipSuccess) e = launch(fill_kernel, gvec, b256, 0, st, x, 1.0, n);
    if (e == hipSuccess) e = product(kCellBad, x, y, nullptr);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e == hipSuccess) e = hipMemcpy(host.data(), y, (size_t)n * 8, hipMemcpyDeviceToHost);
    BB_TRY(hip_status(who_, e));
    double n_bad = 0.0;
    for (int64_t i = 0; i < n; ++i) n_bad += host[(size_t)i];     // small integers: exact
    if (n_bad != 0.0)
        return fail(BB_ERR_INVALID, who + ": " + std::to_string((long long)n_bad) +
                                        " counted cells of the upper triangle are negative or not "
                                        "finite; the map was left as it is");

    // 2. the mask: min_nnz on the raw map, once; then zero marginals over the live bins, to the
    //    fixed point (the product of the round that changes nothing is iteration 0's)
    if (min_nnz > 0) {
        e = product(kCellNonzero, x, y, nullptr);
        if (e == hipSuccess)
            e = launch(balance_start_kernel, gvec, b256, 0, st, (const double *)y, (double)min_nnz, n,
                       live, x, b);
    } else {
        e = launch(balance_start_kernel, gvec, b256, 0, st, (const double *)nullptr, 0.0, n, live, x, b);
    }
    BalanceState hs;
    hs.changed = 1;
    hs.n_live = 0;
    while (e == hipSuccess && hs.changed != 0) {
        e = product(kCellValue, x, y, nullptr);
        if (e == hipSuccess)
            e = launch(balance_mask_kernel, dim3(1), dim3(1024), 0, st, (const double *)y, n, live, x, dst);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e == hipSuccess) e = hipMemcpy(&hs, dst, sizeof(hs), hipMemcpyDeviceToHost);
    }
    BB_TRY(hip_status(who_, e));
    if (hs.n_live == 0)
        return fail(BB_ERR_INVALID,
                    who + ": no live bin is left (every bin is masked: min_nnz, or no "
                          "count outside the ignored diagonals)");

    // 3. the loop: y holds A x of iteration 0
    e = launch(balance_step_kernel, dim3(1), dim3(1024), 0, st, (const double *)y, n,
               (const unsigned char *)live, x, b, tol, (long long)max_iter, dst);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e == hipSuccess) e = hipMemcpy(&hs, dst, sizeof(hs), hipMemcpyDeviceToHost);
    while (e == hipSuccess && hs.stopped == 0) {
        // at most the updates that are left, and the evaluation at which `it == max_iter` stops
        const int batch = (int)std::min<int64_t>(kBalanceBatch, max_iter - hs.it + 1);
        for (int q = 0; q < batch && e == hipSuccess; ++q) {
            e = product(kCellValue, x, y, &dst->stopped);
            if (e == hipSuccess)
                e = launch(balance_step_kernel, dim3(1), dim3(1024), 0, st, (const double *)y, n,
                           (const unsigned char *)live, x, b, tol, (long long)max_iter, dst);
        }
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e == hipSuccess) e = hipMemcpy(&hs, dst, sizeof(hs), hipMemcpyDeviceToHost);
    }
    std::vector<unsigned char> hlive((size_t)n);
    if (e == hipSuccess) e = hipMemcpy(host.data(), b, (size_t)n * 8, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(hlive.data(), live, (size_t)n, hipMemcpyDeviceToHost);
    BB_TRY(hip_status(who_, e));

    // 4. the scale: the balanced map's mean row sum becomes row_sum, or stays the input's
    const double target = row_sum > 0.0 ? row_sum : hs.mean0;
    const double f = sqrt(hs.mean / target);
    for (int64_t i = 0; i < n; ++i) {
        masked[i] = hlive[(size_t)i] ? 0 : 1;
        bias[i] = hlive[(size_t)i] ? host[(size_t)i] * f : (double)NAN;
    }
    if (iterations) *iterations = hs.it;
    if (variance) *variance = hs.var;
    return BB_OK;
}

}  // namespace bb

extern "C" {

int bb_cm_balance(bb_cm *cm, int64_t n_bins, int64_t ignore_diags, int64_t min_nnz, double tol,
                  int64_t max_iter, double row_sum, double *bias, uint8_t *masked, int64_t *iterations,
                  double *variance) {
    BB_TRY(bb::cm_check(cm, "bb_cm_balance"));
    BB_TRY(bb::cm_check_bins(cm, n_bins, "bb_cm_balance"));
    BB_TRY(bb::balance_check_args("bb_cm_balance", n_bins, ignore_diags, min_nnz, tol, max_iter, row_sum,
                                  bias, masked));
    const int64_t n = n_bins;
    ignore_diags = std::min(ignore_diags, n);         // (beyond n - 1 nothing is counted anyway)
    BB_TRY(bb::hip_status("bb_cm_balance", cm->bal.prepare(n, true, cm->stream), BB_ERR_NOMEM));
    return bb::balance_loop(
        "bb_cm_balance", n, cm->stream,
        [&](int mode, const double *x, double *y, const int *stop) {
            if (mode == kCellBad) return band_symv_enqueue<kCellBad>(cm, ignore_diags, x, y, stop);
            if (mode == kCellNonzero) return band_symv_enqueue<kCellNonzero>(cm, ignore_diags, x, y, stop);
            return band_symv_enqueue<kCellValue>(cm, ignore_diags, x, y, stop);
        },
        min_nnz, tol, max_iter, row_sum, bias, masked, iterations, variance);
}

int bb_cm_expected(bb_cm *cm, int64_t n_bins, const double *bias, double *sums, int64_t *counts) {
    BB_TRY(bb::cm_check(cm, "bb_cm_expected"));
    BB_TRY(bb::cm_check_bins(cm, n_bins, "bb_cm_expected"));
    BB_REQUIRE(sums != nullptr && counts != nullptr, "bb_cm_expected: NULL argument");
    const int64_t n = n_bins;
    if (n == 0) return BB_OK;
    BB_TRY(bb::hip_status("bb_cm_expected", cm->bal.prepare(n, true, cm->stream), BB_ERR_NOMEM));
    bb::DevBuf bx, bs, bc;
    hipError_t e = bx.alloc((size_t)n * 8);
    if (e == hipSuccess) e = bs.alloc((size_t)n * 8);
    if (e == hipSuccess) e = bc.alloc((size_t)n * 8);
    BB_TRY(bb::hip_status("bb_cm_expected", e, BB_ERR_NOMEM));
    hipStream_t st = cm->stream;
    double *x = (double *)bx.p;
    const int2 *diag = cm->bal.diag();
    double *sumpart = (double *)cm->bal.part();
    int *cntpart = (int *)(sumpart + cm->bal.nrb() * n);
    const dim3 grid((unsigned)cm->bal.n_diag), b256(256);
    if (bias != nullptr) {
        // (the sums vector doubles as the staging place of the bias)
        e = hipMemcpyAsync(bs.p, bias, (size_t)n * 8, hipMemcpyHostToDevice, st);
        if (e == hipSuccess)
            e = bb::launch(inverse_bias_kernel, dim3((unsigned)((n + 255) / 256)), b256, 0, st,
                           (const double *)bs.p, x, n);
        if (e == hipSuccess)
            e = bb::launch(diag_sums_kernel<true>, grid, b256, 0, st, (const double *)cm->m, cm->d, n,
                           (const double *)x, diag, sumpart, cntpart);
    } else {
        e = bb::launch(diag_sums_kernel<false>, grid, b256, 0, st, (const double *)cm->m, cm->d, n,
                       (const double *)nullptr, diag, sumpart, cntpart);
    }
    if (e == hipSuccess)
        e = bb::launch(diag_reduce_kernel, dim3((unsigned)((n + 127) / 128)), dim3(1024), 0, st,
                       (const double *)sumpart, (const int *)cntpart, n, (double *)bs.p, (long long *)bc.p);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e == hipSuccess) e = hipMemcpy(sums, bs.p, (size_t)n * 8, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(counts, bc.p, (size_t)n * 8, hipMemcpyDeviceToHost);
    return bb::hip_status("bb_cm_expected", e);
}

}  // extern "C"
