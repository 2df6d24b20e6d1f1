// bb_balance.hip -- from raw counts to a balanced map on the device (docs/SPEC.md 2.5.2): the
// bias vector of iterative correction (Imakaev et al. 2012) and the distance-decay expected of
// the balanced map, both over the leading n x n block (n = n_bins = d - 1) of the resident
// (d, d) float64 matrix.  Row and column n_bins are never read.  Like symv, only the UPPER
// triangle is read (8 B per pair) and the matrix is taken to be symmetric.
//
//   band_symv_kernel   y = A x, A_ij = M_ij for |i - j| >= ignore_diags: symv_upper_kernel's
//                      layout (64 rows x up to 4,096 columns per work item, 16 loads of 512
//                      contiguous bytes in flight per wave, row partials per segment, column
//                      partials per row block) with the band test where the products are
//                      formed -- a cell inside the band is SELECTED out, never multiplied by 0
//                      and never subtracted afterwards, so every sum is a sum of non-negative
//                      terms.  Three cell rules share the kernel: the value (the iteration and
//                      the mask's fixed point), "is not 0" (min_nnz) and "is negative or not
//                      finite" (the input check).  bb::symv_reduce_kernel adds the partials.
//   balance_*_kernel   the mask, and one step of the loop (s, mean, var, the stopping rule,
//                      b and x) in ONE workgroup: every sum in a fixed order, the loop's state
//                      on the device.  A stopped loop turns later launches into no-ops, so the
//                      host enqueues a batch of iterations per scalar read-back.
//   diag_sums_kernel   sum_k and cnt_k of every diagonal in one read of the upper triangle:
//                      row r of a wave loads its 64-element chunk r columns later, so that a
//                      lane holds ONE diagonal for all 16 rows and adds them into one register
//                      (no cross-lane traffic); the 4 waves meet in LDS; one partial per (row
//                      block, diagonal).  diag_reduce_kernel adds a diagonal's partials in
//                      list order, in 8 slices.
// No floating-point atomics anywhere: the same bits on every run (SPEC 2.7).  Traffic and the
// reasons for a second product kernel beside symv's: DESIGN.md 4.15.
#include <float.h>
#include <math.h>

#include <algorithm>
#include <string>
#include <vector>

#include "bb_cm_internal.h"
#include "bb_common.h"

namespace {

using bb::kSvGroup;
using bb::kSvRows;
using bb::kSvSeg;
using bb::lds_barrier;

// ---- the banded product -----------------------------------------------------------------------
enum { kCellValue = 0, kCellNonzero = 1, kCellBad = 2 };

// What a cell contributes, formed as the cell is loaded.  Under kCellBad the column side is
// switched off (its multiplier x_row is taken as 0), so that every cell of the counted upper
// triangle is seen once, by the row side: sum(y) = the number of offending cells.
template <int MODE>
__device__ __forceinline__ double cell_term(double a) {
    if (MODE == kCellValue) return a;
    if (MODE == kCellNonzero) return a != 0.0 ? 1.0 : 0.0;
    return !(a >= 0.0 && a <= DBL_MAX) ? 1.0 : 0.0;      // negative, NaN, +inf
}

// `stop` (may be NULL): the loop's "stopped" word; a launch enqueued behind the stop returns.
template <int MODE>
__global__ __launch_bounds__(256, 2) void band_symv_kernel(const double *__restrict__ m, int64_t ld,
                                                           int64_t n, int64_t ignore,
                                                           const double *__restrict__ x,
                                                           const int2 *__restrict__ items,
                                                           double *__restrict__ rowpart,
                                                           double *__restrict__ colpart,
                                                           const int *__restrict__ stop) {
    if (stop != nullptr && *stop != 0) return;
    __shared__ double meet[4][kSvGroup][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int2 it = items[blockIdx.x];
    const int64_t I = it.x, S = it.y;
    const int64_t row0 = I * kSvRows + wave * 16;
    const int64_t c_begin = std::max<int64_t>(I * kSvRows, S * kSvSeg);
    const int64_t c_end = std::min<int64_t>(n, (S + 1) * (int64_t)kSvSeg);
    // a cell (row, c) counts on the row side from c = row + ignore on; on the column side the
    // diagonal never counts (it would add m_ii x_i twice)
    const int64_t off_row = ignore, off_col = std::max<int64_t>(ignore, 1);
    double xr[16], racc[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        xr[r] = (MODE != kCellBad && row0 + r < n) ? x[row0 + r] : 0.0;
        racc[r] = 0.0;
    }
    for (int64_t cg = c_begin; cg < c_end; cg += 64 * kSvGroup) {
        double cacc[kSvGroup];
#pragma unroll
        for (int g = 0; g < kSvGroup; ++g) {
            cacc[g] = 0.0;
            const int64_t c0 = cg + 64 * g;              // chunk start (uniform)
            if (c0 >= c_end) continue;
            const int64_t c = c0 + lane;
            const bool in_c = c < c_end;
            const double xc = in_c ? x[c] : 0.0;
            double a[16];
#pragma unroll
            for (int r = 0; r < 16; ++r)
                a[r] = (in_c && row0 + r < n) ? cell_term<MODE>(m[(row0 + r) * ld + c]) : 0.0;
            if (c0 < row0 + 16 + off_col) {
                // the chunk reaches into the band (or below the diagonal) of this wave's rows
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int64_t row = row0 + r;
                    const double v = a[r];
                    racc[r] = fma(c >= row + off_row ? v : 0.0, xc, racc[r]);
                    cacc[g] = fma(c >= row + off_col ? v : 0.0, xr[r], cacc[g]);
                }
            } else {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    racc[r] = fma(a[r], xc, racc[r]);
                    cacc[g] = fma(a[r], xr[r], cacc[g]);
                }
            }
        }
#pragma unroll
        for (int g = 0; g < kSvGroup; ++g) meet[wave][g][lane] = cacc[g];
        lds_barrier();   // (LDS only: nobody reads the global cells stored here)
        for (int j = threadIdx.x; j < 64 * kSvGroup; j += 256) {
            const int g = j >> 6, l = j & 63;
            const int64_t c = cg + j;
            if (c < c_end)
                colpart[I * n + c] = ((meet[0][g][l] + meet[1][g][l]) + meet[2][g][l]) + meet[3][g][l];
        }
        lds_barrier();
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        double v = racc[r];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
        if (lane == 0 && row0 + r < n) rowpart[S * n + row0 + r] = v;
    }
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

// Sum of one value per thread of a 1024-thread workgroup through sh[1024]: a binary tree in a
// fixed order; every thread gets the total.
template <typename T>
__device__ __forceinline__ T block_sum_1024(T v, T *sh) {
    __syncthreads();                       // sh may still be read from the sum before
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int off = 512; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) sh[threadIdx.x] += sh[threadIdx.x + off];
        __syncthreads();
    }
    return sh[0];
}

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
    killed = block_sum_1024(killed, sh);
    alive = block_sum_1024(alive, sh);
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
    const double mean = block_sum_1024(acc, sh) / n_live;
    acc = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += 1024)
        if (live[i]) {
            const double t = x[i] * y[i] / mean - 1.0;
            acc += t * t;
        }
    const double var = block_sum_1024(acc, sh) / n_live;
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
inline size_t round256(size_t b) { return (b + 255) & ~(size_t)255; }

// The work list of the diagonal pass: every (row block I, diagonal segment S) with a cell,
// longest first.
std::vector<int2> diag_items(int64_t n) {
    const int64_t nrb = (n + kSvRows - 1) / kSvRows;
    auto len = [&](const int2 &t) {
        return std::min<int64_t>(n - (int64_t)t.x * kSvRows, (t.y + 1) * (int64_t)kSvSeg) -
               (int64_t)t.y * kSvSeg;
    };
    std::vector<int2> items;
    for (int64_t I = 0; I < nrb; ++I)
        for (int64_t S = 0; S * kSvSeg < n - I * kSvRows; ++S) items.push_back(make_int2((int)I, (int)S));
    std::stable_sort(items.begin(), items.end(),
                     [&](const int2 &a, const int2 &b) { return len(a) > len(b); });
    return items;
}

// The handle's scratch for an n x n leading block: product work list | diagonal work list |
// partial sums (of whichever call runs: the product's row and column partials, or the diagonal
// pass's sums and counts).  Made on first use and whenever n has changed (filter).
struct BalanceScratch {
    const int2 *items, *diag;
    void *part;
    int64_t nseg, nrb;
};
hipError_t balance_scratch(bb_cm *cm, int64_t n, BalanceScratch *out) {
    const int64_t nrb = (n + kSvRows - 1) / kSvRows, nseg = (n + kSvSeg - 1) / kSvSeg;
    const size_t part_bytes = std::max((size_t)(nseg + nrb) * (size_t)n * 8, (size_t)nrb * (size_t)n * 12);
    if (cm->bal_n != n) {
        const std::vector<int2> items = bb::symv_items(n), diag = diag_items(n);
        const size_t ib = round256(items.size() * sizeof(int2)), db = round256(diag.size() * sizeof(int2));
        cm->bal_n = -1;
        hipError_t e = cm->bal.reserve(ib + db + part_bytes);
        if (e == hipSuccess)
            e = hipMemcpyAsync(cm->bal.p, items.data(), items.size() * sizeof(int2), hipMemcpyHostToDevice,
                               cm->stream);
        if (e == hipSuccess)
            e = hipMemcpyAsync((char *)cm->bal.p + ib, diag.data(), diag.size() * sizeof(int2),
                               hipMemcpyHostToDevice, cm->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(cm->stream);   // the lists die with this scope
        if (e != hipSuccess) return e;
        cm->bal_items = (int)items.size();
        cm->bal_diag_items = (int)diag.size();
        cm->bal_n = n;
    }
    const size_t ib = round256((size_t)cm->bal_items * sizeof(int2));
    const size_t db = round256((size_t)cm->bal_diag_items * sizeof(int2));
    out->items = (const int2 *)cm->bal.p;
    out->diag = (const int2 *)((char *)cm->bal.p + ib);
    out->part = (char *)cm->bal.p + ib + db;
    out->nseg = nseg;
    out->nrb = nrb;
    return hipSuccess;
}

// y = A x under cell rule MODE, enqueued on the handle's stream
template <int MODE>
hipError_t band_symv_enqueue(bb_cm *cm, const BalanceScratch &sc, int64_t n, int64_t ignore,
                             const double *dx, double *dy, const int *stop) {
    double *rowpart = (double *)sc.part, *colpart = rowpart + sc.nseg * n;
    hipError_t e = bb::launch(band_symv_kernel<MODE>, dim3((unsigned)cm->bal_items), dim3(256), 0, cm->stream,
                              (const double *)cm->m, cm->d, n, ignore, dx, sc.items, rowpart, colpart, stop);
    if (e == hipSuccess)
        e = bb::launch(bb::symv_reduce_kernel, dim3((unsigned)((n + 127) / 128)), dim3(1024), 0, cm->stream,
                       (const double *)rowpart, (const double *)colpart, n, (int)sc.nseg, dy);
    return e;
}

int cm_enter(const bb_cm *cm, int64_t n_bins, const char *who) {
    if (!cm) return bb::fail(BB_ERR_INVALID, std::string(who) + ": contact map is NULL");
    BB_TRY(bb::enter_device(cm->device));
    if (!(n_bins >= 0 && n_bins + 1 == cm->d))
        return bb::fail(BB_ERR_INVALID,
                        std::string(who) + ": the matrix edge is not n_bins + 1 (filtered already?)");
    return BB_OK;
}

// iterations enqueued per read-back of the loop's state: a launch behind the stop costs a few
// microseconds, a read-back a synchronisation
constexpr int kBalanceBatch = 16;

}  // namespace

extern "C" {

int bb_cm_balance(bb_cm *cm, int64_t n_bins, int64_t ignore_diags, int64_t min_nnz, double tol,
                  int64_t max_iter, double row_sum, double *bias, uint8_t *masked, int64_t *iterations,
                  double *variance) {
    BB_TRY(cm_enter(cm, n_bins, "bb_cm_balance"));
    BB_REQUIRE(bias != nullptr && masked != nullptr, "bb_cm_balance: NULL argument");
    BB_REQUIRE(ignore_diags >= 0 && min_nnz >= 0, "bb_cm_balance: ignore_diags / min_nnz is negative");
    BB_REQUIRE(tol >= 0.0 && tol <= DBL_MAX && max_iter >= 0, "bb_cm_balance: bad tol / max_iter");
    BB_REQUIRE(row_sum == row_sum && row_sum <= DBL_MAX, "bb_cm_balance: row_sum is not finite");
    const int64_t n = n_bins;
    ignore_diags = std::min(ignore_diags, n);         // (beyond n - 1 nothing is counted anyway)
    BB_REQUIRE(n >= 1, "bb_cm_balance: no bin is left to balance (the map has no bins)");
    BalanceScratch sc;
    BB_TRY(bb::hip_status("bb_cm_balance", balance_scratch(cm, n, &sc), BB_ERR_NOMEM));
    bb::DevBuf bx, bbias, by, blive, bst;
    hipError_t e = bx.alloc((size_t)n * 8);
    if (e == hipSuccess) e = bbias.alloc((size_t)n * 8);
    if (e == hipSuccess) e = by.alloc((size_t)n * 8);
    if (e == hipSuccess) e = blive.alloc((size_t)n);
    if (e == hipSuccess) e = bst.alloc(sizeof(BalanceState));
    BB_TRY(bb::hip_status("bb_cm_balance", e, BB_ERR_NOMEM));
    hipStream_t st = cm->stream;
    double *x = (double *)bx.p, *b = (double *)bbias.p, *y = (double *)by.p;
    unsigned char *live = (unsigned char *)blive.p;
    BalanceState *dst = (BalanceState *)bst.p;
    const dim3 gvec((unsigned)((n + 255) / 256)), b256(256);
    std::vector<double> host((size_t)n);

    // 1. the input check: one pass over the counted upper triangle
    e = hipMemsetAsync(dst, 0, sizeof(BalanceState), st);
    if (e == hipSuccess) e = bb::launch(fill_kernel, gvec, b256, 0, st, x, 1.0, n);
    if (e == hipSuccess) e = band_symv_enqueue<kCellBad>(cm, sc, n, ignore_diags, x, y, nullptr);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e == hipSuccess) e = hipMemcpy(host.data(), y, (size_t)n * 8, hipMemcpyDeviceToHost);
    BB_TRY(bb::hip_status("bb_cm_balance", e));
    double n_bad = 0.0;
    for (int64_t i = 0; i < n; ++i) n_bad += host[(size_t)i];     // small integers: exact
    if (n_bad != 0.0)
        return bb::fail(BB_ERR_INVALID, "bb_cm_balance: " + std::to_string((long long)n_bad) +
                                            " counted cells of the upper triangle are negative or not "
                                            "finite; the map was left as it is");

    // 2. the mask: min_nnz on the raw map, once; then zero marginals over the live bins, to the
    //    fixed point (the product of the round that changes nothing is iteration 0's)
    if (min_nnz > 0) {
        e = band_symv_enqueue<kCellNonzero>(cm, sc, n, ignore_diags, x, y, nullptr);
        if (e == hipSuccess)
            e = bb::launch(balance_start_kernel, gvec, b256, 0, st, (const double *)y, (double)min_nnz, n,
                           live, x, b);
    } else {
        e = bb::launch(balance_start_kernel, gvec, b256, 0, st, (const double *)nullptr, 0.0, n, live, x, b);
    }
    BalanceState hs;
    hs.changed = 1;
    hs.n_live = 0;
    while (e == hipSuccess && hs.changed != 0) {
        e = band_symv_enqueue<kCellValue>(cm, sc, n, ignore_diags, x, y, nullptr);
        if (e == hipSuccess)
            e = bb::launch(balance_mask_kernel, dim3(1), dim3(1024), 0, st, (const double *)y, n, live, x, dst);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e == hipSuccess) e = hipMemcpy(&hs, dst, sizeof(hs), hipMemcpyDeviceToHost);
    }
    BB_TRY(bb::hip_status("bb_cm_balance", e));
    if (hs.n_live == 0)
        return bb::fail(BB_ERR_INVALID,
                        "bb_cm_balance: no live bin is left (every bin is masked: min_nnz, or no "
                        "count outside the ignored diagonals)");

    // 3. the loop: y holds A x of iteration 0
    e = bb::launch(balance_step_kernel, dim3(1), dim3(1024), 0, st, (const double *)y, n,
                   (const unsigned char *)live, x, b, tol, (long long)max_iter, dst);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e == hipSuccess) e = hipMemcpy(&hs, dst, sizeof(hs), hipMemcpyDeviceToHost);
    while (e == hipSuccess && hs.stopped == 0) {
        // at most the updates that are left, and the evaluation at which `it == max_iter` stops
        const int batch = (int)std::min<int64_t>(kBalanceBatch, max_iter - hs.it + 1);
        for (int q = 0; q < batch && e == hipSuccess; ++q) {
            e = band_symv_enqueue<kCellValue>(cm, sc, n, ignore_diags, x, y, &dst->stopped);
            if (e == hipSuccess)
                e = bb::launch(balance_step_kernel, dim3(1), dim3(1024), 0, st, (const double *)y, n,
                               (const unsigned char *)live, x, b, tol, (long long)max_iter, dst);
        }
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e == hipSuccess) e = hipMemcpy(&hs, dst, sizeof(hs), hipMemcpyDeviceToHost);
    }
    std::vector<unsigned char> hlive((size_t)n);
    if (e == hipSuccess) e = hipMemcpy(host.data(), b, (size_t)n * 8, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(hlive.data(), live, (size_t)n, hipMemcpyDeviceToHost);
    BB_TRY(bb::hip_status("bb_cm_balance", e));

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

int bb_cm_expected(bb_cm *cm, int64_t n_bins, const double *bias, double *sums, int64_t *counts) {
    BB_TRY(cm_enter(cm, n_bins, "bb_cm_expected"));
    BB_REQUIRE(sums != nullptr && counts != nullptr, "bb_cm_expected: NULL argument");
    const int64_t n = n_bins;
    if (n == 0) return BB_OK;
    BalanceScratch sc;
    BB_TRY(bb::hip_status("bb_cm_expected", balance_scratch(cm, n, &sc), BB_ERR_NOMEM));
    bb::DevBuf bx, bs, bc;
    hipError_t e = bx.alloc((size_t)n * 8);
    if (e == hipSuccess) e = bs.alloc((size_t)n * 8);
    if (e == hipSuccess) e = bc.alloc((size_t)n * 8);
    BB_TRY(bb::hip_status("bb_cm_expected", e, BB_ERR_NOMEM));
    hipStream_t st = cm->stream;
    double *x = (double *)bx.p;
    double *sumpart = (double *)sc.part;
    int *cntpart = (int *)(sumpart + sc.nrb * n);
    const dim3 grid((unsigned)cm->bal_diag_items), b256(256);
    if (bias != nullptr) {
        // (the sums vector doubles as the staging place of the bias)
        e = hipMemcpyAsync(bs.p, bias, (size_t)n * 8, hipMemcpyHostToDevice, st);
        if (e == hipSuccess)
            e = bb::launch(inverse_bias_kernel, dim3((unsigned)((n + 255) / 256)), b256, 0, st,
                           (const double *)bs.p, x, n);
        if (e == hipSuccess)
            e = bb::launch(diag_sums_kernel<true>, grid, b256, 0, st, (const double *)cm->m, cm->d, n,
                           (const double *)x, sc.diag, sumpart, cntpart);
    } else {
        e = bb::launch(diag_sums_kernel<false>, grid, b256, 0, st, (const double *)cm->m, cm->d, n,
                       (const double *)nullptr, sc.diag, sumpart, cntpart);
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
