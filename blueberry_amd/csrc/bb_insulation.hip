// bb_insulation.hip -- the insulation sums of a map on the device (docs/SPEC.md 2.13):
// bb_cm_insulation (resident dense matrix) and bb_triples_insulation (resident pixel list).  The
// O(n) tail -- score, log2, boundaries -- is host numpy (blueberry_amd/datatypes.py).
//
// The diamond of bin i is the cells (a, b), max(0, i - w + 1) <= a <= i <= b <= min(n - 1, i + w - 1),
// b - a >= g; a cell is live iff x_a != 0 and x_b != 0 (x = 1 / bias, 0 where the bias is NaN).
// sum_i has a FIXED order (SPEC 2.13): per row a of the diamond, top to bottom, a row partial of
// M_ab (x_a x_b) over its live cells, left to right; then the partials top to bottom; every
// accumulator from +0.0.  An accumulator that starts at +0.0 never becomes -0.0, so adding a
// +-0.0 never changes its bits (bb_coarsen.hip): a cell that is 0, dead, outside the diamond or
// absent may be added as 0.0 or skipped.  A dead cell is SELECTED out, never multiplied by 0.
// The product and the sum are two roundings: nothing here may be contracted into an fma.
//
//   insulation_kernel   dense.  A workgroup owns kInsBins consecutive bins i0 .. and walks the
//               band tile they need -- rows [i0 - w + 1, i0 + kInsBins), columns [i0, i0 +
//               kInsBins + w - 1) -- in steps of kInsRows rows x kInsCols columns through LDS:
//               wave v loads rows 4 v .. 4 v + 3 of the step, 2 loads of 64 contiguous doubles
//               per row (8 loads in flight per wave), weighs each cell as it arrives, and the
//               NEXT step's loads are issued before this step's sums (lds_barrier orders LDS
//               only).  The order forbids a tree along a row or across rows, so the parallel
//               items are the (bin, row) pairs: thread (lane, wave) owns bin i0 + lane and rows
//               wave, wave + 4, .. of the step, adds its cells of the step left to right and
//               carries the four row partials in registers across the column chunks.  The 64
//               lanes of a wave walk ONE tile row at consecutive (or, where a + g clamps them,
//               equal) columns: conflict-free without a padded pitch.  After the last column
//               chunk the partials meet in LDS and thread `bin` adds them top to bottom into the
//               register it keeps across the row steps.  Any w works in 24 KB of LDS.
//   triples_insulation_kernel   pixel list, over the canonical index (bb_triples.h): one wave
//               per bin, one lane per row a, 4 bins per workgroup; a lane finds the
//               first column >= max(i, a + g) of its row by binary search and walks while the
//               column is < min(n, i + w).  The 64 partials are added top to bottom by lane
//               reads (every lane carries the same sum; no LDS, no barrier); windows beyond 64
//               rows walk the rows in chunks of 64, carrying the sum.
//
// cnt_i needs no device: one host rule over a prefix count of the live bins serves both routes.
#include <math.h>

#include <algorithm>
#include <new>
#include <string>
#include <vector>

#include "bb_cm_internal.h"
#include "bb_common.h"
#include "bb_triples.h"

// The product and the sum of a term are two roundings, as in numpy: no fma in this file.
#pragma clang fp contract(off)

namespace bb {

// The constants of the two kernels (tests/test_gpu_insulation.py names them).
constexpr int kInsBins = 64;      // bins of a workgroup of insulation_kernel: one per lane
constexpr int kInsRows = 16;      // rows of a step: 4 per wave
constexpr int kInsCols = 128;     // columns of a step: 2 loads of 64 doubles per row
constexpr int kInsWaveRows = 64;  // rows of a bin that triples_insulation_kernel adds per chunk

}  // namespace bb

namespace {

using bb::kInsBins;
using bb::kInsCols;
using bb::kInsRows;
using bb::kInsWaveRows;
using bb::lds_barrier;

// what a cell adds: its value times (x_a x_b) if both bins are live, else nothing
__device__ __forceinline__ double weighed(double v, double xa, double xb) {
    return (xa != 0.0 && xb != 0.0) ? v * (xa * xb) : 0.0;
}

__global__ __launch_bounds__(256) void insulation_kernel(const double *__restrict__ m, int64_t ld,
                                                         int64_t n, int64_t w, int64_t g,
                                                         const double *__restrict__ x,
                                                         double *__restrict__ sums) {
    __shared__ double tile[kInsRows * kInsCols];
    __shared__ double rp[kInsRows * kInsBins];        // the row partials of the step's rows
    constexpr int kPer = kInsRows / 4;                // rows of a step per wave, loading and adding
    constexpr int kLoads = kInsCols / 64;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t i0 = (int64_t)blockIdx.x * kInsBins, i1 = std::min<int64_t>(n, i0 + kInsBins);
    const int64_t ra = std::max<int64_t>(0, i0 - w + 1), rb = i1;           // rows [ra, rb)
    const int64_t ca = i0, cb = std::min<int64_t>(n, i1 - 1 + w);           // columns [ca, cb)
    const int64_t nrs = (rb - ra + kInsRows - 1) / kInsRows, ncs = (cb - ca + kInsCols - 1) / kInsCols;
    const int64_t steps = nrs * ncs;
    const int64_t i = i0 + lane;                      // this thread's bin
    const int64_t bin_hi = std::min<int64_t>(n - 1, i + w - 1);
    double v[kPer][kLoads];
    auto load = [&](int64_t s) {
        const int64_t rs = s / ncs, cs = s - rs * ncs;
#pragma unroll
        for (int rr = 0; rr < kPer; ++rr) {
            const int64_t row = ra + rs * kInsRows + kPer * wave + rr;
            const double xa = row < rb ? x[row] : 0.0;
#pragma unroll
            for (int q = 0; q < kLoads; ++q) {
                const int64_t col = ca + cs * kInsCols + lane + 64 * q;
                const bool ok = row < rb && col < cb && col >= row + g;     // (g >= 0: upper triangle)
                v[rr][q] = ok ? weighed(m[row * ld + col], xa, x[col]) : 0.0;
            }
        }
    };
    double part[kPer];      // the row partials of rows wave + 4 q of the step, for bin i
    double acc = 0.0;       // tid < kInsBins: sum_i so far
    load(0);
    for (int64_t s = 0; s < steps; ++s) {
        const int64_t rs = s / ncs, cs = s - rs * ncs;
        lds_barrier();      // (the last step's readers are done; LDS only: the loads stay in flight)
#pragma unroll
        for (int rr = 0; rr < kPer; ++rr)
#pragma unroll
            for (int q = 0; q < kLoads; ++q) tile[(kPer * wave + rr) * kInsCols + lane + 64 * q] = v[rr][q];
        if (s + 1 < steps) load(s + 1);
        lds_barrier();
        const int64_t c0 = ca + cs * kInsCols;
#pragma unroll
        for (int q = 0; q < kPer; ++q) {
            const int r = wave + 4 * q;
            const int64_t a = ra + rs * kInsRows + r;
            double p = cs == 0 ? 0.0 : part[q];
            if (i < i1 && a <= i && a + w > i) {                            // row a is in bin i's diamond
                // (where the row's cells of this chunk start and end; lo > hi: none here)
                const int lo = (int)std::min<int64_t>(std::max(std::max(i, a + g), c0) - c0, kInsCols);
                const int hi = (int)std::max<int64_t>(std::min(bin_hi, c0 + kInsCols - 1) - c0, -1);
                const double *cell = tile + r * kInsCols;
                for (int b = lo; b <= hi; ++b) p += cell[b];
            }
            part[q] = p;
        }
        if (cs != ncs - 1) continue;
#pragma unroll
        for (int q = 0; q < kPer; ++q) rp[(wave + 4 * q) * kInsBins + lane] = part[q];
        lds_barrier();
        // the rows' partials, top to bottom (a row outside the diamond left +0.0)
        if (tid < kInsBins)
            for (int r = 0; r < kInsRows; ++r) acc += rp[r * kInsBins + tid];
    }
    if (tid < kInsBins && i < i1) sums[i] = acc;
}

// the first entry of [b, e) whose column is >= key
__device__ __forceinline__ int64_t first_at_least(const int *__restrict__ col, int64_t b, int64_t e,
                                                  int64_t key) {
    while (b < e) {
        const int64_t mid = b + (e - b) / 2;
        if (col[mid] < key) b = mid + 1; else e = mid;
    }
    return b;
}

// the double lane k of the wave holds
__device__ __forceinline__ double lane_value(double v, int k) {
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)u, k);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(u >> 32), k);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

__global__ __launch_bounds__(256) void triples_insulation_kernel(const long long *__restrict__ ptr,
                                                                 const int *__restrict__ col,
                                                                 const double *__restrict__ val,
                                                                 int64_t n, int64_t w, int64_t g,
                                                                 const double *__restrict__ x,
                                                                 double *__restrict__ sums) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t i = (int64_t)blockIdx.x * 4 + wave;
    if (i >= n) return;                                   // (the whole wave)
    const int64_t a_lo = std::max<int64_t>(0, i - w + 1);
    const int64_t c_end = std::min<int64_t>(n, i + w);    // columns below this
    double acc = 0.0;                                     // the same in every lane
    for (int64_t a0 = a_lo; a0 <= i; a0 += kInsWaveRows) {
        const int64_t a = a0 + lane;
        double r = 0.0;
        if (a <= i) {
            const double xa = x[a];
            if (xa != 0.0) {
                const int64_t re = ptr[a + 1];
                for (int64_t e = first_at_least(col, ptr[a], re, std::max(i, a + g)); e < re; ++e) {
                    const int64_t c = col[e];
                    if (c >= c_end) break;
                    r += weighed(val[e], xa, x[c]);
                }
            }
        }
#pragma unroll
        for (int k = 0; k < kInsWaveRows; ++k) acc += lane_value(r, k);
    }
    if (lane == 0) sums[i] = acc;
}

// What both routes check, and what they prepare on the host: w and g clipped to the map (a window beyond n
// is n's, an offset beyond n leaves nothing), x = 1 / bias (0 where it is NaN; ones without a
// bias), and cnt_i from the prefix count L of the live bins: for each live row a of the diamond
// the live bins of [max(i, a + g), hi_i] -- the rows a <= i - g share the range [i, hi_i], the
// other min(g, ..) rows are taken one by one.
int check_args(const char *who, int64_t n, int64_t w, int64_t g, const double *sums, const int64_t *counts) {
    BB_REQUIRE(w >= 1, std::string(who) + ": window must be at least 1");
    BB_REQUIRE(g >= 0, std::string(who) + ": ignore_diags must not be negative");
    BB_REQUIRE(n == 0 || (sums != nullptr && counts != nullptr), std::string(who) + ": NULL argument");
    return BB_OK;
}

int prepare(const char *who, int64_t n, int64_t *w, int64_t *g, const double *bias, int64_t *counts,
            std::vector<double> *x) {
    *w = std::min(*w, std::max<int64_t>(n, 1));
    *g = std::min(*g, n);
    std::vector<int64_t> L;
    try {
        x->resize((size_t)n);
        L.resize((size_t)n + 1);
    } catch (const std::bad_alloc &) {
        return bb::fail(BB_ERR_NOMEM, std::string(who) + ": out of host memory");
    }
    L[0] = 0;
    for (int64_t i = 0; i < n; ++i) {
        const double b = bias ? bias[i] : 1.0;
        (*x)[i] = bias ? (b != b ? 0.0 : 1.0 / b) : 1.0;
        L[i + 1] = L[i] + ((*x)[i] != 0.0 ? 1 : 0);
    }
    for (int64_t i = 0; i < n; ++i) {
        const int64_t lo = std::max<int64_t>(0, i - *w + 1), hi = std::min(n - 1, i + *w - 1);
        const int64_t shared_to = i - *g;                 // rows lo .. shared_to read [i, hi]
        int64_t c = 0;
        if (shared_to >= lo) c = (L[shared_to + 1] - L[lo]) * (L[hi + 1] - L[i]);
        for (int64_t a = std::max(lo, shared_to + 1); a <= i; ++a)
            if ((*x)[a] != 0.0 && a + *g <= hi) c += L[hi + 1] - L[a + *g];
        counts[i] = c;
    }
    return BB_OK;
}

// x to the device, the kernel `enqueue` launches between two marks of the clock, sums back.
template <typename Enqueue>
int run(const char *who, int64_t n, const std::vector<double> &x, double *sums, double *kernel_ms,
        hipStream_t st, Enqueue enqueue) {
    bb::DevBuf bx, bs;
    hipError_t e = bx.alloc((size_t)n * 8);
    if (e == hipSuccess) e = bs.alloc((size_t)n * 8);
    BB_TRY(bb::hip_status(who, e, BB_ERR_NOMEM));
    bb::StageClock<2> clock;
    e = clock.start();
    if (e == hipSuccess) e = hipMemcpyAsync(bx.p, x.data(), (size_t)n * 8, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = clock.mark(0, st);
    if (e == hipSuccess) e = enqueue((const double *)bx.p, bs.as<double>());
    if (e == hipSuccess) e = clock.mark(1, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e == hipSuccess) e = clock.read(0, kernel_ms);
    if (e == hipSuccess) e = hipMemcpy(sums, bs.p, (size_t)n * 8, hipMemcpyDeviceToHost);
    return bb::hip_status(who, e);
}

}  // namespace

extern "C" {

int bb_cm_insulation(bb_cm *cm, int64_t n_bins, int64_t window, int64_t ignore_diags, const double *bias,
                     double *sums, int64_t *counts) {
    const char *who = "bb_cm_insulation";
    BB_TRY(bb::cm_check(cm, who));
    BB_TRY(bb::cm_check_bins(cm, n_bins, who));
    const int64_t n = n_bins;
    int64_t w = window, g = ignore_diags;
    std::vector<double> x;
    BB_TRY(check_args(who, n, w, g, sums, counts));
    BB_TRY(prepare(who, n, &w, &g, bias, counts, &x));
    cm->insulation_ms = 0.0;
    if (n == 0) return BB_OK;
    hipStream_t st = cm->stream;
    return run(who, n, x, sums, &cm->insulation_ms, st, [&](const double *dx, double *dsums) {
        return bb::launch(insulation_kernel, dim3((unsigned)((n + kInsBins - 1) / kInsBins)), dim3(256), 0, st,
                          (const double *)cm->m, cm->d, n, w, g, dx, dsums);
    });
}

int bb_cm_insulation_timing(const bb_cm *cm, double *kernel_ms) {
    BB_REQUIRE(cm != nullptr && kernel_ms != nullptr, "bb_cm_insulation_timing: NULL argument");
    *kernel_ms = cm->insulation_ms;
    return BB_OK;
}

int bb_triples_insulation(bb_triples *t, int64_t n_bins, int64_t window, int64_t ignore_diags,
                          const double *bias, double *sums, int64_t *counts) {
    const char *who = "bb_triples_insulation";
    BB_REQUIRE(t != nullptr, std::string(who) + ": triples is NULL");
    BB_REQUIRE(n_bins >= 0, std::string(who) + ": n_bins must not be negative");
    const int64_t n = n_bins;
    int64_t w = window, g = ignore_diags;
    std::vector<double> x;
    BB_TRY(check_args(who, n, w, g, sums, counts));
    BB_TRY(bb::triples_ensure_index(t, n_bins, who));
    BB_TRY(prepare(who, n, &w, &g, bias, counts, &x));
    t->insulation_ms = 0.0;
    if (n == 0) return BB_OK;
    const bb::SegmentedList &rows = t->index.rows;
    hipStream_t st = nullptr;
    return run(who, n, x, sums, &t->insulation_ms, st, [&](const double *dx, double *dsums) {
        return bb::launch(triples_insulation_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st,
                          (const long long *)rows.ptr.p, (const int *)rows.other.p,
                          (const double *)rows.val.p, n, w, g, dx, dsums);
    });
}

int bb_triples_insulation_timing(const bb_triples *t, double *kernel_ms) {
    BB_REQUIRE(t != nullptr && kernel_ms != nullptr, "bb_triples_insulation_timing: NULL argument");
    *kernel_ms = t->insulation_ms;
    return BB_OK;
}

}  // extern "C"
