// bb_significance.hip -- the Fit-Hi-C significance call on a resident map (docs/SPEC.md 2.9): the
// in-range stored cells of the upper triangle as a list in canonical order (row-major, i <= j) and
// the binomial survival function p = P(Binomial(N, pi) >= count) of every listed cell, pi =
// f[j - i] b_i b_j.  (Reference: blueberry/fithic.py:413-435, one text line at a time through
// scipy.special.bdtrc.)
//
//   bb::binomial_sf  the one copy of the rule, float64: Loader's saddle-point pmf (stirlerr + bd0:
//               no difference of two huge lgamma values) at the starting term, then the ratio
//               recurrence of neighbouring pmf values -- upward from k when k lies above the mode,
//               else downward from k - 1 and 1 - sum -- until a term no longer changes the sum.
//               The number of terms grows like sqrt(N p): 8.5 sqrt(N p) + 64 bounds every case the
//               float64 model has seen (tests/_fithic_model.py counts them), so for N p <=
//               kSfMaxMean = 2^20 fewer than 8,768 are needed and the loop's compile-time cap
//               kSfMaxTerms = 16,384 is never reached; the entry points refuse a larger N p, and a
//               lane that reaches the cap all the same raises a flag that turns the call into an
//               error.  No array, no scratch.
//   the list    a WORK ITEM is one wave's share of one row: up to kSigSeg = 1024 columns of the
//               row's in-range span (dense), or one segment of the row's entries in the triples'
//               canonical index (bb_triples.h).  Pass 1 counts the listed cells of every item (wave
//               ballots), an exclusive scan of the counts in item order gives every item its place,
//               pass 2 forms the same predicates again and writes row, col and count there: a
//               cell's place is a function of the map alone -- no atomic cursor -- and the matrix
//               is read twice.  Pass 1 also counts what makes the call an error: counted cells that
//               are not raw counts, and listed cells whose N pi is above kSfMaxMean.
//   sig_p_kernel  one lane per LISTED cell, so that no lane idles on an empty one; neighbouring
//               lanes are neighbouring columns of a row and carry similar priors, hence similar
//               term counts.  Both routes end in this kernel.
//   q-values    of the resident p-values, kept on the handle (bb_sig_q_values): the rule of SPEC
//               2.9.7 through bb::q_values_device (bb_qvalues.h: key, stable sort, BH scan,
//               scatter).  bb_sig_select makes the list of the cells with q <= q_max as the list
//               itself is made: a flag per cell, an exclusive scan, a write -- list order stays.
// Integer atomics only (counters whose sum does not depend on the order); the same bits on
// every run and on both routes.
#include <float.h>
#include <math.h>

#include <memory>
#include <string>

#include "bb_cm_internal.h"
#include "bb_common.h"
#include "bb_qvalues.h"
#include "bb_sort.h"
#include "bb_triples.h"

namespace bb {

constexpr double kSfMaxMean = 1048576.0;   // the largest N p the term cap was derived for
constexpr int kSfMaxTerms = 16384;         // > 8.5 sqrt(kSfMaxMean) + 64 = 8,768

// stirlerr(n) = log n! - log(sqrt(2 pi n) (n / e)^n) for n = 0 .. 15
__device__ const double kStirlerr[16] = {
    0.0,
    0.08106146679532725821967026,  0.04134069595540929409382208,  0.02767792568499833914878929,
    0.02079067210376509311152277,  0.01664469118982119216319487,  0.01387612882307074799874573,
    0.01189670994589177009505572,  0.01041126526197209649747857,  0.009255462182712732917728637,
    0.008330563433362871256469319, 0.007573675487951840794972024, 0.006942840107209529865664153,
    0.006408994188004207068439631, 0.005951370112758847735624416, 0.00555473355196280137103869};

// n: a whole number >= 0.  Above the table the series in 1 / n^2; its first dropped term is
// below 1.1e-16 at n = 16.
__device__ __forceinline__ double sf_stirlerr(double n) {
    if (n <= 15.0) return kStirlerr[(int)n];
    const double nn = n * n;
    return (1.0 / 12.0 - (1.0 / 360.0 - (1.0 / 1260.0 - (1.0 / 1680.0 - (1.0 / 1188.0) / nn) / nn) / nn) / nn) / n;
}

// bd0(x, np) = x log(x / np) + np - x, by its series in (x - np) / (x + np) where the three
// terms would cancel (Loader 2000)
__device__ __forceinline__ double sf_bd0(double x, double np) {
    if (fabs(x - np) < 0.1 * (x + np)) {
        double v = (x - np) / (x + np);
        double s = (x - np) * v;
        double ej = 2.0 * x * v;
        v *= v;
#pragma unroll
        for (int j = 1; j <= 10; ++j) {       // v < 0.01: the 10th term is below 1e-19 of the sum
            ej *= v;
            s += ej / (double)(2 * j + 1);
        }
        return s;
    }
    return x * log(x / np) + np - x;
}

// P(X = x), X ~ Binomial(n, p), for whole 0 < x <= n and 0 < p < 1, q = 1 - p
__device__ __forceinline__ double sf_pmf(double x, double n, double p, double q) {
    if (x == n) return exp(q < 0.1 ? -sf_bd0(n, n * p) - n * q : n * log(p));
    const double lc = sf_stirlerr(n) - sf_stirlerr(x) - sf_stirlerr(n - x) - sf_bd0(x, n * p) -
                      sf_bd0(n - x, n * q);
    const double lf = 1.8378770664093454835606594728112 + log(x) + log1p(-x / n);   // log(2 pi) + ..
    return exp(lc - 0.5 * lf);
}

// P(X >= k), X ~ Binomial(n, p); n a whole number >= 0.  NaN for p outside [0, 1].  *terms: pmf
// values summed (0 in a closed case); *capped is set if the loop ran into kSfMaxTerms.
__device__ __forceinline__ double binomial_sf(long long k, double n, double p, int *terms, int *capped) {
    *terms = 0;
    if (!(p >= 0.0 && p <= 1.0)) return (double)NAN;
    if (k <= 0) return 1.0;
    const double x = (double)k;
    if (x > n) return 0.0;
    if (p == 0.0) return 0.0;
    if (p == 1.0) return 1.0;
    if (k == 1) return -expm1(n * log1p(-p));
    const double q = 1.0 - p;
    const bool up = x > (n + 1.0) * p;             // k above the mode: the terms fall from k on
    const double r = up ? p / q : q / p;
    double j = up ? x : x - 1.0;
    double term = sf_pmf(j, n, p, q), sum = term;
    int t = 1;
    for (; t < kSfMaxTerms; ++t) {
        // the next pmf over this one; 0 at j = n (upward) and j = 0 (downward), which ends the loop
        term *= up ? (n - j) / (j + 1.0) * r : j / (n - j + 1.0) * r;
        j += up ? 1.0 : -1.0;
        const double s1 = sum + term;
        if (s1 == sum) break;
        sum = s1;
    }
    *terms = t;
    if (t >= kSfMaxTerms) *capped = 1;
    return up ? sum : 1.0 - sum;
}

// pi_ij, formed in this one order wherever it is needed
__device__ __forceinline__ double sig_prior(double f, double bi, double bj) { return f * bi * bj; }

}  // namespace bb

// The results of one significance call: the list in canonical order, resident.
struct bb_sig {
    int device = 0;
    int64_t n = 0;                   // listed cells
    int64_t terms = 0;               // pmf values summed over all of them
    double list_ms = 0.0, p_ms = 0.0;
    bb::DevBuf row, col, count, p;   // int32, int32, float64, float64
    bb::DevBuf q;                    // float64, once bb_sig_q_values has run (have_q)
    bool have_q = false;
};

namespace {

typedef unsigned long long u64;

constexpr int kSigSeg = 1024;        // columns of one row that one wave lists (dense route)
constexpr int kSfBlock = 256;        // workgroup of every kernel here: 4 waves

struct SigStatus {
    u64 listed;     // the list's length (written by sig_total_kernel)
    u64 bad;        // counted cells that are negative, not finite or not whole
    u64 over;       // listed cells with N pi > kSfMaxMean
    u64 terms;      // pmf values summed
    int capped;     // a lane ran into kSfMaxTerms
    int pad[3];     // (48 bytes: the record is cleared by a memset of a multiple of 16)
};
static_assert(sizeof(SigStatus) % 16 == 0, "SigStatus is cleared in 16-byte words");

struct SigArgs {
    int64_t n, k_lo, k_hi;
    const double *bias, *f;
    double lo, hi, n_total;
};

// What a cell (i, j) with value a is: bit 0 = not a raw count, bit 1 = listed, bit 2 = listed
// and above the limit of N pi.  bi_ok: b_i lies inside the bias bounds.
__device__ __forceinline__ int sig_classify(double a, bool bi_ok, double bi, double bj, double fk,
                                            const SigArgs &g) {
    if (!(a >= 0.0 && a <= DBL_MAX && a == floor(a))) return 1;
    const double pi = bb::sig_prior(fk, bi, bj);
    const bool listed = a >= 1.0 && bi_ok && bj >= g.lo && bj <= g.hi && pi >= 0.0 && pi <= 1.0;
    if (!listed) return 0;
    return (pi < 1.0 && g.n_total * pi > bb::kSfMaxMean) ? 6 : 2;
}

// One wave's walk over its work item, 64 cells at a time in list order: `cell(e, j, a)` gives, for
// position e of [begin, end), whether it is a counted cell, its column and its value.
template <bool WRITE, typename Cell>
__device__ __forceinline__ void sig_item(int64_t w, int64_t i, int64_t begin, int64_t end, const SigArgs &g,
                                         Cell cell, u64 *__restrict__ counts,
                                         const u64 *__restrict__ offset, int *__restrict__ row,
                                         int *__restrict__ col, double *__restrict__ cnt,
                                         SigStatus *__restrict__ status) {
    const int lane = threadIdx.x & 63;
    const double bi = g.bias[i];
    const bool bi_ok = bi >= g.lo && bi <= g.hi;
    u64 base = WRITE ? offset[w] : 0;
    unsigned listed = 0, bad = 0, over = 0;
    for (int64_t e0 = begin; e0 < end; e0 += 64) {
        const int64_t e = e0 + lane;
        int64_t j = 0;
        double a = 0.0;
        const bool in = e < end && cell(e, j, a);
        const int what = in ? sig_classify(a, bi_ok, bi, g.bias[j], g.f[j - i], g) : 0;
        const u64 votes = __ballot((what & 2) != 0);
        if (WRITE) {
            if (what & 2) {
                const u64 pos = base + (u64)__popcll(votes & (((u64)1 << lane) - 1));
                row[pos] = (int)i;
                col[pos] = (int)j;
                cnt[pos] = a;
            }
            base += (u64)__popcll(votes);
        } else {
            listed += (unsigned)__popcll(votes);
            bad += (unsigned)__popcll(__ballot((what & 1) != 0));
            over += (unsigned)__popcll(__ballot((what & 4) != 0));
        }
    }
    if (!WRITE && lane == 0) {
        counts[w] = listed;
        if (bad) atomicAdd(&status->bad, (u64)bad);
        if (over) atomicAdd(&status->over, (u64)over);
    }
}

// Dense route.  Item w = (row i, segment s) = w / nseg, w % nseg: the columns i + k_lo + s kSigSeg
// .. of row i that are in range and below n.  Rows whose span is shorter have empty items.
template <bool WRITE>
__global__ __launch_bounds__(kSfBlock) void sig_dense_kernel(const double *__restrict__ m, int64_t ld,
                                                            int64_t nseg, SigArgs g,
                                                            u64 *__restrict__ counts,
                                                            const u64 *__restrict__ offset,
                                                            int *__restrict__ row, int *__restrict__ col,
                                                            double *__restrict__ cnt,
                                                            SigStatus *__restrict__ status) {
    const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= g.n * nseg) return;                  // (whole waves: no barrier follows)
    const int64_t i = w / nseg, s = w - i * nseg;
    const int64_t begin = i + g.k_lo + s * kSigSeg;
    const int64_t end = std::min(std::min<int64_t>(g.n, i + g.k_hi + 1), begin + kSigSeg);
    const double *__restrict__ mrow = m + i * ld;
    sig_item<WRITE>(w, i, begin, end, g,
                    [&](int64_t e, int64_t &j, double &a) {
                        j = e;
                        a = mrow[e];
                        return true;
                    },
                    counts, offset, row, col, cnt, status);
}

// Triples route.  Item w = segment w of the canonical index's rows; its upper entries in range.
template <bool WRITE>
__global__ __launch_bounds__(kSfBlock) void sig_triples_kernel(
    const long long *__restrict__ ptr, const int *__restrict__ other, const double *__restrict__ val,
    const long long *__restrict__ seg_ptr, const int *__restrict__ seg_owner, int64_t n_seg, SigArgs g,
    u64 *__restrict__ counts, const u64 *__restrict__ offset, int *__restrict__ row,
    int *__restrict__ col, double *__restrict__ cnt, SigStatus *__restrict__ status) {
    const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= n_seg) return;                       // (whole waves: no barrier follows)
    const int64_t i = seg_owner[w];
    const int64_t begin = ptr[i] + (w - seg_ptr[i]) * bb::kTbSeg;
    const int64_t end = std::min<int64_t>(ptr[i + 1], begin + bb::kTbSeg);
    sig_item<WRITE>(w, i, begin, end, g,
                    [&](int64_t e, int64_t &j, double &a) {
                        j = other[e];
                        a = val[e];
                        return j >= i + g.k_lo && j <= i + g.k_hi;
                    },
                    counts, offset, row, col, cnt, status);
}

__global__ void sig_total_kernel(const u64 *__restrict__ counts, const u64 *__restrict__ offset,
                                 int64_t items, SigStatus *__restrict__ status) {
    status->listed = items > 0 ? offset[items - 1] + counts[items - 1] : 0;
}

// terms of the wave's lanes into the status, one integer atomic per wave
__device__ __forceinline__ void sf_account(int terms, int capped, SigStatus *__restrict__ status) {
    const u64 t = bb::wave_sum_first((u64)terms);
    if ((threadIdx.x & 63) == 0 && t != 0) atomicAdd(&status->terms, t);
    if (capped) status->capped = 1;
}

// a count as the k of binomial_sf (a count beyond the int64 range is beyond every N)
__device__ __forceinline__ long long sig_k(double count) {
    return count >= 9.2e18 ? 9223372036854775807LL : (long long)count;
}

__global__ __launch_bounds__(kSfBlock) void sig_p_kernel(const int *__restrict__ row,
                                                        const int *__restrict__ col,
                                                        const double *__restrict__ cnt, int64_t m,
                                                        const double *__restrict__ bias,
                                                        const double *__restrict__ f, double n_total,
                                                        double *__restrict__ p,
                                                        SigStatus *__restrict__ status) {
    const int64_t e = (int64_t)blockIdx.x * kSfBlock + threadIdx.x;
    int terms = 0, capped = 0;
    if (e < m) {
        const int i = row[e], j = col[e];
        p[e] = bb::binomial_sf(sig_k(cnt[e]), n_total, bb::sig_prior(f[j - i], bias[i], bias[j]), &terms,
                               &capped);
    }
    sf_account(terms, capped, status);
}

__global__ __launch_bounds__(kSfBlock) void binomial_sf_kernel(const long long *__restrict__ k, double n,
                                                              const double *__restrict__ p, int64_t m,
                                                              double *__restrict__ out,
                                                              SigStatus *__restrict__ status) {
    const int64_t e = (int64_t)blockIdx.x * kSfBlock + threadIdx.x;
    int terms = 0, capped = 0;
    if (e < m) out[e] = bb::binomial_sf(k[e], n, p[e], &terms, &capped);
    sf_account(terms, capped, status);
}

// ---- the selection: the cells with q <= q_max, as the list itself is made -------------------------
// keep[e] = 1 for a cell with q <= q_max (a NaN q fails the comparison: never selected)
__global__ __launch_bounds__(kSfBlock) void sig_keep_kernel(const double *__restrict__ q, int64_t m,
                                                           double q_max, u64 *__restrict__ keep) {
    const int64_t e = (int64_t)blockIdx.x * kSfBlock + threadIdx.x;
    if (e < m) keep[e] = q[e] <= q_max ? 1 : 0;
}

// the kept cells to their places pos[e] (the exclusive scan of keep): list order stays
__global__ __launch_bounds__(kSfBlock) void sig_pick_kernel(
    const u64 *__restrict__ keep, const u64 *__restrict__ pos, int64_t m, const int *__restrict__ row,
    const int *__restrict__ col, const double *__restrict__ cnt, const double *__restrict__ p,
    const double *__restrict__ q, int *__restrict__ orow, int *__restrict__ ocol, double *__restrict__ ocnt,
    double *__restrict__ op, double *__restrict__ oq) {
    const int64_t e = (int64_t)blockIdx.x * kSfBlock + threadIdx.x;
    if (e >= m || keep[e] == 0) return;
    const u64 at = pos[e];
    orow[at] = row[e];
    ocol[at] = col[e];
    ocnt[at] = cnt[e];
    op[at] = p[e];
    oq[at] = q[e];
}

// ---- host side ---------------------------------------------------------------------------------
inline bool whole_count(double v) { return v >= 0.0 && v <= 9007199254740992.0 && v == floor(v); }

inline dim3 wave_grid(int64_t waves) { return dim3((unsigned)((waves + 3) / 4)); }

// The call behind both routes.  `items` work items; pass(write, counts, offset, row, col, cnt,
// status) launches the route's kernel on `st`.  The work buffer holds bias | f | status | counts |
// offsets | the scan's temporary storage; it and the results are all the call allocates.
template <typename Pass>
int significance_run(const std::string &who, int device, hipStream_t st, int64_t items, SigArgs g,
                     const double *bias, const double *prior, Pass pass, bb_sig **out) {
    const int64_t n = g.n;
    const size_t vec = bb::align256((size_t)n * 8), cells = bb::align256((size_t)std::max<int64_t>(items, 1) * 8);
    size_t scan_bytes = 0;
    hipError_t e = hipSuccess;
    if (items > 0) e = bb::exclusive_scan_bytes((size_t)items, &scan_bytes);
    BB_TRY(bb::hip_status(who.c_str(), e));
    bb::DevBuf work;
    BB_TRY(bb::hip_status(who.c_str(), work.alloc(2 * vec + 256 + 2 * cells + scan_bytes), BB_ERR_NOMEM));
    char *base = (char *)work.p;
    double *dbias = (double *)base, *df = (double *)(base + vec);
    SigStatus *status = (SigStatus *)(base + 2 * vec);
    u64 *counts = (u64 *)(base + 2 * vec + 256), *offset = (u64 *)(base + 2 * vec + 256 + cells);
    void *scan_tmp = base + 2 * vec + 256 + 2 * cells;
    g.bias = dbias;
    g.f = df;
    bb::StageClock<3> clock;                      // the list | its p-values
    e = clock.start();
    if (e == hipSuccess) e = hipMemcpyAsync(dbias, bias, (size_t)n * 8, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(df, prior, (size_t)n * 8, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemsetAsync(status, 0, sizeof(SigStatus), st);
    if (e == hipSuccess) e = clock.mark(0, st);
    if (e == hipSuccess && items > 0) e = pass(false, g, counts, offset, nullptr, nullptr, nullptr, status);
    if (e == hipSuccess && items > 0)
        e = bb::exclusive_scan(scan_tmp, scan_bytes, counts, offset, (size_t)items, st);
    if (e == hipSuccess)
        e = bb::launch(sig_total_kernel, dim3(1), dim3(1), 0, st, (const u64 *)counts, (const u64 *)offset,
                       items, status);
    SigStatus hs;
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e == hipSuccess) e = hipMemcpy(&hs, status, sizeof(hs), hipMemcpyDeviceToHost);
    BB_TRY(bb::hip_status(who.c_str(), e));
    if (hs.bad != 0)
        return bb::fail(BB_ERR_INVALID, who + ": significance needs raw counts: " +
                                            std::to_string(hs.bad) +
                                            " counted cells are negative, not finite or not whole numbers");
    if (hs.over != 0)
        return bb::fail(BB_ERR_INVALID,
                        who + ": " + std::to_string(hs.over) +
                            " listed cells have an expected count N * prior above 1048576, the limit "
                            "the binomial tail sum is built for");
    std::unique_ptr<bb_sig> sig(new bb_sig());
    sig->device = device;
    sig->n = (int64_t)hs.listed;
    const size_t m = (size_t)sig->n;
    e = sig->row.alloc(m * 4);
    if (e == hipSuccess) e = sig->col.alloc(m * 4);
    if (e == hipSuccess) e = sig->count.alloc(m * 8);
    if (e == hipSuccess) e = sig->p.alloc(m * 8);
    BB_TRY(bb::hip_status(who.c_str(), e, BB_ERR_NOMEM));
    if (items > 0 && m > 0)
        e = pass(true, g, counts, offset, sig->row.as<int>(), sig->col.as<int>(), sig->count.as<double>(), status);
    if (e == hipSuccess) e = clock.mark(1, st);
    if (e == hipSuccess && m > 0)
        e = bb::launch(sig_p_kernel, dim3((unsigned)((m + kSfBlock - 1) / kSfBlock)), dim3(kSfBlock), 0, st,
                       (const int *)sig->row.p, (const int *)sig->col.p, (const double *)sig->count.p,
                       (int64_t)m, (const double *)dbias, (const double *)df, g.n_total, sig->p.as<double>(),
                       status);
    if (e == hipSuccess) e = clock.mark(2, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e == hipSuccess) e = hipMemcpy(&hs, status, sizeof(hs), hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = clock.read(0, &sig->list_ms);
    if (e == hipSuccess) e = clock.read(1, &sig->p_ms);
    BB_TRY(bb::hip_status(who.c_str(), e));
    if (hs.capped != 0)
        return bb::fail(BB_ERR_STATE, who + ": a binomial tail sum ran into its cap of terms; no result");
    sig->terms = (int64_t)hs.terms;
    *out = sig.release();
    return BB_OK;
}

int significance_check_args(const std::string &who, int64_t n_bins, int64_t k_lo, int64_t k_hi,
                            const double *bias, double bias_lo, double bias_hi, const double *prior,
                            double n_total, bb_sig **out) {
    BB_REQUIRE(out != nullptr && bias != nullptr && prior != nullptr, who + ": NULL argument");
    *out = nullptr;
    BB_REQUIRE(n_bins >= 1 && n_bins < 2147483647, who + ": n_bins is out of range");
    BB_REQUIRE(k_lo >= 0 && k_lo <= k_hi && k_hi < n_bins,
               who + ": the range of diagonals must satisfy 0 <= k_lo <= k_hi < n_bins");
    BB_REQUIRE(bias_lo <= bias_hi, who + ": the bias bounds are not ordered");
    BB_REQUIRE(whole_count(n_total), who + ": n_total must be a whole number in [0, 2^53]");
    return BB_OK;
}

}  // namespace

extern "C" {

int bb_binomial_sf(const int64_t *k, double n, const double *p, double *out, int64_t m, int device) {
    BB_REQUIRE(m >= 0, "bb_binomial_sf: negative length");
    BB_REQUIRE(whole_count(n), "bb_binomial_sf: n must be a whole number in [0, 2^53]");
    if (m == 0) return BB_OK;
    BB_REQUIRE(k != nullptr && p != nullptr && out != nullptr, "bb_binomial_sf: NULL argument");
    for (int64_t i = 0; i < m; ++i)
        if (p[i] > 0.0 && p[i] < 1.0 && n * p[i] > bb::kSfMaxMean)
            return bb::fail(BB_ERR_INVALID,
                            "bb_binomial_sf: n * p is above 1048576, the limit the tail sum is built "
                            "for (element " + std::to_string((long long)i) + ")");
    BB_TRY(bb::use_device(device));
    const size_t vec = bb::align256((size_t)m * 8);
    bb::DevBuf work;
    BB_TRY(bb::hip_status("bb_binomial_sf", work.alloc(3 * vec + 256), BB_ERR_NOMEM));
    char *base = (char *)work.p;
    SigStatus *status = (SigStatus *)(base + 3 * vec);
    hipStream_t st = nullptr;
    hipError_t e = hipMemcpyAsync(base, k, (size_t)m * 8, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(base + vec, p, (size_t)m * 8, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemsetAsync(status, 0, sizeof(SigStatus), st);
    if (e == hipSuccess)
        e = bb::launch(binomial_sf_kernel, dim3((unsigned)((m + kSfBlock - 1) / kSfBlock)), dim3(kSfBlock), 0,
                       st, (const long long *)base, n, (const double *)(base + vec), m,
                       (double *)(base + 2 * vec), status);
    SigStatus hs;
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e == hipSuccess) e = hipMemcpy(&hs, status, sizeof(hs), hipMemcpyDeviceToHost);
    BB_TRY(bb::hip_status("bb_binomial_sf", e));
    if (hs.capped != 0)
        return bb::fail(BB_ERR_STATE, "bb_binomial_sf: a tail sum ran into its cap of terms; no result");
    return bb::hip_status("bb_binomial_sf",
                          hipMemcpy(out, base + 2 * vec, (size_t)m * 8, hipMemcpyDeviceToHost));
}

int bb_cm_significance(bb_cm *cm, int64_t n_bins, int64_t k_lo, int64_t k_hi, const double *bias,
                       double bias_lo, double bias_hi, const double *prior_by_distance, double n_total,
                       bb_sig **out) {
    const std::string who = "bb_cm_significance";
    BB_TRY(significance_check_args(who, n_bins, k_lo, k_hi, bias, bias_lo, bias_hi, prior_by_distance,
                                   n_total, out));
    BB_TRY(bb::cm_check(cm, who.c_str()));
    BB_TRY(bb::cm_check_bins(cm, n_bins, who.c_str()));
    const int64_t n = n_bins;
    // the longest in-range span of a row is row 0's
    const int64_t span = std::min(n - 1, k_hi) - k_lo + 1, nseg = (span + kSigSeg - 1) / kSigSeg;
    SigArgs g{n, k_lo, k_hi, nullptr, nullptr, bias_lo, bias_hi, n_total};
    hipStream_t st = cm->stream;
    const double *m = cm->m;
    const int64_t ld = cm->d;
    return significance_run(
        who, cm->device, st, n * nseg, g, bias, prior_by_distance,
        [&](bool write, const SigArgs &a, u64 *counts, const u64 *offset, int *row, int *col, double *cnt,
            SigStatus *status) {
            return write ? bb::launch(sig_dense_kernel<true>, wave_grid(n * nseg), dim3(kSfBlock), 0, st, m,
                                      ld, nseg, a, counts, offset, row, col, cnt, status)
                         : bb::launch(sig_dense_kernel<false>, wave_grid(n * nseg), dim3(kSfBlock), 0, st, m,
                                      ld, nseg, a, counts, offset, row, col, cnt, status);
        },
        out);
}

int bb_triples_significance(bb_triples *t, int64_t n_bins, int64_t k_lo, int64_t k_hi, const double *bias,
                            double bias_lo, double bias_hi, const double *prior_by_distance,
                            double n_total, bb_sig **out) {
    const std::string who = "bb_triples_significance";
    BB_TRY(significance_check_args(who, n_bins, k_lo, k_hi, bias, bias_lo, bias_hi, prior_by_distance,
                                   n_total, out));
    BB_TRY(bb::triples_ensure_index(t, n_bins, who.c_str()));
    const bb::SegmentedList &rows = t->index.rows;
    SigArgs g{n_bins, k_lo, k_hi, nullptr, nullptr, bias_lo, bias_hi, n_total};
    hipStream_t st = nullptr;
    const int64_t n_seg = rows.n_seg;
    return significance_run(
        who, t->device, st, n_seg, g, bias, prior_by_distance,
        [&](bool write, const SigArgs &a, u64 *counts, const u64 *offset, int *row, int *col, double *cnt,
            SigStatus *status) {
            const long long *ptr = (const long long *)rows.ptr.p, *seg_ptr = (const long long *)rows.seg_ptr.p;
            const int *other = (const int *)rows.other.p, *seg_owner = (const int *)rows.seg_owner.p;
            const double *val = (const double *)rows.val.p;
            return write ? bb::launch(sig_triples_kernel<true>, wave_grid(n_seg), dim3(kSfBlock), 0, st, ptr,
                                      other, val, seg_ptr, seg_owner, n_seg, a, counts, offset, row, col, cnt,
                                      status)
                         : bb::launch(sig_triples_kernel<false>, wave_grid(n_seg), dim3(kSfBlock), 0, st, ptr,
                                      other, val, seg_ptr, seg_owner, n_seg, a, counts, offset, row, col, cnt,
                                      status);
        },
        out);
}

int bb_sig_size(const bb_sig *s, int64_t *n_listed, int64_t *terms) {
    BB_REQUIRE(s != nullptr && n_listed != nullptr, "bb_sig_size: NULL argument");
    *n_listed = s->n;
    if (terms) *terms = s->terms;
    return BB_OK;
}

int bb_sig_timing(const bb_sig *s, double *list_ms, double *p_ms) {
    BB_REQUIRE(s != nullptr, "bb_sig_timing: results are NULL");
    if (list_ms) *list_ms = s->list_ms;
    if (p_ms) *p_ms = s->p_ms;
    return BB_OK;
}

int bb_sig_read(const bb_sig *s, int32_t *row, int32_t *col, double *count, double *p) {
    BB_REQUIRE(s != nullptr, "bb_sig_read: results are NULL");
    if (s->n == 0) return BB_OK;
    BB_REQUIRE(row != nullptr && col != nullptr && count != nullptr && p != nullptr,
               "bb_sig_read: NULL argument");
    BB_TRY(bb::enter_device(s->device));
    const size_t m = (size_t)s->n;
    hipError_t e = hipMemcpy(row, s->row.p, m * 4, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(col, s->col.p, m * 4, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(count, s->count.p, m * 8, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(p, s->p.p, m * 8, hipMemcpyDeviceToHost);
    return bb::hip_status("bb_sig_read", e);
}

int bb_sig_q_values(bb_sig *s, int64_t n_tests, double *sort_ms, double *scan_ms) {
    BB_REQUIRE(s != nullptr, "bb_sig_q_values: results are NULL");
    BB_REQUIRE(n_tests >= 0, "bb_sig_q_values: negative n_tests");
    BB_TRY(bb::enter_device(s->device));
    s->have_q = false;                            // (a call that fails leaves the handle without q)
    s->q.reset();
    bb::DevBuf q;
    BB_TRY(bb::hip_status("bb_sig_q_values", q.alloc((size_t)s->n * 8), BB_ERR_NOMEM));
    BB_TRY(bb::q_values_device("bb_sig_q_values", (const double *)s->p.p, s->n, n_tests, q.as<double>(),
                               nullptr, (hipStream_t) nullptr, sort_ms, scan_ms));
    s->q = std::move(q);
    s->have_q = true;
    return BB_OK;
}

int bb_sig_read_q(const bb_sig *s, double *q) {
    BB_REQUIRE(s != nullptr, "bb_sig_read_q: results are NULL");
    if (!s->have_q) return bb::fail(BB_ERR_STATE, "bb_sig_read_q: no q-values yet (bb_sig_q_values)");
    if (s->n == 0) return BB_OK;
    BB_REQUIRE(q != nullptr, "bb_sig_read_q: NULL argument");
    BB_TRY(bb::enter_device(s->device));
    return bb::hip_status("bb_sig_read_q", hipMemcpy(q, s->q.p, (size_t)s->n * 8, hipMemcpyDeviceToHost));
}

int bb_sig_select(const bb_sig *s, double q_max, bb_sig **out) {
    const char *who = "bb_sig_select";
    BB_REQUIRE(out != nullptr, "bb_sig_select: NULL argument");
    *out = nullptr;
    BB_REQUIRE(s != nullptr, "bb_sig_select: results are NULL");
    BB_REQUIRE(q_max == q_max, "bb_sig_select: q_max is NaN");
    if (!s->have_q) return bb::fail(BB_ERR_STATE, "bb_sig_select: no q-values yet (bb_sig_q_values)");
    BB_TRY(bb::enter_device(s->device));
    hipStream_t st = nullptr;
    const int64_t m = s->n;
    std::unique_ptr<bb_sig> sel(new bb_sig());
    sel->device = s->device;
    sel->have_q = true;
    bb::DevBuf work;
    u64 *keep = nullptr, *pos = nullptr;
    hipError_t e = hipSuccess;
    if (m > 0) {
        // keep | pos | the scan's temporary storage
        const size_t cells = bb::align256((size_t)m * 8);
        size_t scan_bytes = 0;
        e = bb::exclusive_scan_bytes((size_t)m, &scan_bytes);
        BB_TRY(bb::hip_status(who, e));
        BB_TRY(bb::hip_status(who, work.alloc(2 * cells + scan_bytes), BB_ERR_NOMEM));
        keep = (u64 *)work.p;
        pos = (u64 *)((char *)work.p + cells);
        e = bb::launch(sig_keep_kernel, dim3((unsigned)((m + kSfBlock - 1) / kSfBlock)), dim3(kSfBlock), 0, st,
                       (const double *)s->q.p, m, q_max, keep);
        if (e == hipSuccess)
            e = bb::exclusive_scan((char *)work.p + 2 * cells, scan_bytes, keep, pos, (size_t)m, st);
        u64 last_pos = 0, last_keep = 0;
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e == hipSuccess) e = hipMemcpy(&last_pos, pos + (m - 1), 8, hipMemcpyDeviceToHost);
        if (e == hipSuccess) e = hipMemcpy(&last_keep, keep + (m - 1), 8, hipMemcpyDeviceToHost);
        BB_TRY(bb::hip_status(who, e));
        sel->n = (int64_t)(last_pos + last_keep);
    }
    const size_t k = (size_t)sel->n;
    e = sel->row.alloc(k * 4);
    if (e == hipSuccess) e = sel->col.alloc(k * 4);
    if (e == hipSuccess) e = sel->count.alloc(k * 8);
    if (e == hipSuccess) e = sel->p.alloc(k * 8);
    if (e == hipSuccess) e = sel->q.alloc(k * 8);
    BB_TRY(bb::hip_status(who, e, BB_ERR_NOMEM));
    if (k > 0) {
        e = bb::launch(sig_pick_kernel, dim3((unsigned)((m + kSfBlock - 1) / kSfBlock)), dim3(kSfBlock), 0, st,
                       (const u64 *)keep, (const u64 *)pos, m, (const int *)s->row.p, (const int *)s->col.p,
                       (const double *)s->count.p, (const double *)s->p.p, (const double *)s->q.p,
                       sel->row.as<int>(), sel->col.as<int>(), sel->count.as<double>(), sel->p.as<double>(),
                       sel->q.as<double>());
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        BB_TRY(bb::hip_status(who, e));
    }
    *out = sel.release();
    return BB_OK;
}

int bb_sig_destroy(bb_sig *s) {
    if (!s) return BB_OK;
    (void)bb::enter_device(s->device);
    delete s;
    return BB_OK;
}

}  // extern "C"
