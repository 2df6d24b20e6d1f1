// bb_score.hip -- scoring a structure against the resident map (docs/SPEC.md 2.8, DESIGN.md
// 4.16): one pass over a rank's units that forms, in float64, nine sums per genomic separation
// k = j - i and three sums per bin over the constrained pairs.  No iteration, no solver state:
// bb_solver_score (bb_solver_queries.hip) checks the handle and hands its views in (bb_score.h).
// gfx950 only.
//
// Three kernels, no floating-point atomics, every sum in an order fixed by the layout and the
// rank's unit range:
//   score_profile_kernel  one workgroup per RUN (the consecutive local units of one tile); a
//                         thread owns tile-relative diagonals and keeps their nine sums in
//                         registers; every unit is read once, a matrix row by consecutive threads
//   score_fold_kernel     profile[k][col] = the runs' sums of diagonal k, in run order
//   score_bins_kernel     one wave per bin over its row and its column of the units
//
// Slot memory of a call: n_runs * (2 vw - 1) * 9 * 8 bytes (73,656 B per run at vw = 512, a run
// being at most one tile: 1 MiB of fp32 units, 2 MiB of fp64), + (9 + 3) * 8 * n_bins for the two
// results and 16 B per run of indices.  One allocation, made for the call and released with it.
//
// The log-log sums of SPEC 2.11 (bb_solver_loglog) are the same pass with other terms: the
// profile and fold kernels take what a pair adds (ScoreTerms: 9 columns, LogTerms: 7) as a
// template parameter, so the slot scheme, the order of every sum and the reads are shared.
#include <cmath>
#include <vector>

#include "bb_common.h"
#include "bb_device_sums.h"
#include "bb_score.h"

namespace {

constexpr int kProfileCols = 9, kBinCols = 3, kLogCols = 7;

// |x_i - x_j| in float64: products and sums rounded one by one, ((dx^2 + dy^2) + dz^2), and a
// correctly rounded root.  No floor: nothing divides by it.
__device__ __forceinline__ double pair_distance(double xi, double yi, double zi, double xj, double yj,
                                                double zj) {
#pragma clang fp contract(off)
    const double dx = xi - xj, dy = yi - yj, dz = zi - zj;
    return sqrt((dx * dx + dy * dy) + dz * dz);
}

// The terms of SPEC 2.8 that hold a residual, as written there (never from the moments).
struct Residuals {
    double sq, sammon, rel;   // (d - delta)^2, (d - delta)^2 / delta, ((d - delta) / delta)^2
};
__device__ __forceinline__ Residuals residuals(double d, double delta) {
#pragma clang fp contract(off)
    const double res = d - delta, u = res / delta;
    return {res * res, (res * res) / delta, u * u};
}

// What a pair adds to the sums of its diagonal: the nine columns of SPEC 2.8 ...
struct ScoreTerms {
    static constexpr int COLS = kProfileCols;
    static __device__ __forceinline__ void add(double (&a)[COLS], double d, double delta) {
#pragma clang fp contract(off)
        const Residuals r = residuals(d, delta);
        a[0] += 1.0;
        a[1] += d;
        a[2] += delta;
        a[3] += d * d;
        a[4] += delta * delta;
        a[5] += d * delta;
        a[6] += r.sq;
        a[7] += r.sammon;
        a[8] += r.rel;
    }
};
// ... or the seven of SPEC 2.11: u = log delta, v = log d, products rounded one by one.  A pair
// with d = 0 has no logarithm: it is counted on its own (column 6) and adds nothing else.  So is
// a d that is not a number (the solver's own coordinates after a fit that diverged; a given xyz
// is checked to be finite): the caller that scores its own coordinates checks them.
struct LogTerms {
    static constexpr int COLS = kLogCols;
    static __device__ __forceinline__ void add(double (&a)[COLS], double d, double delta) {
#pragma clang fp contract(off)
        if (!(d > 0.0)) {
            a[6] += 1.0;
            return;
        }
        const double u = log(delta), v = log(d);
        a[0] += 1.0;
        a[1] += u;
        a[2] += v;
        a[3] += u * u;
        a[4] += v * v;
        a[5] += u * v;
    }
};

// runs[b] = {first local unit, units} of run b: consecutive local units of ONE tile (same strip
// j0, same block of rows I0 = i0 - i0 % VW).  Thread t owns the diagonals o = t + 256 m of the
// tile, o = (j - j0) - (i - I0) + VW - 1 in [0, 2 VW - 2]; in matrix row i its column is
// c = o - (VW - 1) + (i - I0), so consecutive threads read consecutive elements and every
// element of the row has exactly one reader.  slots: (Terms::COLS, 2 VW - 1) doubles per run.
template <typename T, int VW, int RPU, typename Terms>
__global__ __launch_bounds__(256) void score_profile_kernel(const T *__restrict__ units,
                                                            const int2 *__restrict__ udesc,
                                                            const int2 *__restrict__ runs,
                                                            const double *__restrict__ xyz,
                                                            int64_t n_bins, double *__restrict__ slots) {
    constexpr int NO = 2 * VW - 1, OPT = (NO + 255) / 256;
    __shared__ double xs[3 * VW];             // the strip's coordinates
    const int2 run = runs[blockIdx.x];
    const int2 first = udesc[run.x];
    const int j0 = first.y, I0 = first.x - first.x % VW;
    for (int q = threadIdx.x; q < 3 * VW; q += 256) xs[q] = xyz[(int64_t)j0 * 3 + q];
    __syncthreads();
    constexpr int COLS = Terms::COLS;
    double acc[OPT][COLS];
#pragma unroll
    for (int m = 0; m < OPT; ++m)
#pragma unroll
        for (int q = 0; q < COLS; ++q) acc[m][q] = 0.0;

    for (int u = 0; u < run.y; ++u) {
        const int64_t ul = (int64_t)run.x + u;
        const int i0 = first.x + u * RPU;
        const T *in = units + ul * (RPU * VW);
        // the whole unit first (8 KiB in flight per workgroup), then its arithmetic
        T v[RPU][OPT];
#pragma unroll
        for (int r = 0; r < RPU; ++r)
#pragma unroll
            for (int m = 0; m < OPT; ++m) {
                const int c = (int)threadIdx.x + 256 * m - (VW - 1) + (i0 + r - I0);
                v[r][m] = (c >= 0 && c < VW) ? in[r * VW + c] : T(0);
            }
#pragma unroll
        for (int r = 0; r < RPU; ++r) {
            const int i = i0 + r;
            const int64_t ic = i < n_bins ? i : 0;          // (rows past the map hold no pair)
            const double xi = xyz[3 * ic], yi = xyz[3 * ic + 1], zi = xyz[3 * ic + 2];
#pragma unroll
            for (int m = 0; m < OPT; ++m) {
                const int c = (int)threadIdx.x + 256 * m - (VW - 1) + (i - I0);
                const int64_t j = (int64_t)j0 + c;
                const double delta = (double)v[r][m];
                if (c >= 0 && c < VW && j > i && j < n_bins && delta > 0.0)
                    Terms::add(acc[m], pair_distance(xi, yi, zi, xs[3 * c], xs[3 * c + 1], xs[3 * c + 2]),
                               delta);
            }
        }
    }
    double *slot = slots + (int64_t)blockIdx.x * (COLS * NO);
#pragma unroll
    for (int m = 0; m < OPT; ++m) {
        const int o = (int)threadIdx.x + 256 * m;
        if (o < NO)
#pragma unroll
            for (int q = 0; q < COLS; ++q) slot[q * NO + o] = acc[m][q];
    }
}

// profile[k][col] = the sum over the runs that hold diagonal k, in run order.  A run of tile
// (I, J) holds k at o = k - (J - I) VW + VW - 1, so only D = J - I in {k / VW, k / VW + 1} can:
// diff_runs[diff_ptr[D] .. diff_ptr[D + 1]) lists the runs of tile difference D in run order.
template <int VW, int COLS>
__global__ __launch_bounds__(256) void score_fold_kernel(const double *__restrict__ slots,
                                                         const int *__restrict__ diff_ptr,
                                                         const int *__restrict__ diff_runs, int n_blocks,
                                                         int64_t n_bins, double *__restrict__ profile) {
    constexpr int NO = 2 * VW - 1;
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int col = blockIdx.y;
    if (k >= n_bins) return;
    double s = 0.0;
    if (k > 0) {
        const int q = (int)(k / VW);
        for (int D = q; D <= q + 1 && D < n_blocks; ++D) {
            const int o = (int)(k - (int64_t)D * VW) + VW - 1;
            if (o < 0) continue;
            for (int p = diff_ptr[D]; p < diff_ptr[D + 1]; ++p)
                s += slots[(int64_t)diff_runs[p] * (COLS * NO) + col * NO + o];
        }
    }
    profile[k * COLS + col] = s;
}

// Per bin i: pairs, sum (d - delta)^2 and sum ((d - delta) / delta)^2 over this rank's stored
// pairs that hold i.  One wave per bin, as the weighted degrees (unit_weight_sums_kernel): the
// row side walks row i of every strip J >= block(i), lane l taking the columns l, l + 64, ...;
// the column side walks column i of strip block(i), lane l taking the row groups l, l + 64, ...;
// units are found by binary search in udesc (ordered by (j0, i0)).  Who adds which pair, and
// when, depends on the pair's position alone.
template <typename T, int VW, int RPU>
__global__ __launch_bounds__(256) void score_bins_kernel(const T *__restrict__ units,
                                                         const int2 *__restrict__ udesc, int64_t n_local,
                                                         const double *__restrict__ xyz, int64_t n_bins,
                                                         double *__restrict__ bins) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n_bins) return;
    auto lower = [&](int j0, int i0) -> int64_t {   // first local unit not below (j0, i0)
        int64_t lo = 0, hi = n_local;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            const int2 d = udesc[mid];
            if (d.y < j0 || (d.y == j0 && d.x < i0)) lo = mid + 1;
            else hi = mid;
        }
        return lo;
    };
    const double xi = xyz[3 * i], yi = xyz[3 * i + 1], zi = xyz[3 * i + 2];
    double cnt = 0.0, sq = 0.0, rel = 0.0;
    auto add = [&](double delta, int64_t j) {
        if (!(delta > 0.0)) return;
        const Residuals r =
            residuals(pair_distance(xi, yi, zi, xyz[3 * j], xyz[3 * j + 1], xyz[3 * j + 2]), delta);
        cnt += 1.0;
        sq += r.sq;
        rel += r.rel;
    };
    const int b = (int)(i / VW);
    const int n_blocks = (int)((n_bins + VW - 1) / VW);
    const int i0 = (int)(i - i % RPU), r = (int)(i % RPU);
    for (int J = b; J < n_blocks; ++J) {
        const int64_t ul = lower(J * VW, i0);
        if (ul >= n_local || udesc[ul].y != J * VW || udesc[ul].x != i0) continue;
        const T *row = units + ul * (RPU * VW) + (int64_t)r * VW;
        for (int c = lane; c < VW; c += 64) {
            const int64_t j = (int64_t)J * VW + c;
            if (j > i && j < n_bins) add((double)row[c], j);
        }
    }
    const int c = (int)(i - (int64_t)b * VW);
    for (int64_t p = lane; p * RPU < i; p += 64) {
        const int64_t ul = lower(b * VW, (int)(p * RPU));
        if (ul >= n_local || udesc[ul].y != b * VW || udesc[ul].x != (int)(p * RPU)) continue;
        const T *col = units + ul * (RPU * VW) + c;
        for (int q = 0; q < RPU; ++q)
            if (p * RPU + q < i) add((double)col[q * VW], p * RPU + q);
    }
    cnt = bb::wave_sum_all(cnt);
    sq = bb::wave_sum_all(sq);
    rel = bb::wave_sum_all(rel);
    if (lane == 0) {
        bins[i * kBinCols] = cnt;
        bins[i * kBinCols + 1] = sq;
        bins[i * kBinCols + 2] = rel;
    }
}

// Terms = ScoreTerms: profile (n, 9) and bins (n, 3).  Terms = LogTerms: profile (n, 7), bins NULL
// (no per-bin kernel runs).
template <typename T, int VW, int RPU, typename Terms>
int score_pass_t(const bb::ScoreInput &in, double *profile, double *bins, double *ms) {
    constexpr int64_t NO = 2 * VW - 1;
    constexpr int COLS = Terms::COLS;
    const int64_t n = in.n_bins, n_blocks = (n + VW - 1) / VW;
    // the runs, and per tile difference D = J - I the runs that have it, in run order
    std::vector<int2> runs;
    std::vector<int> run_diff;
    for (int64_t ul = 0; ul < in.n_local; ++ul) {
        const int2 d = in.udesc[ul];
        const int I = d.x / VW, J = d.y / VW;
        if (!runs.empty()) {
            const int2 f = in.udesc[runs.back().x];
            if (f.y == d.y && f.x / VW == I) {
                ++runs.back().y;
                continue;
            }
        }
        runs.push_back(make_int2((int)ul, 1));
        run_diff.push_back(J - I);
    }
    const int64_t n_runs = (int64_t)runs.size();
    std::vector<int> diff_ptr((size_t)n_blocks + 2, 0), diff_runs((size_t)n_runs);
    for (int64_t b = 0; b < n_runs; ++b) ++diff_ptr[(size_t)run_diff[(size_t)b] + 1];
    for (int64_t D = 0; D <= n_blocks; ++D) diff_ptr[(size_t)D + 1] += diff_ptr[(size_t)D];
    {
        std::vector<int> fill(diff_ptr.begin(), diff_ptr.end() - 1);
        for (int64_t b = 0; b < n_runs; ++b) diff_runs[(size_t)fill[(size_t)run_diff[(size_t)b]]++] = (int)b;
    }

    const size_t slot_bytes = bb::align256((size_t)(n_runs * NO * COLS) * sizeof(double));
    const size_t prof_bytes = bb::align256((size_t)n * COLS * sizeof(double));
    const size_t bins_bytes = bins ? bb::align256((size_t)n * kBinCols * sizeof(double)) : 0;
    const size_t runs_bytes = bb::align256((size_t)n_runs * sizeof(int2));
    const size_t ptr_bytes = bb::align256(diff_ptr.size() * sizeof(int));
    const size_t list_bytes = bb::align256((size_t)n_runs * sizeof(int));
    bb::DevBuf buf;                                  // released when the call returns
    BB_TRY(bb::alloc_status(buf, slot_bytes + prof_bytes + bins_bytes + runs_bytes + ptr_bytes + list_bytes));
    char *p = buf.as<char>();
    double *d_slots = (double *)p;
    double *d_profile = (double *)(p += slot_bytes);
    double *d_bins = (double *)(p += prof_bytes);
    int2 *d_runs = (int2 *)(p += bins_bytes);
    int *d_diff_ptr = (int *)(p += runs_bytes);
    int *d_diff_runs = (int *)(p += ptr_bytes);

    hipStream_t st = in.stream;
    BB_HIP_CHECK(hipMemcpyAsync(d_runs, runs.data(), (size_t)n_runs * sizeof(int2), hipMemcpyHostToDevice, st));
    BB_HIP_CHECK(hipMemcpyAsync(d_diff_ptr, diff_ptr.data(), diff_ptr.size() * sizeof(int),
                                hipMemcpyHostToDevice, st));
    BB_HIP_CHECK(hipMemcpyAsync(d_diff_runs, diff_runs.data(), (size_t)n_runs * sizeof(int),
                                hipMemcpyHostToDevice, st));
    bb::StageClock<4> clock;                         // profile | fold | bins
    BB_HIP_CHECK(clock.start(ms != nullptr));
    BB_HIP_CHECK(clock.mark(0, st));
    BB_HIP_CHECK(bb::launch(score_profile_kernel<T, VW, RPU, Terms>, dim3((unsigned)n_runs), dim3(256), 0, st,
                            (const T *)in.d_units, in.d_udesc, d_runs, in.d_xyz, n, d_slots));
    BB_HIP_CHECK(clock.mark(1, st));
    BB_HIP_CHECK(bb::launch(score_fold_kernel<VW, COLS>, dim3((unsigned)((n + 255) / 256), COLS), dim3(256),
                            0, st, d_slots, d_diff_ptr, d_diff_runs, (int)n_blocks, n, d_profile));
    BB_HIP_CHECK(clock.mark(2, st));
    if (bins) {
        BB_HIP_CHECK(bb::launch(score_bins_kernel<T, VW, RPU>, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st,
                                (const T *)in.d_units, in.d_udesc, in.n_local, in.d_xyz, n, d_bins));
        BB_HIP_CHECK(clock.mark(3, st));
    }
    BB_HIP_CHECK(hipMemcpyAsync(profile, d_profile, (size_t)n * COLS * sizeof(double),
                                hipMemcpyDeviceToHost, st));
    if (bins)
        BB_HIP_CHECK(hipMemcpyAsync(bins, d_bins, (size_t)n * kBinCols * sizeof(double), hipMemcpyDeviceToHost, st));
    BB_HIP_CHECK(hipStreamSynchronize(st));
    if (ms) BB_HIP_CHECK(clock.read_all(ms));        // (no per-bin kernel: its entry is 0)
    return BB_OK;
}

}  // namespace

namespace bb {

namespace {
template <typename Terms>
int pass_by_shape(const ScoreInput &in, double *profile, double *bins, double *ms) {
    for (int64_t q = 0; q < in.n_bins * Terms::COLS; ++q) profile[q] = 0.0;
    if (bins)
        for (int64_t q = 0; q < in.n_bins * kBinCols; ++q) bins[q] = 0.0;
    if (ms) ms[0] = ms[1] = ms[2] = 0.0;
    if (in.n_local == 0) return BB_OK;             // a rank without units: zeros
    // the three unit shapes of docs/SPEC.md 3 (Lay<T, W> of the solver's kernels)
    if (in.dtype == BB_F32) return score_pass_t<float, 512, 4, Terms>(in, profile, bins, ms);
    if (in.wide) return score_pass_t<double, 512, 2, Terms>(in, profile, bins, ms);
    return score_pass_t<double, 128, 8, Terms>(in, profile, bins, ms);
}
}  // namespace

int score_pass(const ScoreInput &in, double *profile, double *bins, double *ms) {
    return pass_by_shape<ScoreTerms>(in, profile, bins, ms);
}

int loglog_pass(const ScoreInput &in, double *profile, double *ms) {
    return pass_by_shape<LogTerms>(in, profile, nullptr, ms);
}

}  // namespace bb
