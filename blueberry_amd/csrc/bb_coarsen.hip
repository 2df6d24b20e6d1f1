// bb_coarsen.hip -- pooling a map to a coarser resolution on the device (docs/SPEC.md 2.12):
// bb_cm_coarsen (resident dense matrix -> a second, k^2 times smaller one) and bb_triples_coarsen
// (resident pixel list -> a new resident pixel list), with the read-back of a triples handle.
//
// The pooled value has a FIXED order of summation (SPEC 2.12): a row partial per fine row of the
// block, its cells added left to right, and the row partials added top to bottom, all from +0.0.
// An accumulator that starts at +0.0 never becomes -0.0 (x + (-x) is +0.0 in round-to-nearest),
// so adding a +-0.0 never changes its bits: a cell that is 0, masked (below the diagonal, beyond
// n_bins) or absent may be added as 0.0 or skipped, whichever is cheaper.  That is what makes
// the dense and the pixel-list route the same bits, and what lets both kernels pad.
//
//   coarsen_kernel   dense.  grid (row group, column tile); a workgroup owns the pooled cells
//               of Rc = max(1, 8 / k) coarse rows x WcT = min(512 / k, 256) coarse columns (one
//               coarse column, walked in tiles of 512 fine columns, when k > 512), i.e. at most
//               max(k, 8) x 512 fine cells: no item is long.  Workgroups below the diagonal
//               leave at once; cells below the diagonal are never loaded.
//               A step is kCoRows = 8 fine rows x up to kCoTile = 512 fine columns: wave w loads
//               rows 2 w and 2 w + 1, 8 loads of 64 contiguous doubles per row (8 B per lane,
//               512 B per wave and load, 16 loads in flight), and the NEXT step's loads are
//               issued before this step's sums (the barriers order LDS only: lds_barrier).
//               The tile goes through LDS because the order forbids a tree across the k
//               columns of a block: thread (row a, coarse column j) adds its k cells left to
//               right from LDS.  Coarse column j starts at j (k + 1) when k is even, so that
//               the 32 lanes of a ds_read_b64 group are an odd number of doubles apart
//               (conflict-free; a stride of k doubles would be gcd(k, 32)-way).  Then thread j
//               adds the rows' partials top to bottom into a register it keeps across the
//               ceil(k / 8) steps of its coarse row.
//   triples_pool_kernel   pixel list, over the canonical index (bb_triples.h): a workgroup owns
//               pooled row I and holds kCoChunk of its accumulators in LDS at a time (any nc
//               works: the row is walked in column chunks).  Fine rows in order, a barrier
//               between them; within a fine row the thread whose entry is the FIRST of its
//               coarse column adds that column's run left to right (at most k entries) and
//               then adds the run's sum to the accumulator, which no other thread touches for
//               this row.  Run twice: count (which pooled cells exist), scan, write.
#include <math.h>

#include <algorithm>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "bb_cm_internal.h"
#include "bb_common.h"
#include "bb_sort.h"
#include "bb_triples.h"

namespace bb {

// The constants of the two kernels (tests/test_gpu_coarsen.py names them).
constexpr int kCoRows = 8;        // fine rows of a step of coarsen_kernel
constexpr int kCoTile = 512;      // fine columns of a step, at most
constexpr int kCoCols = 256;      // coarse columns of a workgroup, at most
constexpr int kCoStride = 768;    // doubles per tile row in LDS: 512 + one pad per coarse column
constexpr int kCoChunk = 2048;    // pooled columns whose accumulators triples_pool_kernel holds

}  // namespace bb

namespace {

using bb::kCoChunk;
using bb::kCoCols;
using bb::kCoRows;
using bb::kCoStride;
using bb::kCoTile;
using bb::lds_barrier;

typedef unsigned long long u64;

// the number of fine cells pooled into (I, J), I <= J (SPEC 2.12, how='mean')
__device__ __forceinline__ double pooled_cells(int64_t I, int64_t J, int64_t k, int64_t n) {
    const int64_t hi = std::min<int64_t>(k, n - I * k), hj = std::min<int64_t>(k, n - J * k);
    return I == J ? (double)(hi * (hi + 1) / 2) : (double)(hi * hj);
}

// How the launch is cut; a function of (n, k) alone.
struct CoGeom {
    int64_t n, k, nc;     // fine bins, factor (<= max(n, 1)), coarse bins
    int rc;               // coarse rows of a workgroup: max(1, 8 / k)
    int rows_per;         // fine rows of one coarse row within a step: min(k, 8)
    int wct;              // coarse columns of a workgroup: min(512 / k, 256); 1 if k > 512
    int tw;               // fine columns of a step: wct k; 512 if k > 512
    int nct;              // column steps of a workgroup: 1; ceil(k / 512) if k > 512
    int nrc;              // row steps: 1 if k <= 8, else ceil(k / 8)
    int pad;              // 1: coarse column j starts at j (k + 1) in LDS (k even)
};

CoGeom co_geom(int64_t n, int64_t k) {
    CoGeom g;
    g.n = n, g.k = k, g.nc = (n + k - 1) / k;
    g.rc = (int)std::max<int64_t>(1, kCoRows / k);
    g.rows_per = (int)std::min<int64_t>(k, kCoRows);
    const bool wide = k > kCoTile;
    g.wct = wide ? 1 : (int)std::min<int64_t>(kCoTile / k, kCoCols);
    g.tw = wide ? kCoTile : (int)(g.wct * k);
    g.nct = wide ? (int)((k + kCoTile - 1) / kCoTile) : 1;
    g.nrc = k <= kCoRows ? 1 : (int)((k + kCoRows - 1) / kCoRows);
    g.pad = (!wide && k % 2 == 0) ? 1 : 0;
    return g;
}

__global__ __launch_bounds__(256) void coarsen_kernel(const double *__restrict__ m, int64_t ld, CoGeom g,
                                                      int mean, double *__restrict__ dst, int64_t ldd) {
    __shared__ double tile[kCoRows * kCoStride];
    __shared__ double rp[kCoRows * kCoCols];      // the row partials of the step's rows
    const int64_t k = g.k, n = g.n;
    const int64_t I0 = (int64_t)blockIdx.x * g.rc, J0 = (int64_t)blockIdx.y * g.wct;
    const int wj = (int)std::min<int64_t>(g.wct, g.nc - J0);    // coarse columns here
    if (J0 + wj - 1 < I0) return;                               // below the diagonal (whole workgroup)
    const int64_t a0 = I0 * k, a1 = std::min<int64_t>(n, (I0 + g.rc) * k);
    const int64_t c0 = J0 * k, c1 = std::min<int64_t>(n, (J0 + g.wct) * k);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int lpos[8];                                                // where column lane + 64 q goes in LDS
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int cl = lane + 64 * q;
        lpos[q] = cl + (g.pad ? cl / (int)k : 0);
    }
    const int jstride = (int)k + g.pad;
    const int run = g.nct == 1 ? (int)k : kCoTile;              // cells a row partial adds per step
    const int steps = g.nrc * g.nct;
    double v[2][8];
    auto load = [&](int s) {
        const int rs = s / g.nct, ct = s - rs * g.nct;
#pragma unroll
        for (int rr = 0; rr < 2; ++rr) {
            const int64_t row = a0 + (int64_t)rs * kCoRows + 2 * wave + rr;
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int cl = lane + 64 * q;
                const int64_t col = c0 + (int64_t)ct * g.tw + cl;
                const bool ok = cl < g.tw && row < a1 && col < c1 && col >= row;
                v[rr][q] = ok ? m[row * ld + col] : 0.0;
            }
        }
    };
    double acc = 0.0;       // nrc > 1: the pooled cell (I0, J0 + tid) so far
    load(0);
    for (int s = 0; s < steps; ++s) {
        const int rs = s / g.nct, ct = s - rs * g.nct;
        lds_barrier();      // (the last step's readers are done; LDS only: the loads stay in flight)
#pragma unroll
        for (int rr = 0; rr < 2; ++rr)
#pragma unroll
            for (int q = 0; q < 8; ++q)
                if (lane + 64 * q < g.tw) tile[(2 * wave + rr) * kCoStride + lpos[q]] = v[rr][q];
        if (s + 1 < steps) load(s + 1);
        lds_barrier();
        // row partials: row a of the step, coarse column j, left to right
        for (int t = tid; t < kCoRows * wj; t += 256) {
            const int a = t / wj, j = t - a * wj;
            const double *cell = tile + a * kCoStride + j * jstride;
            double r = ct == 0 ? 0.0 : rp[a * kCoCols + j];
            for (int b = 0; b < run; ++b) r += cell[b];
            rp[a * kCoCols + j] = r;
        }
        if (ct != g.nct - 1) continue;
        lds_barrier();
        // the rows' partials, top to bottom
        for (int t = tid; t < g.rc * wj; t += 256) {
            const int ci = t / wj, j = t - ci * wj;
            double sum = g.nrc > 1 ? acc : 0.0;                 // (nrc > 1: rc = 1 and wj <= 64 < 256)
            for (int r = 0; r < g.rows_per; ++r) sum += rp[(ci * (int)k + r) * kCoCols + j];
            acc = sum;
            const int64_t I = I0 + ci, J = J0 + j;
            if (rs == g.nrc - 1 && I < g.nc && J >= I) {
                const double out = mean ? sum / pooled_cells(I, J, k, n) : sum;
                dst[I * ldd + J] = out;
                if (J != I) dst[J * ldd + I] = out;
            }
        }
    }
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

// Pooled row blockIdx.x of the list (ptr, col, val).  WRITE false: count[I] = its pooled cells;
// true: their triples [I R, J R, value] from slot offset[I] on, J ascending (R: the new resolution).
template <bool WRITE>
__global__ __launch_bounds__(256) void triples_pool_kernel(const long long *__restrict__ ptr,
                                                           const int *__restrict__ col,
                                                           const double *__restrict__ val, int64_t n,
                                                           int64_t k, int64_t nc, int mean, double R,
                                                           const u64 *__restrict__ offset,
                                                           u64 *__restrict__ count,
                                                           double *__restrict__ out) {
    __shared__ double acc[kCoChunk];
    __shared__ int present[kCoChunk];
    __shared__ int before[256];
    constexpr int kOwn = kCoChunk / 256;          // consecutive slots a thread compacts
    const int tid = threadIdx.x;
    const int64_t I = blockIdx.x;
    const int64_t a0 = I * k, a1 = std::min<int64_t>(n, (I + 1) * k);
    u64 base = WRITE ? offset[I] : 0;
    for (int64_t Jc = I / kCoChunk * kCoChunk; Jc < nc; Jc += kCoChunk) {
        for (int j = tid; j < kCoChunk; j += 256) acc[j] = 0.0, present[j] = 0;
        __syncthreads();
        const int64_t fhi = (Jc + kCoChunk) * k;               // fine columns below this are the chunk's
        for (int64_t a = a0; a < a1; ++a) {
            const int64_t rb = ptr[a], re = ptr[a + 1];
            const int64_t e0 = first_at_least(col, rb, re, std::max<int64_t>(a, Jc * k));
            const int64_t e1 = fhi >= n ? re : first_at_least(col, e0, re, fhi);
            for (int64_t e = e0 + tid; e < e1; e += 256) {
                const int64_t J = col[e] / (int)k;
                if (e != e0 && col[e - 1] / (int)k == J) continue;   // not the first of its run
                present[J - Jc] = 1;
                if (WRITE) {
                    const int64_t end = (J + 1) * k;
                    double r = 0.0;
                    for (int64_t f = e; f < e1 && col[f] < end; ++f) r += val[f];
                    acc[J - Jc] += r;
                }
            }
            __syncthreads();                                    // the next row adds to the same cells
        }
        // the chunk's pooled cells to their places, J ascending
        int mine = 0;
#pragma unroll
        for (int q = 0; q < kOwn; ++q) mine += present[tid * kOwn + q];
        before[tid] = mine;
        __syncthreads();
        for (int off = 1; off < 256; off <<= 1) {
            const int add = tid >= off ? before[tid - off] : 0;
            __syncthreads();
            before[tid] += add;
            __syncthreads();
        }
        const u64 chunk_total = (u64)before[255];
        if (WRITE) {
            u64 p = base + (u64)(before[tid] - mine);
            for (int q = 0; q < kOwn; ++q) {
                const int s = tid * kOwn + q;
                if (!present[s]) continue;
                const int64_t J = Jc + s;
                out[3 * p] = (double)I * R;
                out[3 * p + 1] = (double)J * R;
                out[3 * p + 2] = mean ? acc[s] / pooled_cells(I, J, k, n) : acc[s];
                ++p;
            }
        }
        base += chunk_total;
        __syncthreads();                                        // (acc, present and before are reused)
    }
    if (!WRITE && tid == 0) count[I] = base;
}

int check_pooling(const char *who, int64_t n_bins, int64_t factor, int how) {
    BB_REQUIRE(n_bins >= 0, std::string(who) + ": n_bins must not be negative");
    BB_REQUIRE(factor >= 1, std::string(who) + ": factor must be at least 1");
    BB_REQUIRE(how == BB_COARSEN_SUM || how == BB_COARSEN_MEAN,
               std::string(who) + ": how must be BB_COARSEN_SUM or BB_COARSEN_MEAN");
    return BB_OK;
}

// A factor beyond n_bins pools everything into bin 0, as n_bins itself does.
inline int64_t effective_factor(int64_t n_bins, int64_t factor) {
    return std::min(factor, std::max<int64_t>(n_bins, 1));
}

}  // namespace

extern "C" {

int bb_cm_coarsen(const bb_cm *src, int64_t n_bins, int64_t factor, int how, bb_cm *dst) {
    const char *who = "bb_cm_coarsen";
    BB_TRY(bb::cm_check(src, who));
    BB_REQUIRE(dst != nullptr && dst != src, std::string(who) + ": dst must be another contact map");
    BB_TRY(check_pooling(who, n_bins, factor, how));
    BB_TRY(bb::cm_check_bins(src, n_bins, who));
    const int64_t k = effective_factor(n_bins, factor);
    const CoGeom g = co_geom(n_bins, k);
    BB_REQUIRE(dst->device == src->device, std::string(who) + ": dst is on another device");
    BB_REQUIRE(dst->d == g.nc + 1, std::string(who) + ": dst's edge must be ceil(n_bins / factor) + 1");
    const int64_t gx = (g.nc + g.rc - 1) / g.rc, gy = (g.nc + g.wct - 1) / g.wct;
    BB_REQUIRE(gy <= 65535, std::string(who) + ": the map is too large");
    hipStream_t st = src->stream;
    bb::StageClock<2> clock;
    hipError_t e = clock.start();
    // (the lower triangle's and the padding's cells that the kernel does not write)
    if (e == hipSuccess) e = hipMemsetAsync(dst->m, 0, (size_t)dst->d * dst->d * sizeof(double), st);
    if (e == hipSuccess) e = clock.mark(0, st);
    if (e == hipSuccess && g.nc > 0)
        e = bb::launch(coarsen_kernel, dim3((unsigned)gx, (unsigned)gy), dim3(256), 0, st,
                       (const double *)src->m, src->d, g, how == BB_COARSEN_MEAN ? 1 : 0, dst->m, dst->d);
    if (e == hipSuccess) e = clock.mark(1, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e == hipSuccess) e = clock.read(0, &dst->coarsen_ms);
    return bb::hip_status(who, e);
}

int bb_cm_coarsen_timing(const bb_cm *dst, double *kernel_ms) {
    BB_REQUIRE(dst != nullptr && kernel_ms != nullptr, "bb_cm_coarsen_timing: NULL argument");
    *kernel_ms = dst->coarsen_ms;
    return BB_OK;
}

int bb_triples_coarsen(bb_triples *src, int64_t n_bins, int64_t factor, int how, bb_triples **out) {
    const char *who = "bb_triples_coarsen";
    BB_REQUIRE(out != nullptr, std::string(who) + ": out is NULL");
    *out = nullptr;
    BB_REQUIRE(src != nullptr, std::string(who) + ": triples is NULL");
    BB_TRY(check_pooling(who, n_bins, factor, how));
    BB_REQUIRE(src->resolution * (double)factor <= 2147483647.0,
               std::string(who) + ": resolution x factor does not fit 31 bits");
    BB_TRY(bb::triples_ensure_index(src, n_bins, who));
    const int64_t k = effective_factor(n_bins, factor);
    const int64_t nc = (n_bins + k - 1) / k;
    const double R = src->resolution * (double)factor;
    const bb::SegmentedList &rows = src->index.rows;
    std::unique_ptr<bb_triples> t(new (std::nothrow) bb_triples());
    if (!t) return bb::fail(BB_ERR_NOMEM, std::string(who) + ": out of host memory");
    t->device = src->device;
    t->resolution = R;
    hipStream_t st = nullptr;
    bb::DevBuf count, offset, tmp;
    bb::StageClock<2> clock;                      // count + scan + write
    size_t scan_bytes = 0;
    u64 total = 0;
    hipError_t e = count.alloc((size_t)(nc + 1) * 8);
    if (e == hipSuccess) e = offset.alloc((size_t)(nc + 1) * 8);
    if (e == hipSuccess) e = bb::exclusive_scan_bytes((size_t)(nc + 1), &scan_bytes);
    if (e == hipSuccess) e = tmp.alloc(scan_bytes);
    BB_TRY(bb::hip_status(who, e, BB_ERR_NOMEM));
    e = clock.start();
    if (e == hipSuccess) e = hipMemsetAsync(count.p, 0, (size_t)(nc + 1) * 8, st);
    if (e == hipSuccess) e = clock.mark(0, st);
    if (e == hipSuccess && nc > 0)
        e = bb::launch(triples_pool_kernel<false>, dim3((unsigned)nc), dim3(256), 0, st,
                       (const long long *)rows.ptr.p, (const int *)rows.other.p,
                       (const double *)rows.val.p, n_bins, k, nc, 0, R, (const u64 *)nullptr,
                       count.as<u64>(), (double *)nullptr);
    // (count[nc] is 0: offset[nc] is the number of pooled cells)
    if (e == hipSuccess)
        e = bb::exclusive_scan(tmp.p, scan_bytes, count.as<u64>(), offset.as<u64>(), (size_t)(nc + 1), st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e == hipSuccess) e = hipMemcpy(&total, offset.as<u64>() + nc, 8, hipMemcpyDeviceToHost);
    BB_TRY(bb::hip_status(who, e));
    t->n = (int64_t)total;
    BB_TRY(bb::hip_status(who, t->d.alloc((size_t)total * 24), BB_ERR_NOMEM));
    if (total > 0)
        e = bb::launch(triples_pool_kernel<true>, dim3((unsigned)nc), dim3(256), 0, st,
                       (const long long *)rows.ptr.p, (const int *)rows.other.p,
                       (const double *)rows.val.p, n_bins, k, nc, how == BB_COARSEN_MEAN ? 1 : 0, R,
                       (const u64 *)offset.p, (u64 *)nullptr, t->d.as<double>());
    if (e == hipSuccess) e = clock.mark(1, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e == hipSuccess) e = clock.read(0, &t->coarsen_ms);
    BB_TRY(bb::hip_status(who, e));
    *out = t.release();
    return BB_OK;
}

int bb_triples_coarsen_timing(const bb_triples *dst, double *pool_ms) {
    BB_REQUIRE(dst != nullptr && pool_ms != nullptr, "bb_triples_coarsen_timing: NULL argument");
    *pool_ms = dst->coarsen_ms;
    return BB_OK;
}

int bb_triples_size(const bb_triples *t, int64_t *n) {
    BB_REQUIRE(t != nullptr && n != nullptr, "bb_triples_size: NULL argument");
    *n = t->n;
    return BB_OK;
}

int bb_triples_download(const bb_triples *t, double *triples) {
    BB_REQUIRE(t != nullptr, "bb_triples_download: triples is NULL");
    BB_REQUIRE(t->n == 0 || triples != nullptr, "bb_triples_download: NULL buffer");
    BB_TRY(bb::enter_device(t->device));
    if (t->n == 0) return BB_OK;
    if (t->st == 3)
        return bb::hip_status("bb_triples_download",
                              hipMemcpy(triples, t->d.p, (size_t)t->n * 24, hipMemcpyDeviceToHost));
    // the handle holds the reference's column-major (3, n): turned on the host
    std::vector<double> cols;
    try {
        cols.resize((size_t)t->n * 3);
    } catch (const std::bad_alloc &) {
        return bb::fail(BB_ERR_NOMEM, "bb_triples_download: out of host memory");
    }
    BB_TRY(bb::hip_status("bb_triples_download",
                          hipMemcpy(cols.data(), t->d.p, (size_t)t->n * 24, hipMemcpyDeviceToHost)));
    for (int64_t i = 0; i < t->n; ++i)
        for (int c = 0; c < 3; ++c) triples[3 * i + c] = cols[(size_t)(c * t->n + i)];
    return BB_OK;
}

}  // extern "C"
