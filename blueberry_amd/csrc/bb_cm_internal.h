// bb_cm_internal.h -- what the translation units that work on a resident ContactMap matrix
// share: the handle itself (bb_contactmap.hip owns its lifetime) and its checks, the per-device
// grow-only scratch that holds matrix-sized temporaries (bb_cm_correlation,
// bb_cm_shortest_paths), the workgroup sum of their fixed-order reductions, and the symmetric
// matrix-vector product over the upper triangle: ONE body of a work item behind the two kernels
// (symv_upper_kernel in bb_contactmap.hip: symv, eigenvector; band_symv_kernel in
// bb_balance.hip: the banded product of the balancing iteration), its work lists, its scratch
// on the handle, its enqueue and its reduce kernel.
#pragma once

#include <float.h>
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <string>
#include <vector>

#include "bb_common.h"
#include "bb_device_sums.h"

namespace bb {

// ---- the symmetric product over the upper triangle ---------------------------------------------
// y = M x from the UPPER triangle alone (round 3).  Reading both triangles of a symmetric
// matrix costs 8 B per element where 8 B per PAIR will do (round 2's kernel did that: 4.25
// TB/s, 53 % of peak, on its own accounting).  Here element (i, j),
// j >= i, is read once and serves both ends, y_i += m_ij x_j and y_j += m_ij x_i -- the
// pattern of the solver's sweep (kOpMatvec2).  The matrix is taken to be symmetric, as the
// reference's eigsh call takes it (datatypes.pyx:234) and as every ContactMap is built.
//   work item   64 rows (4 waves x 16) x up to 4096 columns of the upper triangle; the list
//               is cut by rows AND columns so that no item is long (a row block alone would
//               be 0.2 to 12.8 MB at d = 25k and the launch as slow as its longest)
//   row side    16 per-lane accumulators per wave, reduced across the lanes once per item
//               -> rowpart[segment][row]
//   column side a lane owns one column of a 64-column chunk; the 16 rows of the wave add
//               into one register; after 8 chunks the 4 waves' sums meet in LDS and leave
//               as one value per column -> colpart[row block][column] (1.5 % of the bytes read)
//   symv_reduce_kernel adds, per element of y, its row partials (<= n / 4096 + 1) and its
//               column partials (<= n / 64 + 1) in a fixed order, 8 slices in parallel.
// All loads are 8 bytes per lane, 512 contiguous bytes per wave: rows of an odd-d matrix
// start 8 bytes off every other time, and 16 loads of a wave are in flight per chunk.
//
// A work item is kSvRows rows x up to kSvSeg columns; kSvGroup chunks of 64 columns are in
// flight per wave at a time.
constexpr int kSvRows = 64, kSvSeg = 4096, kSvGroup = 8;

// A workgroup barrier that orders LDS only.  __syncthreads() is also a release of the
// wave's GLOBAL stores: s_waitcnt vmcnt(0) in front of every s_barrier, i.e. the write
// acknowledgements of a whole tile (and the next tile's loads) twice per tile.  The tile
// pair belongs to this workgroup alone and no thread reads a global cell another thread
// of the launch writes, so nothing global needs ordering here.
__device__ __forceinline__ void lds_barrier() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// What a cell contributes, formed as the cell is loaded: its value, "is not 0", or "is negative
// or not finite".  Under kCellBad the column side is switched off (its multiplier x_row is
// taken as 0), so that every cell of the counted upper triangle is seen once, by the row side:
// sum(y) = the number of offending cells.
enum { kCellValue = 0, kCellNonzero = 1, kCellBad = 2 };
template <int MODE>
__device__ __forceinline__ double cell_term(double a) {
    if (MODE == kCellValue) return a;
    if (MODE == kCellNonzero) return a != 0.0 ? 1.0 : 0.0;
    return !(a >= 0.0 && a <= DBL_MAX) ? 1.0 : 0.0;      // negative, NaN, +inf
}

// Work item blockIdx.x of the product over the leading n x n block of a matrix with row stride
// ld.  A cell (row, c) counts on the row side from c = row + off_row on and on the column side
// from c = row + off_col on; off_col >= 1: the diagonal never counts there (it would add
// m_ii x_i twice).  The plain product is ld = n, off_row = 0, off_col = 1, all of them
// compile-time constants of its kernel once this is inlined.  A cell that does not count is
// SELECTED out where the products are formed, never multiplied by 0.
template <int MODE>
__device__ __forceinline__ void symv_item(const double *__restrict__ m, int64_t ld, int64_t n,
                                          int64_t off_row, int64_t off_col,
                                          const double *__restrict__ x, const int2 *__restrict__ items,
                                          double *__restrict__ rowpart, double *__restrict__ colpart) {
    __shared__ double meet[4][kSvGroup][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int2 it = items[blockIdx.x];
    const int64_t I = it.x, S = it.y;
    const int64_t row0 = I * kSvRows + wave * 16;
    const int64_t c_begin = std::max<int64_t>(I * kSvRows, S * kSvSeg);
    const int64_t c_end = std::min<int64_t>(n, (S + 1) * (int64_t)kSvSeg);
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
            // plain loads: the 512-byte segments of a wave are not line-aligned (odd d),
            // neighbouring chunks share their end lines, and a non-temporal load does not leave
            // them in L2 for the neighbour -- 481 against 505 us per product at d = 24,927
            double a[16];
#pragma unroll
            for (int r = 0; r < 16; ++r)
                a[r] = (in_c && row0 + r < n) ? cell_term<MODE>(m[(row0 + r) * ld + c]) : 0.0;
            if (c0 < row0 + 15 + off_col) {
                // the chunk holds a cell of this wave's rows that does not count on the column
                // side: one below the diagonal, on it, or inside the band
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int64_t row = row0 + r;
                    racc[r] = fma(c >= row + off_row ? a[r] : 0.0, xc, racc[r]);
                    cacc[g] = fma(c >= row + off_col ? a[r] : 0.0, xr[r], cacc[g]);
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
        const double v = bb::wave_sum_first(racc[r]);
        if (lane == 0 && row0 + r < n) rowpart[S * n + row0 + r] = v;
    }
}

// A work list: every (row block I, segment S) that `enumerate` names and that has a cell
// (len > 0), longest first -- the dispatcher hands the items out in order -- and in the order
// of the enumeration among equals.
template <typename Enumerate, typename Len>
std::vector<int2> items_longest_first(Enumerate enumerate, Len len) {
    std::vector<int2> items;
    enumerate([&](int64_t I, int64_t S) {
        const int2 t = make_int2((int)I, (int)S);
        if (len(t) > 0) items.push_back(t);
    });
    std::stable_sort(items.begin(), items.end(),
                     [&](const int2 &a, const int2 &b) { return len(a) > len(b); });
    return items;
}

// The product over an n x n upper triangle: S is a segment of kSvSeg COLUMNS; an item runs from
// the diagonal (or the segment's start) to the segment's end.
inline std::vector<int2> symv_items(int64_t n) {
    const int64_t nrb = (n + kSvRows - 1) / kSvRows, nseg = (n + kSvSeg - 1) / kSvSeg;
    return items_longest_first(
        [&](auto item) {
            for (int64_t S = nseg - 1; S >= 0; --S)
                for (int64_t I = 0; I < nrb && I * kSvRows < (S + 1) * (int64_t)kSvSeg; ++I) item(I, S);
        },
        [&](const int2 &t) {
            return std::min<int64_t>(n, (t.y + 1) * (int64_t)kSvSeg) -
                   std::max<int64_t>((int64_t)t.x * kSvRows, (int64_t)t.y * kSvSeg);
        });
}

// The diagonal pass (diag_sums_kernel, bb_balance.hip): S is a segment of kSvSeg DIAGONALS of
// the n - 64 I that row block I has.
inline std::vector<int2> diag_items(int64_t n) {
    const int64_t nrb = (n + kSvRows - 1) / kSvRows;
    return items_longest_first(
        [&](auto item) {
            for (int64_t I = 0; I < nrb; ++I)
                for (int64_t S = 0; S * kSvSeg < n - I * kSvRows; ++S) item(I, S);
        },
        [&](const int2 &t) {
            return std::min<int64_t>(n - (int64_t)t.x * kSvRows, (t.y + 1) * (int64_t)kSvSeg) -
                   (int64_t)t.y * kSvSeg;
        });
}

// The product's grow-only scratch for one size n: product work list | diagonal work list (if
// asked for) | partial sums, each at a 256-byte boundary.  The partials are those of whichever
// call runs: the product's row and column partials ((n/4096 + n/64) n doubles), or the
// diagonal pass's sums and counts (n/64 n doubles and ints).
struct ProductScratch {
    DevBuf buf;
    int64_t n = -1;               // the size the work lists were built for
    int n_items = 0, n_diag = 0;
    int64_t nrb() const { return (n + kSvRows - 1) / kSvRows; }
    int64_t nseg() const { return (n + kSvSeg - 1) / kSvSeg; }
    const int2 *items() const { return (const int2 *)buf.p; }
    const int2 *diag() const { return (const int2 *)((char *)buf.p + align256(n_items * sizeof(int2))); }
    void *part() const { return (char *)diag() + align256(n_diag * sizeof(int2)); }

    // Made on first use and whenever n has changed (filter): the lists go to the device on
    // `stream`, which is then synchronised (they die with this scope).
    hipError_t prepare(int64_t size, bool with_diag, hipStream_t stream) {
        if (n == size) return hipSuccess;
        n = -1;
        const std::vector<int2> it = symv_items(size), dg = with_diag ? diag_items(size) : std::vector<int2>();
        const size_t rb = (size_t)((size + kSvRows - 1) / kSvRows), sg = (size_t)((size + kSvSeg - 1) / kSvSeg);
        const size_t part_bytes = std::max((sg + rb) * (size_t)size * 8, with_diag ? rb * (size_t)size * 12 : 0);
        const size_t ib = align256(it.size() * sizeof(int2)), db = align256(dg.size() * sizeof(int2));
        hipError_t e = buf.reserve(ib + db + part_bytes);
        if (e == hipSuccess)
            e = hipMemcpyAsync(buf.p, it.data(), it.size() * sizeof(int2), hipMemcpyHostToDevice, stream);
        if (e == hipSuccess && !dg.empty())
            e = hipMemcpyAsync((char *)buf.p + ib, dg.data(), dg.size() * sizeof(int2), hipMemcpyHostToDevice,
                               stream);
        if (e == hipSuccess) e = hipStreamSynchronize(stream);
        if (e != hipSuccess) return e;
        n_items = (int)it.size();
        n_diag = (int)dg.size();
        n = size;
        return hipSuccess;
    }
};

// y[c] = sum of c's row partials (segments c / 4096 ..) + its column partials (row blocks
// 0 .. c / 64), each list in order, cut into 8 slices that are added in slice order.
static __global__ __launch_bounds__(1024) void symv_reduce_kernel(const double *__restrict__ rowpart,
                                                           const double *__restrict__ colpart,
                                                           int64_t d, int nseg, double *__restrict__ y) {
    __shared__ double meet[8][128];
    const int el = threadIdx.x & 127, sl = threadIdx.x >> 7;
    const int64_t c = (int64_t)blockIdx.x * 128 + el;
    double acc = 0.0;
    if (c < d) {
        const int64_t s0 = c / kSvSeg, nrow = nseg - s0, ncol = c / kSvRows + 1, n = nrow + ncol;
        const int64_t per = (n + 7) / 8, k0 = sl * per, k1 = std::min<int64_t>(n, k0 + per);
        for (int64_t k = k0; k < k1; k += 16) {
            double v[16];
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int64_t kk = k + q;
                v[q] = kk >= k1 ? 0.0
                                : (kk < nrow ? rowpart[(s0 + kk) * d + c] : colpart[(kk - nrow) * d + c]);
            }
#pragma unroll
            for (int q = 0; q < 16; ++q) acc += v[q];
        }
    }
    meet[sl][el] = acc;
    __syncthreads();
    if (sl == 0 && c < d) {
        double t = meet[0][el];
#pragma unroll
        for (int q = 1; q < 8; ++q) t += meet[q][el];
        y[c] = t;
    }
}

// y = the product over a prepared scratch, enqueued on `stream`: `launch_product(grid, items,
// rowpart, colpart)` launches either product kernel, symv_reduce_kernel adds its partials.
template <typename LaunchProduct>
hipError_t product_enqueue(const ProductScratch &sc, hipStream_t stream, double *y,
                           LaunchProduct launch_product) {
    double *rowpart = (double *)sc.part(), *colpart = rowpart + sc.nseg() * sc.n;
    hipError_t e = launch_product(dim3((unsigned)sc.n_items), sc.items(), rowpart, colpart);
    if (e == hipSuccess)
        e = launch(symv_reduce_kernel, dim3((unsigned)((sc.n + 127) / 128)), dim3(1024), 0, stream,
                   (const double *)rowpart, (const double *)colpart, sc.n, (int)sc.nseg(), y);
    return e;
}

// ---- everything else the ContactMap side shares ------------------------------------------------
// ONE grow-only allocation per DEVICE for matrix-sized temporaries, shared by every map on it
// (per_device<CmScratch>; its stream is not used: the work runs on the handle's): the first
// touch of a fresh matrix-sized allocation costs 0.2-0.35 s on this platform.
// bb_cm_release_scratch gives it back.
struct CmScratch : DeviceScratch {};

// Sum of one value per thread of an N-thread workgroup through sh[N]: a binary tree in a fixed
// order (thread t adds t + N/2, then t + N/4, ...); every thread gets the total.  No barrier in
// front: a caller that sums twice through one sh puts a __syncthreads() between the two (the
// total of the first is still being read).
template <int N, typename T>
__device__ __forceinline__ T block_sum(T v, T *sh) {
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int off = N / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) sh[threadIdx.x] += sh[threadIdx.x + off];
        __syncthreads();
    }
    return sh[0];
}

}  // namespace bb

struct bb_cm {
    int device = 0;
    int64_t d = 0;            // current edge (shrinks in filter)
    double *m = nullptr;      // (d, d) row-major, resident
    hipStream_t stream = nullptr;
    // the scratch of the symmetric product, made by the first call that needs it and kept with
    // the handle: one for the edge d (symv, eigenvector) and one for the leading n_bins = d - 1
    // rows and columns (bb_cm_balance / bb_cm_expected), which also holds the diagonal work
    // list.  Two, so that alternating calls do not rebuild the lists.
    bb::ProductScratch sv, bal;
    double coarsen_ms = 0.0;  // on a map bb_cm_coarsen wrote: the pooling kernel, by HIP events
    double insulation_ms = 0.0;  // the kernel of the last bb_cm_insulation on this map, by HIP events
};

namespace bb {

// Entry of every call on a handle: it is there, and its device is selected.
inline int cm_check(const bb_cm *cm, const char *who) {
    if (!cm) return fail(BB_ERR_INVALID, std::string(who) + ": contact map is NULL");
    return enter_device(cm->device);
}

// The calls that work on the leading n_bins rows and columns: the map has not been filtered.
inline int cm_check_bins(const bb_cm *cm, int64_t n_bins, const char *who) {
    if (!(n_bins >= 0 && n_bins + 1 == cm->d))
        return fail(BB_ERR_INVALID,
                    std::string(who) + ": the matrix edge is not n_bins + 1 (filtered already?)");
    return BB_OK;
}

}  // namespace bb
