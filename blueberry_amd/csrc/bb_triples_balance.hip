// bb_triples_balance.hip -- balancing without the dense matrix (docs/SPEC.md 2.5.3): the ICE bias
// vector and the distance-decay expected of the matrix that resident triples DEFINE (what
// ContactMap.from_triples would hold), computed from a canonical index of its stored cells.
//
//   the index   every triple with both bins below n_bins emits its directed entries (a, b) and
//               (b, a) -- one if a == b -- into slots 2 t and 2 t + 1, keyed a n_bins + b; a
//               triple that emits nothing leaves the slot's key above every real one.  A STABLE
//               radix sort by key (bb_sort.h) keeps equal keys in triple order, so the LAST entry
//               of a run of equal keys is the winner of its cell; the winners are compacted
//               into a CSR of the symmetric matrix: row_ptr (int64), col (int32), val
//               (float64), 12 B per directed entry.  Keys are 64 bits: n_bins^2 passes 2^32 at
//               n_bins = 65,536.  A row holds at most n_bins < 2^31 entries (its columns are
//               distinct), so a row's length always fits 31 bits; row_ptr is 64 bits.
//               Memory: 12 B per directed entry resident (at most 24 B per triple); while it
//               is built, 2 slots x (8 B key + 8 B value) x 2 (the sort's two buffers) = 64 B
//               per triple plus the sort's counters (1 B per slot), all given back before the call
//               returns.  An allocation that fails is BB_ERR_NOMEM; nothing half-built is
//               kept (the index is assembled aside and moved into the handle when complete).
//   seg_sum_kernel   the hot path: y_i = sum of row i's counted entries val_k x[col_k].  Rows
//               are badly skewed (a live bin of a whole-genome map has thousands of entries, a
//               dead one none), so a wave gets a SEGMENT of at most kTbSeg entries of one row,
//               not a row: lane l adds entries l, l + 64, ... of the segment in order (4-byte
//               col and 8-byte val loads, both coalesced; x through L2), the 64 lanes meet in
//               a fixed shuffle tree, one partial per segment in its own slot.
//               seg_reduce_kernel adds a row's partials in segment order.  kTbSeg and the
//               lane-to-entry mapping are constants of the build: the bits are a function of
//               the index and n_bins alone.  Three cell rules and the band test where the
//               products are formed, as band_symv_kernel (bb_balance.hip).
//   the loop    bb::balance_loop (bb_balance_loop.h): bb_cm_balance's, with this product.
//   expected    counts[k] from the live bins alone: the 0/1 live vector packed into 64-bit
//               words, counts[k] = sum_w popcount(L[w] & (L >> k)[w]) -- exact, and pairs
//               without a triple count, as the dense definition counts zero cells.  sums[k]
//               over a second, diagonal-major ordering of the stored upper entries (key
//               (col - row) n_bins + row, made on the first call), summed by the same two
//               kernels with the diagonal in the row's place.
// Float64, no floating-point atomics, every order fixed by the index: the same bits on every
// run, and for every triple list that defines the same matrix without duplicates (SPEC 2.7).
#include <float.h>
#include <math.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "bb_balance_loop.h"
#include "bb_cm_internal.h"
#include "bb_common.h"
#include "bb_sort.h"
#include "bb_triples.h"

namespace {

using bb::kCellBad;
using bb::kCellNonzero;
using bb::kCellValue;
using bb::SegmentedList;
using bb::stable_sort_pairs;   // the stable radix sort (bb_sort.h), here with double payloads
using bb::TriplesIndex;

using bb::kTbSeg;   // entries of one owner (row or diagonal) that one wave sums
// the two further rules of the diagonal sums: weights x_row x_{row + k}, or all weights 1
enum { kDiagWeighted = 3, kDiagPlain = 4 };

typedef unsigned long long u64;

// ---- building the index -----------------------------------------------------------------------
// flags[0]: a bin outside [0, n_bins]
__global__ __launch_bounds__(256) void emit_kernel(const double *__restrict__ tr, int64_t n, int64_t st,
                                                   int64_t sc, double resolution, int64_t n_bins,
                                                   u64 none, u64 *__restrict__ keys,
                                                   double *__restrict__ vals, int *__restrict__ flags) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    int j, k;
    u64 k0 = none, k1 = none;
    double c = 0.0;
    if (!bb::triple_bins(bb::nan_to_num(tr[t * st]), bb::nan_to_num(tr[t * st + sc]), resolution,
                         n_bins + 1, j, k)) {
        flags[0] = 1;
    } else if (j < n_bins && k < n_bins) {       // (a pair that touches bin n_bins is never read)
        c = bb::nan_to_num(tr[t * st + 2 * sc]);
        k0 = (u64)j * (u64)n_bins + (u64)k;
        if (j != k) k1 = (u64)k * (u64)n_bins + (u64)j;
    }
    keys[2 * t] = k0;
    keys[2 * t + 1] = k1;
    vals[2 * t] = c;
    vals[2 * t + 1] = c;
}

// keep[i] = 1 for the last entry of every run of equal real keys
__global__ __launch_bounds__(256) void winners_kernel(const u64 *__restrict__ keys, int64_t m, u64 none,
                                                      u64 *__restrict__ keep) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    const u64 k = keys[i];
    keep[i] = (k != none && (i + 1 == m || keys[i + 1] != k)) ? 1 : 0;
}

// the winners to their places: other = key % n_bins, and the key itself for the pointer search.
// `upper` counts the entries with other >= owner (key / n_bins), one integer atomic per wave.
__global__ __launch_bounds__(256) void compact_kernel(const u64 *__restrict__ keys,
                                                      const double *__restrict__ vals, int64_t m,
                                                      u64 none, const u64 *__restrict__ pos, u64 n_bins,
                                                      u64 *__restrict__ ckeys, int *__restrict__ other,
                                                      double *__restrict__ val, u64 *__restrict__ upper) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool up = false;
    if (i < m) {
        const u64 k = keys[i];
        if (k != none && (i + 1 == m || keys[i + 1] != k)) {
            const u64 p = pos[i], a = k / n_bins, b = k - a * n_bins;
            ckeys[p] = k;
            other[p] = (int)b;
            val[p] = vals[i];
            up = b >= a;
        }
    }
    const u64 votes = __ballot(up);
    if ((threadIdx.x & 63) == 0 && votes != 0) atomicAdd(upper, (u64)__popcll(votes));
}

// ptr[r] = the number of entries with owner < r = the first entry whose key is >= r n_bins
__global__ __launch_bounds__(256) void pointers_kernel(const u64 *__restrict__ ckeys, int64_t nnz,
                                                       int64_t owners, u64 n_bins,
                                                       long long *__restrict__ ptr) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r > owners) return;
    const u64 want = (u64)r * n_bins;
    int64_t lo = 0, hi = nnz;
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (ckeys[mid] < want) lo = mid + 1; else hi = mid;
    }
    ptr[r] = lo;
}

// the diagonal-major key of every stored upper entry of the CSR, `none` for a lower one
__global__ __launch_bounds__(256) void diag_keys_kernel(const long long *__restrict__ row_ptr,
                                                        const int *__restrict__ col,
                                                        const double *__restrict__ val, int64_t nnz,
                                                        int64_t n_bins, u64 none, u64 *__restrict__ keys,
                                                        double *__restrict__ vals) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= nnz) return;
    int64_t lo = 0, hi = n_bins;                 // the row of entry p: the last r with row_ptr[r] <= p
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo + 1) / 2;
        if (row_ptr[mid] <= p) lo = mid; else hi = mid - 1;
    }
    const int64_t row = lo, c = col[p];
    keys[p] = c >= row ? (u64)(c - row) * (u64)n_bins + (u64)row : none;
    vals[p] = val[p];
}

// ---- the segmented sum: the product, and the diagonal sums ------------------------------------
// Segment w of owner o = seg_owner[w]: entries ptr[o] + s kTbSeg .. of o, s = w - seg_ptr[o].
// One wave per segment, 4 per workgroup.  MODE:
//   kCellValue / kCellNonzero / kCellBad   o is a row, other its column; a cell counts when
//       |o - other| >= ignore (selected, never multiplied by 0); kCellBad sees the upper entries
//       alone, so that sum(y) is the number of offending cells
//   kDiagWeighted / kDiagPlain             o is a diagonal k, other the row: val x_row x_{row+k}
//       over the pairs whose weight is not 0 / the plain sum
template <int MODE>
__global__ __launch_bounds__(256) void seg_sum_kernel(const long long *__restrict__ ptr,
                                                      const int *__restrict__ other,
                                                      const double *__restrict__ val,
                                                      const long long *__restrict__ seg_ptr,
                                                      const int *__restrict__ seg_owner, int64_t n_seg,
                                                      int64_t ignore, const double *__restrict__ x,
                                                      double *__restrict__ part,
                                                      const int *__restrict__ stop) {
    if (stop != nullptr && *stop != 0) return;
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= n_seg) return;                       // (whole waves: no barrier follows)
    const int64_t o = seg_owner[w];
    const int64_t begin = ptr[o] + (w - seg_ptr[o]) * kTbSeg;
    const int64_t end = std::min<int64_t>(ptr[o + 1], begin + kTbSeg);
    double acc = 0.0;
    for (int64_t e0 = begin; e0 < end; e0 += 64 * 4) {
        int c[4];
        double v[4], xc[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int64_t e = e0 + 64 * q + lane;
            const bool in = e < end;
            c[q] = in ? other[e] : -1;
            v[q] = in ? val[e] : 0.0;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (MODE == kCellValue) xc[q] = c[q] >= 0 ? x[c[q]] : 0.0;
            else if (MODE == kDiagWeighted) xc[q] = c[q] >= 0 ? x[c[q]] * x[c[q] + o] : 0.0;
            else xc[q] = 0.0;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (MODE == kDiagWeighted) {
                acc = xc[q] != 0.0 ? fma(v[q], xc[q], acc) : acc;
            } else if (MODE == kDiagPlain) {
                acc += v[q];                      // (outside the segment v is 0)
            } else {
                const int64_t sep = c[q] >= o ? c[q] - o : o - c[q];
                const bool on = c[q] >= 0 && sep >= ignore;
                if (MODE == kCellValue) acc = fma(on ? v[q] : 0.0, xc[q], acc);
                else if (MODE == kCellNonzero) acc += (on && v[q] != 0.0) ? 1.0 : 0.0;
                else acc += (on && c[q] >= o && !(v[q] >= 0.0 && v[q] <= DBL_MAX)) ? 1.0 : 0.0;
            }
        }
    }
    acc = bb::wave_sum_first(acc);
    if (lane == 0) part[w] = acc;
}

// y[o] = the partials of o's segments, in segment order (0 for an owner without entries)
__global__ __launch_bounds__(256) void seg_reduce_kernel(const double *__restrict__ part,
                                                         const long long *__restrict__ seg_ptr,
                                                         int64_t owners, double *__restrict__ y,
                                                         const int *__restrict__ stop) {
    if (stop != nullptr && *stop != 0) return;
    const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (o >= owners) return;
    double acc = 0.0;
    for (int64_t w = seg_ptr[o]; w < seg_ptr[o + 1]; ++w) acc += part[w];
    y[o] = acc;
}

// ---- the expected's counts ---------------------------------------------------------------------
// L[w] bit i = bin 64 w + i is live (x != 0; x == NULL: every bin below n); words up to n_words
// are written, those past the last bin 0
__global__ __launch_bounds__(256) void pack_live_kernel(const double *__restrict__ x, int64_t n,
                                                        int64_t n_words, u64 *__restrict__ L) {
    const int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (w >= n_words) return;
    u64 bits = 0;
    for (int i = 0; i < 64; ++i) {
        const int64_t b = w * 64 + i;
        if (b < n && (x == nullptr || x[b] != 0.0)) bits |= (u64)1 << i;
    }
    L[w] = bits;
}

// counts[k] = sum_w popcount(L[w] & (L >> k)[w]); one wave per k.  L has two zero words beyond
// the (n + 63) / 64 that hold bins.
__global__ __launch_bounds__(256) void pair_counts_kernel(const u64 *__restrict__ L, int64_t n,
                                                          long long *__restrict__ counts) {
    const int lane = threadIdx.x & 63;
    const int64_t k = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (k >= n) return;
    const int64_t q = k >> 6, words = (n - k + 63) >> 6;     // bins i < n - k
    const int r = (int)(k & 63);
    long long acc = 0;
    for (int64_t w = lane; w < words; w += 64) {
        const u64 lo = L[w + q], hi = L[w + q + 1];
        const u64 shifted = r == 0 ? lo : (lo >> r) | (hi << (64 - r));
        acc += __popcll(L[w] & shifted);
    }
    acc = bb::wave_sum_first(acc);
    if (lane == 0) counts[k] = acc;
}

// ---- host side ---------------------------------------------------------------------------------
#define TB_HIP(expr)                             \
    do {                                         \
        const hipError_t _e = (expr);            \
        if (_e != hipSuccess) return _e;         \
    } while (0)

inline dim3 grid256(int64_t n) { return dim3((unsigned)((std::max<int64_t>(n, 1) + 255) / 256)); }

// keys / vals (m slots; `none` marks an empty one) -> list: sort, keep the last of equal keys,
// pointers for `owners` owners of key / n_bins.  `upper` (may be NULL): the entries with
// other >= owner.  Ends synchronised; the inputs are consumed.
hipError_t build_list(bb::DevBuf &keys, bb::DevBuf &vals, int64_t m, u64 none, unsigned key_bits,
                      int64_t owners, int64_t n_bins, SegmentedList *out, int64_t *upper) {
    hipStream_t st = nullptr;
    bb::DevBuf keys2, vals2, tmp, pos, cnt;
    int64_t nnz = 0;
    TB_HIP(cnt.alloc(16));
    TB_HIP(hipMemsetAsync(cnt.p, 0, 16, st));
    const u64 *sorted_keys = nullptr, *places = nullptr;
    const double *sorted_vals = nullptr;
    if (m > 0) {
        TB_HIP(keys2.alloc((size_t)m * 8));
        TB_HIP(vals2.alloc((size_t)m * 8));
        u64 *sk = keys.as<u64>(), *fk = keys2.as<u64>();
        double *sv = vals.as<double>(), *fv = vals2.as<double>();
        TB_HIP(stable_sort_pairs(sk, sv, fk, fv, m, key_bits, st));
        // the free pair of buffers now holds the winners' marks and their places
        u64 *keep = fk, *place = (u64 *)fv;
        TB_HIP(bb::launch(winners_kernel, grid256(m), dim3(256), 0, st, (const u64 *)sk, m, none, keep));
        size_t scan_bytes = 0;
        TB_HIP(bb::exclusive_scan_bytes((size_t)m, &scan_bytes));
        TB_HIP(tmp.reserve(scan_bytes));
        TB_HIP(bb::exclusive_scan(tmp.p, scan_bytes, keep, place, (size_t)m, st));
        u64 last_place = 0, last_keep = 0;
        TB_HIP(hipStreamSynchronize(st));
        TB_HIP(hipMemcpy(&last_place, place + (m - 1), 8, hipMemcpyDeviceToHost));
        TB_HIP(hipMemcpy(&last_keep, keep + (m - 1), 8, hipMemcpyDeviceToHost));
        nnz = (int64_t)(last_place + last_keep);
        sorted_keys = sk;
        sorted_vals = sv;
        places = place;
    }
    out->n_entries = nnz;
    bb::DevBuf ckeys;
    TB_HIP(ckeys.alloc((size_t)nnz * 8));
    TB_HIP(out->other.alloc((size_t)nnz * 4));
    TB_HIP(out->val.alloc((size_t)nnz * 8));
    TB_HIP(out->ptr.alloc((size_t)(owners + 1) * 8));
    if (m > 0)
        TB_HIP(bb::launch(compact_kernel, grid256(m), dim3(256), 0, st, sorted_keys, sorted_vals,
                          m, none, places, (u64)n_bins, ckeys.as<u64>(), out->other.as<int>(),
                          out->val.as<double>(), cnt.as<u64>()));
    TB_HIP(bb::launch(pointers_kernel, grid256(owners + 1), dim3(256), 0, st, (const u64 *)ckeys.p, nnz,
                      owners, (u64)n_bins, out->ptr.as<long long>()));
    // the cut into segments, on the host: owners + 1 pointers down, as many and one int per
    // segment up (set-up; 2.4 MB each way at 309,568 bins)
    std::vector<long long> ptr((size_t)owners + 1), seg_ptr((size_t)owners + 1);
    TB_HIP(hipStreamSynchronize(st));
    TB_HIP(hipMemcpy(ptr.data(), out->ptr.p, ptr.size() * 8, hipMemcpyDeviceToHost));
    if (upper != nullptr) {
        u64 up = 0;
        TB_HIP(hipMemcpy(&up, cnt.p, 8, hipMemcpyDeviceToHost));
        *upper = (int64_t)up;
    }
    std::vector<int> seg_owner;
    seg_ptr[0] = 0;
    for (int64_t o = 0; o < owners; ++o) {
        const long long segs = (ptr[(size_t)o + 1] - ptr[(size_t)o] + kTbSeg - 1) / kTbSeg;
        seg_ptr[(size_t)o + 1] = seg_ptr[(size_t)o] + segs;
        seg_owner.insert(seg_owner.end(), (size_t)segs, (int)o);
    }
    out->n_seg = seg_ptr[(size_t)owners];
    TB_HIP(out->seg_ptr.alloc(seg_ptr.size() * 8));
    TB_HIP(out->seg_owner.alloc(seg_owner.size() * 4));
    TB_HIP(hipMemcpy(out->seg_ptr.p, seg_ptr.data(), seg_ptr.size() * 8, hipMemcpyHostToDevice));
    if (!seg_owner.empty())
        TB_HIP(hipMemcpy(out->seg_owner.p, seg_owner.data(), seg_owner.size() * 4, hipMemcpyHostToDevice));
    return hipSuccess;
}

// the smallest number of bits that hold every value below `bound`
unsigned bits_below(u64 bound) {
    unsigned b = 1;
    while (b < 64 && ((u64)1 << b) < bound) ++b;
    return b;
}

}  // namespace

// The handle's index for n_bins, built if it is not there.
int bb::triples_ensure_index(bb_triples *t, int64_t n_bins, const char *who) {
    BB_REQUIRE(t != nullptr, std::string(who) + ": triples is NULL");
    BB_REQUIRE(n_bins >= 0 && n_bins < 2147483647, std::string(who) + ": n_bins is out of range");
    BB_TRY(bb::enter_device(t->device));
    if (t->index.n_bins == n_bins) return BB_OK;
    t->index = TriplesIndex();                    // (another size's index goes first: its memory)
    TriplesIndex ix;
    const int64_t m = 2 * t->n;
    // real keys are below n_bins^2 <= 2^62; an empty slot's key is the next power of two
    const unsigned real_bits = bits_below((u64)std::max<int64_t>(n_bins, 1) * (u64)std::max<int64_t>(n_bins, 1));
    const u64 none = (u64)1 << real_bits;
    bb::DevBuf keys, vals, flags;
    hipError_t e = keys.alloc((size_t)m * 8);
    if (e == hipSuccess) e = vals.alloc((size_t)m * 8);
    if (e == hipSuccess) e = flags.alloc(sizeof(int));
    BB_TRY(bb::hip_status(who, e, BB_ERR_NOMEM));
    int bad = 0;
    e = hipMemsetAsync(flags.p, 0, sizeof(int), nullptr);
    if (e == hipSuccess && t->n > 0)
        e = bb::launch(emit_kernel, grid256(t->n), dim3(256), 0, (hipStream_t) nullptr, t->from(0), t->n,
                       t->st, t->sc, t->resolution, n_bins, none, keys.as<u64>(), vals.as<double>(),
                       flags.as<int>());
    if (e == hipSuccess) e = hipMemcpy(&bad, flags.p, sizeof(int), hipMemcpyDeviceToHost);
    BB_TRY(bb::hip_status(who, e));
    if (bad)
        return bb::fail(BB_ERR_INVALID, std::string(who) + ": a position maps to a bin outside [0, n_bins]");
    int64_t upper = 0;
    e = build_list(keys, vals, m, none, real_bits + 1, n_bins, n_bins, &ix.rows, &upper);
    if (e == hipErrorOutOfMemory) return bb::hip_status(who, e, BB_ERR_NOMEM);
    BB_TRY(bb::hip_status(who, e));
    ix.n_pairs = upper;
    ix.n_bins = n_bins;
    t->index = std::move(ix);
    return BB_OK;
}

namespace {

// The diagonal-major ordering of the stored upper entries, made on first use.
int ensure_diags(bb_triples *t, const char *who) {
    TriplesIndex &ix = t->index;
    if (ix.have_diags) return BB_OK;
    const int64_t n = ix.n_bins, nnz = ix.rows.n_entries;
    const unsigned real_bits = bits_below((u64)std::max<int64_t>(n, 1) * (u64)std::max<int64_t>(n, 1));
    const u64 none = (u64)1 << real_bits;
    bb::DevBuf keys, vals;
    hipError_t e = keys.alloc((size_t)nnz * 8);
    if (e == hipSuccess) e = vals.alloc((size_t)nnz * 8);
    BB_TRY(bb::hip_status(who, e, BB_ERR_NOMEM));
    if (nnz > 0)
        e = bb::launch(diag_keys_kernel, grid256(nnz), dim3(256), 0, (hipStream_t) nullptr,
                       (const long long *)ix.rows.ptr.p, (const int *)ix.rows.other.p,
                       (const double *)ix.rows.val.p, nnz, n, none, keys.as<u64>(), vals.as<double>());
    SegmentedList diags;
    if (e == hipSuccess) e = build_list(keys, vals, nnz, none, real_bits + 1, n, n, &diags, nullptr);
    if (e == hipErrorOutOfMemory) return bb::hip_status(who, e, BB_ERR_NOMEM);
    BB_TRY(bb::hip_status(who, e));
    ix.diags = std::move(diags);
    ix.have_diags = true;
    return BB_OK;
}

// y[o] = the segmented sum of `list` under MODE, enqueued on the null stream
template <int MODE>
hipError_t seg_sum_enqueue(const SegmentedList &list, int64_t owners, int64_t ignore, const double *x,
                           double *part, double *y, const int *stop) {
    hipStream_t st = nullptr;
    if (list.n_seg > 0)
        TB_HIP(bb::launch(seg_sum_kernel<MODE>, dim3((unsigned)((list.n_seg + 3) / 4)), dim3(256), 0, st,
                          (const long long *)list.ptr.p, (const int *)list.other.p,
                          (const double *)list.val.p, (const long long *)list.seg_ptr.p,
                          (const int *)list.seg_owner.p, list.n_seg, ignore, x, part, stop));
    return bb::launch(seg_reduce_kernel, grid256(owners), dim3(256), 0, st, (const double *)part,
                      (const long long *)list.seg_ptr.p, owners, y, stop);
}

}  // namespace

extern "C" {

int bb_triples_pairs(bb_triples *t, int64_t n_bins, int64_t *n_pairs) {
    BB_REQUIRE(n_pairs != nullptr, "bb_triples_pairs: NULL argument");
    BB_TRY(bb::triples_ensure_index(t, n_bins, "bb_triples_pairs"));
    *n_pairs = t->index.n_pairs;
    return BB_OK;
}

int bb_triples_balance(bb_triples *t, int64_t n_bins, int64_t ignore_diags, int64_t min_nnz, double tol,
                       int64_t max_iter, double row_sum, double *bias, uint8_t *masked,
                       int64_t *iterations, double *variance) {
    BB_REQUIRE(t != nullptr, "bb_triples_balance: triples is NULL");
    BB_TRY(bb::balance_check_args("bb_triples_balance", n_bins, ignore_diags, min_nnz, tol, max_iter,
                                  row_sum, bias, masked));
    BB_TRY(bb::triples_ensure_index(t, n_bins, "bb_triples_balance"));
    const int64_t n = n_bins;
    ignore_diags = std::min(ignore_diags, n);         // (beyond n - 1 nothing is counted anyway)
    const SegmentedList &rows = t->index.rows;
    bb::DevBuf part;
    BB_TRY(bb::hip_status("bb_triples_balance", part.alloc((size_t)rows.n_seg * 8), BB_ERR_NOMEM));
    double *p = part.as<double>();
    return bb::balance_loop(
        "bb_triples_balance", n, nullptr,
        [&](int mode, const double *x, double *y, const int *stop) {
            if (mode == kCellBad) return seg_sum_enqueue<kCellBad>(rows, n, ignore_diags, x, p, y, stop);
            if (mode == kCellNonzero) return seg_sum_enqueue<kCellNonzero>(rows, n, ignore_diags, x, p, y, stop);
            return seg_sum_enqueue<kCellValue>(rows, n, ignore_diags, x, p, y, stop);
        },
        min_nnz, tol, max_iter, row_sum, bias, masked, iterations, variance);
}

int bb_triples_expected(bb_triples *t, int64_t n_bins, const double *bias, double *sums, int64_t *counts) {
    BB_REQUIRE(t != nullptr, "bb_triples_expected: triples is NULL");
    BB_REQUIRE(sums != nullptr && counts != nullptr, "bb_triples_expected: NULL argument");
    BB_TRY(bb::triples_ensure_index(t, n_bins, "bb_triples_expected"));
    const int64_t n = n_bins;
    if (n == 0) return BB_OK;
    BB_TRY(ensure_diags(t, "bb_triples_expected"));
    const SegmentedList &diags = t->index.diags;
    const int64_t n_words = (n + 63) / 64 + 2;
    bb::DevBuf bx, bs, bc, bl, part;
    hipError_t e = bx.alloc((size_t)n * 8);
    if (e == hipSuccess) e = bs.alloc((size_t)n * 8);
    if (e == hipSuccess) e = bc.alloc((size_t)n * 8);
    if (e == hipSuccess) e = bl.alloc((size_t)n_words * 8);
    if (e == hipSuccess) e = part.alloc((size_t)diags.n_seg * 8);
    BB_TRY(bb::hip_status("bb_triples_expected", e, BB_ERR_NOMEM));
    hipStream_t st = nullptr;
    double *x = nullptr;
    if (bias != nullptr) {
        // (the sums vector doubles as the staging place of the bias)
        x = bx.as<double>();
        e = hipMemcpyAsync(bs.p, bias, (size_t)n * 8, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = bb::inverse_bias_enqueue((const double *)bs.p, x, n, st);
        if (e == hipSuccess)
            e = seg_sum_enqueue<kDiagWeighted>(diags, n, 0, x, part.as<double>(), bs.as<double>(), nullptr);
    } else {
        e = seg_sum_enqueue<kDiagPlain>(diags, n, 0, nullptr, part.as<double>(), bs.as<double>(), nullptr);
    }
    if (e == hipSuccess)
        e = bb::launch(pack_live_kernel, grid256(n_words), dim3(256), 0, st, (const double *)x, n, n_words,
                       bl.as<u64>());
    if (e == hipSuccess)
        e = bb::launch(pair_counts_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st,
                       (const u64 *)bl.p, n, bc.as<long long>());
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e == hipSuccess) e = hipMemcpy(sums, bs.p, (size_t)n * 8, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(counts, bc.p, (size_t)n * 8, hipMemcpyDeviceToHost);
    return bb::hip_status("bb_triples_expected", e);
}

}  // extern "C"
