// bb_input_kernels.h -- device code of the input routes of the 3D-structure solver (gfx950
// only): every kernel that writes the units (staged rows, a device matrix, scattered entries,
// coordinates, the re-exponentiation), the row-owner path's full matrix built from them, and
// the tile census of a list of entries.  Included by bb_solver_inputs.hip and by nothing else:
// everything here lives in that translation unit's anonymous namespace.  The value rule of a
// stored wish distance: bb_wish.h.  Shapes: bb_solver_device.h.
#pragma once

#include "bb_solver_device.h"

namespace {

// --------------------------------------------------------------------------
// packing kernels
// --------------------------------------------------------------------------
// What becomes a stored wish distance -- flush_wish and wish_from_value -- is said in ONE
// place, bb_wish.h; the sweep's 0/1 weight depends on the flush (wish_floor).

// The cell walk of unit `dsc` = {i0, j0} by a workgroup of 256 threads: f(e, i, j, stored) for
// the cells e = r * VW + c of the thread, (i, j) = (i0 + r, j0 + c) its bin pair, stored =
// whether the cell holds a pair at all (upper triangle, inside the map).
template <typename T, bool W, typename F>
__device__ __forceinline__ void for_each_cell(int2 dsc, int64_t n_bins, F f) {
    constexpr int VW = Lay<T, W>::VW, RPU = Lay<T, W>::RPU;
    for (int e = threadIdx.x; e < RPU * VW; e += 256) {
        const int r = e / VW, c = e % VW;
        const int64_t i = (int64_t)dsc.x + r, j = (int64_t)dsc.y + c;
        f(e, i, j, j > i && j < n_bins);
    }
}

// staged fp64 rows (row-major, ld = VW) -> units of one run of tiles.
template <typename T, bool W>
__global__ __launch_bounds__(256) void convert_units_kernel(
    const double *__restrict__ stage, T *__restrict__ units_out, const int2 *__restrict__ udesc,
    int64_t ul0, int64_t stage_row0 /* global row of stage row 0 */, int64_t n_bins, int kind,
    double neg_inv_alpha) {
    constexpr int VW = Lay<T, W>::VW, RPU = Lay<T, W>::RPU;
    const int64_t ul = ul0 + blockIdx.x;
    const int2 dsc = udesc[ul];
    T *out = units_out + ul * (RPU * VW);
    for_each_cell<T, W>(dsc, n_bins, [&](int e, int64_t i, int64_t j, bool stored) {
        const double v = stored ? stage[(i - stage_row0) * VW + (j - dsc.y)] : 0.0;
        out[e] = wish_from_value<T>(v, kind, neg_inv_alpha);
    });
}

// A (d, d) float64 matrix that is ALREADY in HBM (a device-resident ContactMap,
// bb_cm_*) -> this rank's units, device to device: the same conversion as
// convert_units_kernel without the staging copy.  Only elements j > i are read.
template <typename T, bool W>
__global__ __launch_bounds__(256) void pack_units_from_matrix_kernel(
    const double *__restrict__ m, int64_t ld, T *__restrict__ units_out,
    const int2 *__restrict__ udesc, int64_t n_bins, int kind, double neg_inv_alpha, int64_t off) {
    // (off > 0: m is the matrix of the bins [off, n_bins) of a solver of several maps; units of
    // other maps are left alone)
    constexpr int VW = Lay<T, W>::VW, RPU = Lay<T, W>::RPU;
    const int64_t ul = blockIdx.x;
    const int2 dsc = udesc[ul];
    if (dsc.y < off || dsc.y >= n_bins || dsc.x < off) return;
    T *out = units_out + ul * (RPU * VW);
    for_each_cell<T, W>(dsc, n_bins, [&](int e, int64_t i, int64_t j, bool stored) {
        const double v = stored ? m[(i - off) * ld + (j - off)] : 0.0;
        out[e] = wish_from_value<T>(v, kind, neg_inv_alpha);
    });
}

// Sparse (i, j, value) entries -> resident units (blocked-sparse input).  The
// units were zeroed ("no constraint") first.  tilemap[I * n_blocks + J] is the
// tile's index in the global list or -1.
//
// A bin pair that occurs more than once keeps its LAST entry, as in the reference's
// scatter (`matrix[j*d+k] = ...` in file order, blueberry/datatypes.pyx:110-116) and
// in bb_contactmap_scatter.  Three passes over the entries, nothing the size of the
// matrix: `phase` 0 clears every cell an entry names, 1 records the highest entry
// index + 1 per cell (integer atomicMax on the cell's own bits, which the clear left
// at 0), 2 lets that entry alone store its value.
// Where the entries come from: (rows, cols, vals) arrays, or -- `tr` set -- the (n, 3) triples
// [pos_i, pos_j, count] of a Rao-format file as ContactMap.__init__ reads them
// (blueberry/datatypes.pyx:100-113), resident on the device: numpy.nan_to_num applied to each
// value as it is read (pyx:102), bin = (int)(pos / resolution) (pyx:111-112), element (t, c)
// at tr[t * st + c * sc] (row-major rows or the reference's column-major array).
struct EntrySrc {
    const int64_t *rows, *cols;
    const double *vals;
    const double *tr;
    int64_t st, sc;
    double resolution;
};
__device__ __forceinline__ double nan_to_num_f64(double v) {
    return v != v ? 0.0 : (v > 1.7976931348623157e308 ? 1.7976931348623157e308
                                                      : (v < -1.7976931348623157e308 ? -1.7976931348623157e308 : v));
}
// Entry k's bin pair, ordered i < j.  False: an entry to skip -- the diagonal, which carries no
// pair, or a bad one (a position outside what an int can hold, a bin outside the map), which
// sets *bad.
__device__ __forceinline__ bool entry_pair(const EntrySrc &src, int64_t k, int64_t n_bins, int64_t &i,
                                           int64_t &j, int *__restrict__ bad) {
    if (src.tr == nullptr) {
        i = src.rows[k]; j = src.cols[k];
    } else {
        const double qi = nan_to_num_f64(src.tr[k * src.st]) / src.resolution,
                     qj = nan_to_num_f64(src.tr[k * src.st + src.sc]) / src.resolution;
        if (!(qi > -2147483648.0 && qi < 2147483648.0 && qj > -2147483648.0 && qj < 2147483648.0)) {
            atomicExch(bad, 1);
            return false;
        }
        i = (int)qi; j = (int)qj;
    }
    if (i == j) return false;
    if (i > j) { const int64_t t = i; i = j; j = t; }
    if (i < 0 || j >= n_bins) { atomicExch(bad, 1); return false; }
    return true;
}

// Which tiles the entries name: present[I * n_blocks + J] = 1 (I <= J), so that the host can
// write down the tile list of a blocked-sparse solver without binning the entries itself.
__global__ __launch_bounds__(256) void entries_tiles_kernel(EntrySrc src, int64_t nnz, int64_t vw,
                                                            int64_t n_blocks, int64_t n_bins,
                                                            unsigned char *__restrict__ present,
                                                            int *__restrict__ bad) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= nnz) return;
    int64_t i, j;
    if (!entry_pair(src, k, n_bins, i, j, bad)) return;
    present[(i / vw) * n_blocks + j / vw] = 1;
}

template <typename T, bool W>
__global__ __launch_bounds__(256) void scatter_entries_kernel(
    EntrySrc src, int64_t nnz, const int32_t *__restrict__ tilemap,
    int64_t n_blocks, int64_t n_bins, int64_t u_begin, int64_t u_end, T *__restrict__ units,
    int kind, double neg_inv_alpha, const double *__restrict__ kr,
    const double *__restrict__ krexp, int *__restrict__ bad, int phase) {
    constexpr int VW = Lay<T, W>::VW, RPU = Lay<T, W>::RPU, UPT = VW / RPU;
    using Bits = typename std::conditional<sizeof(T) == 4, unsigned int, unsigned long long>::type;
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= nnz) return;
    int64_t i, j;
    if (!entry_pair(src, k, n_bins, i, j, bad)) return;
    const int64_t I = i / VW, J = j / VW;
    const int32_t t = tilemap[I * n_blocks + J];
    if (t < 0) { atomicExch(bad, 2); return; }   // entry outside the tile list
    const int64_t ri = i - I * VW;
    const int64_t u = (int64_t)t * UPT + ri / RPU;
    if (u < u_begin || u >= u_end) return;  // another rank's unit
    T *cell = units + (u - u_begin) * (RPU * VW) + (ri % RPU) * VW + (j - J * VW);
    // Entry k's mark: k + 1 under the sign bit.  Phase 2 stores wish distances into cells that
    // other threads of phase 2 are still comparing with their marks; a stored distance is 0 or
    // positive (wish_from_value), so it can equal no mark.  (A bare k + 1 is the bit pattern of
    // a float: from 228,737,632 entries in one chunk on, that of a distance >= wish_floor.)
    // k + 1 <= 2^30 (the callers' chunks), and the marks order as the entries do.
    const Bits mark = ((Bits)1 << (8 * sizeof(Bits) - 1)) | (Bits)(k + 1);
    if (phase == 0) {
        *reinterpret_cast<Bits *>(cell) = 0;
        return;
    }
    if (phase == 1) {
        atomicMax(reinterpret_cast<Bits *>(cell), mark);
        return;
    }
    if (*reinterpret_cast<const Bits *>(cell) != mark) return;   // a later entry won
    double v = src.tr ? nan_to_num_f64(src.tr[k * src.st + 2 * src.sc]) : src.vals[k];
    // KR balancing + observed/expected, the element-wise form of the loop at
    // reference datatypes.pyx:166-169 (same operation order)
    // (... followed by the reference's nan_to_num over the matrix, pyx:171: a NaN quotient is 0 =
    // no constraint, an overflowing one the largest double -- as ContactMap.normalize leaves it)
    if (kr != nullptr) v = nan_to_num_f64(v / (kr[i] * kr[j] * krexp[j - i]));
    *cell = wish_from_value<T>(v, kind, neg_inv_alpha);
}

// delta_ij = |x*_i - x*_j| generated in place (synthetic inputs).
template <typename T, bool W>
__global__ __launch_bounds__(256) void gen_units_kernel(const double *__restrict__ xs,
                                                        T *__restrict__ units_out,
                                                        const int2 *__restrict__ udesc,
                                                        int64_t n_bins) {
    constexpr int VW = Lay<T, W>::VW, RPU = Lay<T, W>::RPU;
    const int64_t ul = blockIdx.x;
    T *out = units_out + ul * (RPU * VW);
    for_each_cell<T, W>(udesc[ul], n_bins, [&](int e, int64_t i, int64_t j, bool stored) {
        double v = 0.0;
        if (stored) {
            const double dx = xs[3 * i] - xs[3 * j], dy = xs[3 * i + 1] - xs[3 * j + 1],
                         dz = xs[3 * i + 2] - xs[3 * j + 2];
            v = sqrt(dx * dx + dy * dy + dz * dz);
        }
        out[e] = flush_wish<T>(v);
    });
}

// SPEC 2.11: every stored word w > 0 of this rank's units becomes pow((double)w, p), taken as
// a kind='wish' input (the one value rule of bb_wish.h: floor, ceiling, rounding to T); zeros
// stay zeros.  n_words = n_local * (8 KiB / sizeof(T)); a grid-stride loop, one word per thread.
template <typename T>
__global__ __launch_bounds__(256) void repower_units_kernel(T *__restrict__ units, int64_t n_words,
                                                            double p) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n_words; e += stride) {
        const T w = units[e];
        if (w > T(0)) units[e] = wish_from_value<T>(pow((double)w, p), BB_KIND_WISH, 0.0);
    }
}

// resident units -> both triangles of the full matrix (zeroed first; one-off)
template <typename T, bool W>
__global__ __launch_bounds__(256) void units_to_full_kernel(const T *__restrict__ units,
                                                            const int2 *__restrict__ udesc,
                                                            T *__restrict__ full, int64_t ld,
                                                            int64_t n_bins) {
    constexpr int VW = Lay<T, W>::VW, RPU = Lay<T, W>::RPU;
    const int64_t ul = blockIdx.x;
    const T *in = units + ul * (RPU * VW);
    for_each_cell<T, W>(udesc[ul], n_bins, [&](int e, int64_t i, int64_t j, bool stored) {
        if (stored) {
            const T v = in[e];
            full[i * ld + j] = v;
            full[j * ld + i] = v;
        }
    });
}

}  // namespace
