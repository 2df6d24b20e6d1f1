// bb_triples.h -- what the translation units that read Rao-format triples share: the resident
// handle (bb_solver_inputs.hip owns its lifetime), the two rules every reader applies to a triple's
// values -- numpy.nan_to_num and the binning of the ContactMap scatter -- and the canonical index
// bb_triples_balance.hip builds on the handle (docs/SPEC.md 2.5.3).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "bb_common.h"

namespace bb {

__device__ __forceinline__ double nan_to_num(double v) {
    // numpy.nan_to_num defaults: NaN -> 0, +/-inf -> +/-DBL_MAX
    if (v != v) return 0.0;
    if (v > 1.7976931348623157e308) return 1.7976931348623157e308;
    if (v < -1.7976931348623157e308) return -1.7976931348623157e308;
    return v;
}

// The two bins of a triple with the (nan_to_num'ed) positions pj, pk; false if one of them is
// outside [0, d).  (A position beyond the int range -- an infinity turned into 1.8e308 -- is
// out of range whatever the cast would make of it.)
__device__ __forceinline__ bool triple_bins(double pj, double pk, double resolution, int64_t d,
                                            int &j, int &k) {
    const double qj = pj / resolution, qk = pk / resolution;
    const bool wild = !(qj > -2147483648.0 && qj < 2147483648.0 && qk > -2147483648.0 && qk < 2147483648.0);
    j = wild ? -1 : (int)qj;
    k = wild ? -1 : (int)qk;
    return !(j < 0 || k < 0 || j >= d || k >= d);
}

// A list of (other index, value) entries grouped by an owner index, CSR style, and the cut of
// every owner's entries into segments of kTbSeg for the segmented sum (bb_triples_balance.hip):
// segment w belongs to owner seg_owner[w] and is the (w - seg_ptr[owner])-th of its entries.
constexpr int kTbSeg = 1024;   // entries of one owner (row or diagonal) that one wave works on
struct SegmentedList {
    int64_t n_entries = 0, n_seg = 0;
    DevBuf ptr;        // int64, owners + 1
    DevBuf other;      // int32 per entry
    DevBuf val;        // float64 per entry
    DevBuf seg_ptr;    // int64, owners + 1
    DevBuf seg_owner;  // int32 per segment
};

// The canonical index of the symmetric matrix the triples define over bins 0 .. n_bins - 1:
//   rows   row i -> (column, count) of every stored cell of row i, columns ascending: both
//          directions of every pair, the last triple of a pair the winner (12 B per entry)
//   diags  made by the first bb_triples_expected: diagonal k -> (row, count) of the stored upper
//          cells (row, row + k), rows ascending
struct TriplesIndex {
    int64_t n_bins = -1;          // the size it was built for; -1: none
    int64_t n_pairs = 0;          // distinct pairs i <= j < n_bins
    SegmentedList rows, diags;
    bool have_diags = false;
};

}  // namespace bb

struct bb_triples {
    int device = 0;
    int64_t n = 0, st = 3, sc = 1;      // element (t, c) at d[t * st + c * sc]
    double resolution = 1.0;
    bb::DevBuf d;                       // 3 n doubles
    bb::TriplesIndex index;             // (bb_triples_balance.hip; freed with the handle)
    double coarsen_ms = 0.0;            // on a list bb_triples_coarsen left: count + scan + write
                                        // over the source's index, by HIP events
    double insulation_ms = 0.0;         // the kernel of the last bb_triples_insulation, by HIP events
    const double *from(int64_t t0) const { return d.as<double>() + t0 * (st == 3 ? 3 : 1); }
};

// The geodesic rows bb_triples_paths leaves (bb_triples_paths.hip owns their lifetime); the solver
// reads them when it copies its anchors (bb_solver_set_anchors, docs/SPEC.md 2.5.5).
struct bb_paths {
    int device = 0;
    int64_t n_sources = 0, n_nodes = 0, ld = 0;   // ld: doubles per node in D
    int64_t sweeps = 0, unreachable = 0;
    double weights_ms = 0.0, sweeps_ms = 0.0;
    std::vector<int64_t> sources;                 // the node of every source
    bb::DevBuf D;                                 // float64 (n_nodes, ld): +inf where no path exists
};

namespace bb {
// The handle's index for n_bins, built if it is not there (bb_triples_balance.hip); `who` names
// the entry point in an error.
int triples_ensure_index(bb_triples *t, int64_t n_bins, const char *who);
}  // namespace bb
