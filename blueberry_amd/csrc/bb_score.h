// bb_score.h -- what bb_solver_score (bb_solver_queries.hip: the handle and its state rules) hands
// to the scoring pass (bb_score.hip: the kernels and their launches).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bb {

// One rank's resident map and the coordinates to score, as views: nothing here is owned.
struct ScoreInput {
    int dtype = 0;                  // BB_F32 / BB_F64: the element type of the units
    bool wide = true;               // unit shape (bb::wide_layout)
    int64_t n_bins = 0, n_local = 0;
    const void *d_units = nullptr;  // n_local units of 8 KiB
    const int2 *d_udesc = nullptr;  // per local unit {i0, j0}, on the device ...
    const int2 *udesc = nullptr;    // ... and on the host
    const double *d_xyz = nullptr;  // (n_pad, 3) float64 coordinates on the device
    hipStream_t stream = nullptr;
};

// The sums of SPEC 2.8 over the input's units: profile (n_bins, 9) and bins (n_bins, 3), host
// float64.  ms (may be NULL): HIP-event times of the profile, fold and per-bin kernels.
int score_pass(const ScoreInput &in, double *profile, double *bins, double *ms);

// The log-log sums of SPEC 2.11 over the same pairs, by the same profile and fold kernels with
// seven columns: profile (n_bins, 7), host float64.  ms as above (the per-bin entry stays 0).
int loglog_pass(const ScoreInput &in, double *profile, double *ms);

}  // namespace bb
