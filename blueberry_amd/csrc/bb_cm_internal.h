// bb_cm_internal.h -- what the translation units that work on a resident ContactMap matrix
// share: the handle itself (bb_contactmap.hip owns its lifetime) and the per-device grow-only
// scratch that holds matrix-sized temporaries (bb_cm_correlation, bb_cm_shortest_paths).
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <mutex>

struct bb_cm {
    int device = 0;
    int64_t d = 0;            // current edge (shrinks in filter)
    double *m = nullptr;      // (d, d) row-major, resident
    hipStream_t stream = nullptr;
    // grow-only scratch of the symmetric matrix-vector product (symv_upper_kernel): the work
    // list and the row / column partial sums; made by the first product, kept with the handle
    void *sv_buf = nullptr;
    size_t sv_bytes = 0;
    int64_t sv_d = -1;        // the edge the work list was built for
    int sv_items = 0;
};

namespace bb {

// ONE grow-only allocation per DEVICE for matrix-sized temporaries, shared by every map on it
// and guarded by a mutex (calls on one device serialise, as bb_band.hip's context does): the
// first touch of a fresh matrix-sized allocation costs 0.2-0.35 s on this platform.
// bb_cm_release_scratch gives it back.
struct CorrScratch {
    std::mutex mu;
    void *buf = nullptr;
    size_t bytes = 0;
};
CorrScratch *corr_scratch(int device);   // never NULL; lives for the process

}  // namespace bb
