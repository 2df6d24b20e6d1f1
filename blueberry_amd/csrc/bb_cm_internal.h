// bb_cm_internal.h -- what the translation units that work on a resident ContactMap matrix
// share: the handle itself (bb_contactmap.hip owns its lifetime), the per-device grow-only
// scratch that holds matrix-sized temporaries (bb_cm_correlation, bb_cm_shortest_paths) and
// the workgroup sum of their fixed-order reductions.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "bb_common.h"

struct bb_cm {
    int device = 0;
    int64_t d = 0;            // current edge (shrinks in filter)
    double *m = nullptr;      // (d, d) row-major, resident
    hipStream_t stream = nullptr;
    // grow-only scratch of the symmetric matrix-vector product (symv_upper_kernel): the work
    // list and the row / column partial sums; made by the first product, kept with the handle
    bb::GrowBuf sv;
    int64_t sv_d = -1;        // the edge the work list was built for
    int sv_items = 0;
};

namespace bb {

// ONE grow-only allocation per DEVICE for matrix-sized temporaries, shared by every map on it
// (per_device<CmScratch>; its stream is not used: the work runs on the handle's): the first
// touch of a fresh matrix-sized allocation costs 0.2-0.35 s on this platform.
// bb_cm_release_scratch gives it back.
struct CmScratch : DeviceScratch {};

// Sum of one value per thread of a 256-thread workgroup through sh[256]: a binary tree in a
// fixed order (thread t adds t + 128, then t + 64, ...); every thread gets the total.
template <typename T>
__device__ __forceinline__ T block_sum_256(T v, T *sh) {
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) sh[threadIdx.x] += sh[threadIdx.x + off];
        __syncthreads();
    }
    return sh[0];
}

}  // namespace bb
