// bb_cm_internal.h -- what the translation units that work on a resident ContactMap matrix
// share: the handle itself (bb_contactmap.hip owns its lifetime), the per-device grow-only
// scratch that holds matrix-sized temporaries (bb_cm_correlation, bb_cm_shortest_paths) and
// the workgroup sum of their fixed-order reductions, and the parts of the symmetric
// matrix-vector product that bb_contactmap.hip (symv, eigenvector) and bb_balance.hip (the
// banded product of the balancing iteration) both use: the tiling constants, the work list, the
// LDS-only barrier and the reduce kernel.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

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
    // the same for bb_cm_balance / bb_cm_expected (bb_balance.hip), which work on the leading
    // n_bins = d - 1 rows and columns: two work lists and the partial sums of either call
    bb::GrowBuf bal;
    int64_t bal_n = -1;       // the n_bins the work lists were built for
    int bal_items = 0, bal_diag_items = 0;
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

// ---- the symmetric product over the upper triangle (symv_upper_kernel, bb_contactmap.hip) ----
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


// The work list of a product over an n x n upper triangle: every (row block I, column segment S)
// that holds a cell on or above the diagonal.
inline std::vector<int2> symv_items(int64_t d) {
    const int64_t nrb = (d + kSvRows - 1) / kSvRows, nseg = (d + kSvSeg - 1) / kSvSeg;
    std::vector<int2> items;
    // longest items first: the dispatcher hands them out in order
    for (int64_t S = nseg - 1; S >= 0; --S)
        for (int64_t I = 0; I < nrb && I * kSvRows < (S + 1) * (int64_t)kSvSeg; ++I)
            if (std::max<int64_t>(I * kSvRows, S * kSvSeg) < std::min<int64_t>(d, (S + 1) * (int64_t)kSvSeg))
                items.push_back(make_int2((int)I, (int)S));
    std::stable_sort(items.begin(), items.end(), [&](const int2 &a, const int2 &b) {
        auto len = [&](const int2 &t) {
            return std::min<int64_t>(d, (t.y + 1) * (int64_t)kSvSeg) -
                   std::max<int64_t>((int64_t)t.x * kSvRows, (int64_t)t.y * kSvSeg);
        };
        return len(a) > len(b);
    });
    return items;
}

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

}  // namespace bb
