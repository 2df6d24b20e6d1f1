// bb_sort.hip -- the scan and the sort of bb_sort.h, compiled here once.  gfx950 only.
//
// The sort is LSD radix, 8 bits per pass.  A pass moves every (key, value) to its place by one
// digit of the key and keeps the order of equal digits, so after the passes over all the key's
// bits equal KEYS are still in slot order.  A workgroup owns kSortTile consecutive slots:
// digit_hist_kernel counts its digits (integer LDS atomics), an exclusive scan of
// hist[digit][workgroup] -- digits outermost -- gives where each workgroup's run of each digit
// starts, and digit_scatter_kernel walks its tile in rounds of 256 consecutive slots: within a
// wave a slot's rank among the equal digits comes from ballots, across the 4 waves and the rounds
// from LDS counters.  (rocprim's radix sort is not used: its one-sweep kernel needs scratch
// memory, and no kernel of this library does.  Its scan is; no other file includes rocprim.)
#include <utility>

#include <rocprim/device/device_scan.hpp>

#include "bb_sort.h"

namespace bb {

constexpr int kSortRounds = 16, kSortTile = 256 * kSortRounds;

static __global__ __launch_bounds__(256) void digit_hist_kernel(const sort_key *__restrict__ keys, int64_t m,
                                                                int shift, int64_t n_wg,
                                                                sort_key *__restrict__ hist) {
    __shared__ unsigned h[256];
    h[threadIdx.x] = 0;
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * kSortTile;
    for (int r = 0; r < kSortRounds; ++r) {
        const int64_t i = base + r * 256 + threadIdx.x;
        if (i < m) atomicAdd(&h[(keys[i] >> shift) & 255], 1u);
    }
    __syncthreads();
    hist[(int64_t)threadIdx.x * n_wg + blockIdx.x] = h[threadIdx.x];
}

template <typename V>
__global__ __launch_bounds__(256) void digit_scatter_kernel(const sort_key *__restrict__ keys,
                                                            const V *__restrict__ vals, int64_t m, int shift,
                                                            int64_t n_wg, const sort_key *__restrict__ start,
                                                            sort_key *__restrict__ okeys,
                                                            V *__restrict__ ovals) {
    __shared__ sort_key run[256];                 // where the next slot of each digit goes
    __shared__ unsigned cnt[4][256];              // this round's slots per wave and digit
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    run[tid] = start[(int64_t)tid * n_wg + blockIdx.x];
    for (int w = 0; w < 4; ++w) cnt[w][tid] = 0;
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * kSortTile;
    for (int r = 0; r < kSortRounds; ++r) {       // (uniform: every thread meets every barrier)
        const int64_t i = base + r * 256 + tid;
        const bool in = i < m;
        const sort_key k = in ? keys[i] : 0;
        const int dg = (int)((k >> shift) & 255);
        sort_key peers = __ballot(in);            // the wave's slots with this slot's digit
        for (int b = 0; b < 8; ++b) {
            const bool bit = (dg >> b) & 1;
            const sort_key vote = __ballot(bit);
            peers &= bit ? vote : ~vote;
        }
        const unsigned rank = (unsigned)__popcll(peers & (((sort_key)1 << lane) - 1));
        if (in && rank == 0) cnt[wave][dg] = (unsigned)__popcll(peers);
        __syncthreads();
        if (in) {
            sort_key pos = run[dg] + rank;
            for (int w = 0; w < wave; ++w) pos += cnt[w][dg];
            okeys[pos] = k;
            ovals[pos] = vals[i];
        }
        __syncthreads();
        run[tid] += (sort_key)cnt[0][tid] + cnt[1][tid] + cnt[2][tid] + cnt[3][tid];
        for (int w = 0; w < 4; ++w) cnt[w][tid] = 0;
        __syncthreads();
    }
}

hipError_t exclusive_scan_bytes(size_t n, size_t *bytes) {
    *bytes = 0;                                   // (no temporary: rocprim only sizes, nothing is read or run)
    return rocprim::exclusive_scan(nullptr, *bytes, (const sort_key *)nullptr, (sort_key *)nullptr, (sort_key)0, n,
                                   rocprim::plus<sort_key>(), (hipStream_t) nullptr);
}

hipError_t exclusive_scan(void *tmp, size_t tmp_bytes, const sort_key *in, sort_key *out, size_t n,
                          hipStream_t st) {
    return rocprim::exclusive_scan(tmp, tmp_bytes, in, out, (sort_key)0, n, rocprim::plus<sort_key>(), st);
}

template <typename V>
hipError_t stable_sort_pairs(sort_key *&k, V *&v, sort_key *&k2, V *&v2, int64_t m, unsigned bits,
                             hipStream_t st) {
    const int64_t n_wg = (m + kSortTile - 1) / kSortTile;
    const size_t cells = (size_t)n_wg * 256;
    DevBuf hist, start, tmp;
    size_t scan_bytes = 0;
    hipError_t e = hist.alloc(cells * 8);
    if (e == hipSuccess) e = start.alloc(cells * 8);
    if (e == hipSuccess) e = exclusive_scan_bytes(cells, &scan_bytes);
    if (e == hipSuccess) e = tmp.alloc(scan_bytes);
    for (unsigned shift = 0; shift < bits && e == hipSuccess; shift += 8) {
        e = launch(digit_hist_kernel, dim3((unsigned)n_wg), dim3(256), 0, st, (const sort_key *)k, m, (int)shift,
                   n_wg, hist.as<sort_key>());
        if (e == hipSuccess)
            e = exclusive_scan(tmp.p, scan_bytes, hist.as<sort_key>(), start.as<sort_key>(), cells, st);
        if (e == hipSuccess)
            e = launch(digit_scatter_kernel<V>, dim3((unsigned)n_wg), dim3(256), 0, st, (const sort_key *)k,
                       (const V *)v, m, (int)shift, n_wg, (const sort_key *)start.p, k2, v2);
        if (e != hipSuccess) return e;
        std::swap(k, k2);
        std::swap(v, v2);
    }
    if (e != hipSuccess) return e;
    return hipStreamSynchronize(st);              // (hist, start and tmp die with this scope)
}
template hipError_t stable_sort_pairs<uint32_t>(sort_key *&, uint32_t *&, sort_key *&, uint32_t *&, int64_t,
                                                unsigned, hipStream_t);
template hipError_t stable_sort_pairs<double>(sort_key *&, double *&, sort_key *&, double *&, int64_t, unsigned,
                                              hipStream_t);

}  // namespace bb
