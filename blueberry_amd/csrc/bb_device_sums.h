// bb_device_sums.h -- THE fixed-order sums over a wave and over the waves of a workgroup (device
// code, header only; 64 lanes).  All are one tree: lane i takes its partner at distance 32, then
// 16, ... down to 1; the waves' totals are then added left to right.  T: a float or integer type.
//
// The two wave forms give the same bits: after the first step every lane i < 32 holds
// v[i] + v[i + 32] in both (a + b = b + a bit for bit), and the later steps pair the same lanes, so
// lane 0 of wave_sum_first carries what every lane of wave_sum_all does.  Both stay because they
// compile to different instructions; a kernel uses the one it was measured with.  (The sweep's
// wave_sum_hi -- DPP, adjacent lanes first -- and bb::block_sum / lds_tree_fold are other trees.)
#pragma once

#include <hip/hip_runtime.h>

namespace bb {

// the total in lane 0 (the other lanes hold partial sums of no use)
template <typename T>
__device__ __forceinline__ T wave_sum_first(T v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// the total in every lane: the butterfly
template <typename T>
__device__ __forceinline__ T wave_sum_all(T v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// sh[wave] = the wave's sum of v, written by lane 0.  The caller's barrier comes before a read of sh.
template <typename T, int WAVES>
__device__ __forceinline__ void wave_sum_to_lds(T v, T (&sh)[WAVES]) {
    v = wave_sum_first(v);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
}

// sh[q][wave] = the wave's sum of v[q], then the barrier
template <typename T, int Q, int WAVES>
__device__ __forceinline__ void wave_sums_to_lds(const T (&v)[Q], T (&sh)[Q][WAVES]) {
#pragma unroll
    for (int q = 0; q < Q; ++q) wave_sum_to_lds(v[q], sh[q]);
    __syncthreads();
}

// the waves' sums left to right: ((sh[0] + sh[1]) + sh[2]) + ...
template <typename T, int WAVES>
__device__ __forceinline__ T lds_wave_total(const T (&sh)[WAVES]) {
    T v = sh[0];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) v += sh[w];
    return v;
}

// v[q] = the workgroup's sum of v[q], in every thread; sh is free again on return
template <typename T, int Q, int WAVES>
__device__ __forceinline__ void block_sums_all(T (&v)[Q], T (&sh)[Q][WAVES]) {
    wave_sums_to_lds(v, sh);
#pragma unroll
    for (int q = 0; q < Q; ++q) v[q] = lds_wave_total(sh[q]);
    __syncthreads();
}

}  // namespace bb
