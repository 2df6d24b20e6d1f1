// bb_query_kernels.h -- device code of the solver's queries (gfx950 only): what is asked of the
// resident units once per map -- degrees, weighted degrees, the landmark rows' step sums -- and
// the read-only sweeps that measure the HBM read ceiling of the sweep's access pattern.
// Included by bb_solver_queries.hip and by nothing else: everything here lives in that
// translation unit's anonymous namespace.  Shapes, wave sums and the streaming loads:
// bb_solver_device.h.
#pragma once

#include "bb_solver_device.h"

namespace {

// Per bin: how many of this rank's stored pairs constrain it (delta > 0) -- the degrees a step
// per bin is made from (bb_solver_degrees; once per map, not per iteration).  A workgroup takes
// kDegUnits consecutive units: a row's count is a ballot per wave (one atomic per wave and
// row), a column's is kept by the thread that owns the column for as long as the units stay
// in one tile column (one atomic per column and run of units).
constexpr int kDegUnits = 32;
template <typename T, bool W>
__global__ __launch_bounds__(256) void unit_degrees_kernel(const T *__restrict__ units,
                                                           const int2 *__restrict__ udesc,
                                                           int64_t n_local, int64_t n_bins,
                                                           int *__restrict__ deg) {
    constexpr int VW = Lay<T, W>::VW, RPU = Lay<T, W>::RPU, CPT = (VW + 255) / 256;
    const int lane = threadIdx.x & 63;
    const int64_t u0 = (int64_t)blockIdx.x * kDegUnits;
    const int64_t u1 = u0 + kDegUnits < n_local ? u0 + kDegUnits : n_local;
    int col[CPT];
#pragma unroll
    for (int k = 0; k < CPT; ++k) col[k] = 0;
    int j0 = udesc[u0].y;
    auto flush = [&]() {
#pragma unroll
        for (int k = 0; k < CPT; ++k) {
            const int c = (int)threadIdx.x + 256 * k;
            if (c < VW && col[k] > 0) atomicAdd(deg + j0 + c, col[k]);
            col[k] = 0;
        }
    };
    for (int64_t ul = u0; ul < u1; ++ul) {
        const int2 dsc = udesc[ul];
        if (dsc.y != j0) {                              // (uniform: every thread reads the same word)
            flush();
            j0 = dsc.y;
        }
        const T *in = units + ul * (RPU * VW);
        for (int r = 0; r < RPU; ++r) {
            const int64_t i = (int64_t)dsc.x + r;
            int row = 0;
#pragma unroll
            for (int k = 0; k < CPT; ++k) {
                const int c = (int)threadIdx.x + 256 * k;
                const int64_t j = (int64_t)dsc.y + c;
                const bool on = c < VW && j > i && j < n_bins && in[r * VW + c] > T(0);
                col[k] += on ? 1 : 0;
                row += __popcll(__ballot(on));
            }
            if (lane == 0 && row > 0) atomicAdd(deg + i, row);
        }
    }
    flush();
}

// Per bin: s_i = sum_j w_ij over this rank's stored pairs, w = delta^-Q (SPEC 2.4.1, weighted
// degrees; once per map).  One wave per bin and no atomics, so the sum has a fixed order:
// each lane adds its own entries in a fixed sequence and the lanes meet in the fixed DPP tree.
// Row side: the unit holding row i in every strip J >= block(i), found by binary search in
// udesc (local units are ordered by (j0, i0)); column side: the units of strip block(i), lane l
// taking row groups l, l + 64, ... of it.  Which lane adds which pair, and in what order, thus
// depends on the pair's position alone, not on which tiles the layout holds: a blocked-sparse
// and a dense layout of one map give the same bits.  fp64 throughout: delta^-Q of an fp32 delta is exact
// enough to sum in double.
template <typename T, bool W, int Q>
__global__ __launch_bounds__(256) void unit_weight_sums_kernel(const T *__restrict__ units,
                                                               const int2 *__restrict__ udesc,
                                                               int64_t n_local, int64_t n_bins,
                                                               double *__restrict__ sums) {
    constexpr int VW = Lay<T, W>::VW, RPU = Lay<T, W>::RPU;
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n_bins) return;
    auto weight = [](T v) -> double {
        const double d = (double)v;
        return d > 0.0 ? (Q == 1 ? 1.0 / d : 1.0 / (d * d)) : 0.0;
    };
    // first local unit whose (j0, i0) is not below (j0, i0)
    auto lower = [&](int j0, int i0) -> int64_t {
        int64_t lo = 0, hi = n_local;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            const int2 d = udesc[mid];
            if (d.y < j0 || (d.y == j0 && d.x < i0)) lo = mid + 1;
            else hi = mid;
        }
        return lo;
    };
    const int b = (int)(i / VW);
    const int n_blocks = (int)((n_bins + VW - 1) / VW);
    const int i0 = (int)(i - i % RPU), r = (int)(i % RPU);
    double acc = 0.0;
    for (int J = b; J < n_blocks; ++J) {
        const int64_t ul = lower(J * VW, i0);
        if (ul >= n_local || udesc[ul].y != J * VW || udesc[ul].x != i0) continue;
        const T *row = units + ul * (RPU * VW) + (int64_t)r * VW;
        for (int c = lane; c < VW; c += 64) {
            const int64_t j = (int64_t)J * VW + c;
            if (j > i && j < n_bins) acc += weight(row[c]);
        }
    }
    const int c = (int)(i - (int64_t)b * VW);
    for (int64_t p = lane; p * RPU < i; p += 64) {   // lane: the rows p*RPU.. of strip b
        const int64_t ul = lower(b * VW, (int)(p * RPU));
        if (ul >= n_local || udesc[ul].y != b * VW || udesc[ul].x != (int)(p * RPU)) continue;
        const T *col = units + ul * (RPU * VW) + c;
        for (int q = 0; q < RPU; ++q)
            if (p * RPU + q < i) acc += weight(col[q * VW]);
    }
    acc = wave_sum_hi(acc);
    if (lane == 63) sums[i] = acc;
}

// Measurement only: the same waves read the same units with the same rolling
// 8-row window, but do nothing with the data except fold it into a checksum --
// the practical HBM read ceiling for this access pattern on this box.
template <bool NT>
__global__ __launch_bounds__(256, 4) void stream_read_kernel(const float4 *__restrict__ units,
                                                             int chunk_q, int chunk_r,
                                                             float *__restrict__ sink) {
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
    const int ua = w * chunk_q + (w < chunk_r ? w : chunk_r);
    const int ub = ua + chunk_q + (w < chunk_r ? 1 : 0);
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    if (ua < ub) {
        float4 d[8];
        const float4 *first = units + (int64_t)ua * 512 + lane;
#pragma unroll
        for (int r = 0; r < 8; ++r) d[r] = stream_load<NT>(first + r * 64);
        for (int u = ua; u < ub; ++u) {
            const int un = u + 1 < ub ? u + 1 : u;
            const float4 *next = units + (int64_t)un * 512 + lane;
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                acc.x += d[r].x; acc.y += d[r].y; acc.z += d[r].z; acc.w += d[r].w;
                d[r] = stream_load<NT>(next + r * 64);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    }
    if (acc.x + acc.y + acc.z + acc.w == 12345.678f) sink[w] = acc.x;  // keep the loads alive
}

// Measurement only, as stream_read_kernel: the same waves read the stream of their units, KiB
// by KiB with 8 KiB in flight (unit u begins at table[u].z KiB, the stream ends at end_kib).
template <bool NT>
__global__ __launch_bounds__(256, 4) void stream_read_pk24_kernel(const float4 *__restrict__ stream,
                                                                  const int4 *__restrict__ table,
                                                                  int n_units, int end_kib,
                                                                  int chunk_q, int chunk_r,
                                                                  float *__restrict__ sink) {
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
    const int ua = w * chunk_q + (w < chunk_r ? w : chunk_r);
    const int ub = ua + chunk_q + (w < chunk_r ? 1 : 0);
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    if (ua < ub) {
        const int ka = table[ua].z & 0x7fffffff;
        const int kb = ub < n_units ? table[ub].z & 0x7fffffff : end_kib;
        float4 d[8];
        const float4 *base = stream + lane;
#pragma unroll
        for (int r = 0; r < 8; ++r) d[r] = stream_load<NT>(base + (int64_t)min(ka + r, kb - 1) * 64);
        for (int k = ka; k < kb; k += 8) {
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                acc.x += d[r].x; acc.y += d[r].y; acc.z += d[r].z; acc.w += d[r].w;
                d[r] = stream_load<NT>(base + (int64_t)min(k + 8 + r, kb - 1) * 64);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    }
    if (acc.x + acc.y + acc.z + acc.w == 12345.678f) sink[w] = acc.x;  // keep the loads alive
}

// --------------------------------------------------------------------------
// landmark constraints (SPEC 2.5.5), the step quantities only: per bin, lambda * sum of A^-Q
// over the terms that touch it (bb_solver_anchor_sums; A as in bb_anchor_kernels.h)
// --------------------------------------------------------------------------
// (With the queries, not with the other landmark kernels: they are asked once per map, beside
// the degrees and the weight sums, and share their frame on the host.)
template <typename T, int Q>
__device__ __forceinline__ double anchor_weight(T v) {
    const double d = (double)v;
    if (!(d > 0.0)) return 0.0;
    return Q == 0 ? 1.0 : (Q == 1 ? 1.0 / d : 1.0 / (d * d));
}
// node side: sums[v] = lambda * sum_a w(A[a][v]), a ascending
template <typename T, int Q>
__global__ __launch_bounds__(256) void anchor_sums_node_kernel(const T *__restrict__ A, int64_t n_pad,
                                                               int64_t n_bins, int n_rows, double lam,
                                                               double *__restrict__ sums) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= n_bins) return;
    double acc = 0.0;
    for (int a = 0; a < n_rows; ++a) acc += anchor_weight<T, Q>(A[(int64_t)a * n_pad + v]);
    sums[v] = lam * acc;
}
// landmark side, one workgroup per landmark, launched behind the node side: thread t adds nodes
// t, t + 256, ... in order, the threads meet in the fixed tree, sums[s_a] += lambda * the total
template <typename T, int Q>
__global__ __launch_bounds__(256) void anchor_sums_landmark_kernel(const T *__restrict__ A, int64_t n_pad,
                                                                   int64_t n_bins,
                                                                   const int *__restrict__ nodes, double lam,
                                                                   double *__restrict__ sums) {
    __shared__ double sh[256];
    const int tid = threadIdx.x, a = blockIdx.x;
    double acc = 0.0;
    for (int64_t v = tid; v < n_bins; v += 256) acc += anchor_weight<T, Q>(A[(int64_t)a * n_pad + v]);
    sh[tid] = acc;
    __syncthreads();
    lds_tree_fold(sh, tid, 256);
    if (tid == 0) sums[nodes[a]] += lam * sh[0];
}

}  // namespace
