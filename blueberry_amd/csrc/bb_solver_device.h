// bb_solver_device.h -- what the kernel headers of the 3D-structure solver share (gfx950 only):
// the unit shapes (Traits, Lay), the wave-level helpers (DPP sums, lane values, the dropped
// store), the op / mode constants that host and kernels both name, the peer exchange's tables,
// the momentum step and the fixed-order sums.  Helpers only -- no kernel is defined here, so a
// file that includes it compiles none: every kernel belongs to exactly one translation unit,
//   bb_solver_kernels.h    sweep, reduce, one-launch exchange, apply,            bb_solver.hip
//                          row-owner, 24-bit stream
//   bb_peer_kernels.h      the peer exchange's waits, peer_receive_kernel        bb_solver_exchange.hip
//   bb_input_kernels.h     pack / scatter / gen / repower, units -> full matrix  bb_solver_inputs.hip
//   bb_query_kernels.h     degrees / weight sums / anchor sums, read probes      bb_solver_queries.hip
//   bb_anchor_kernels.h   landmark constraints                                  bb_solver_anchors.hip
//   bb_spectral_kernels.h  the N x 3 algebra of the spectral start               bb_solver_spectral.hip
// and group_apply_kernel to bb_group.hip.  Everything here lives in the including translation
// unit's anonymous namespace.
//
// Specification: docs/SPEC.md (build-authored; the reference has no solver,
// SURVEY.md section 0).  Data layout and kernel design: DESIGN.md 3-4.
//
// Layout recap (SPEC 3).  The matrix is cut into vw x vw tiles (vw = 512 columns;
// 128 for small fp64 problems, see Lay<> below), upper-triangular tiles only, ordered
// column-strip major (J, then I).  A tile is vw/rpu "units"; a unit is rpu matrix rows
// x vw columns = 8 KiB, row-major (fp32: 4 rows of 2 KiB; fp64: 2 rows of 4 KiB, or 8
// rows of 1 KiB).
// One wave reads a matrix row of a unit with LPR 16-B-per-lane loads and lane
// l always owns the same LPR*VPL columns of the strip.  That makes the column
// side of the symmetric update register-resident for a whole strip sweep (no
// cross-lane traffic), and only the row side needs one DPP wave reduction per
// matrix row -- amortised over 8 pairs per lane in fp32.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "bb_wish.h"
#include "blueberry_hip.h"

namespace {

// --------------------------------------------------------------------------
// type traits
// --------------------------------------------------------------------------
template <typename T>
struct Traits;
template <>
struct Traits<float> {
    using Vec = float4;
    static constexpr int VPL = 4;  // elements per lane per 16-B load
    static __device__ __forceinline__ float eps2() { return 1e-30f; }
};
template <>
struct Traits<double> {
    using Vec = double2;
    static constexpr int VPL = 2;
    static __device__ __forceinline__ double eps2() { return 1e-300; }
};

// The wish floor and ceiling, the flush and the value rule: bb_wish.h (shared with the
// shortest paths over triples).
using bb::flush_wish;
using bb::wish_ceiling;
using bb::wish_floor;
using bb::wish_from_value;

// Shape of a unit (8 KiB = 8 wave-loads) and of a strip.  LPR 16-byte loads per lane
// and matrix row, VW = 64 * VPL * LPR columns per strip, RPU = 8 / LPR matrix rows.
//   fp32          4 rows x 512 columns: 8 pairs per lane and row, packed math
//   fp64 wide     2 rows x 512 columns: also 8 pairs per lane and row, so the DPP
//                 reduction, the row-coordinate fetch and the row-sum stores are
//                 amortised over 4x more pairs than in the narrow shape (+40 % at
//                 N=20k); 96 VGPRs of column state, so at most 2 waves per SIMD
//   fp64 narrow   8 rows x 128 columns: 4x smaller column partials and 4x more
//                 blocks for the reduce -- what small problems want (N=963: 14.5 us
//                 per iteration against 26 us in the wide shape); bb_common.h picks
//                 it for n_bins <= kF64WideFrom
template <typename T, bool W>
struct Lay;
template <bool W>
struct Lay<float, W> {
    static constexpr int LPR = 2, VW = 512, RPU = 4;
    static constexpr int MIN_WG = 4;            // __launch_bounds__: <= 128 VGPRs
    static constexpr bool SCALAR_XROW = true;   // 12 row coordinates through the scalar cache
};
template <>
struct Lay<double, true> {
    static constexpr int LPR = 4, VW = 512, RPU = 2;
    static constexpr int MIN_WG = 2;            // <= 256 VGPRs
    static constexpr bool SCALAR_XROW = true;   // 6 doubles = 12 SGPRs, double-buffered
};
template <>
struct Lay<double, false> {
    static constexpr int LPR = 1, VW = 128, RPU = 8;
    // <= 256 VGPRs.  This shape only ever runs one workgroup of 4 waves per CU (at most 4096
    // bins: fewer than 65k units, waves_per_cu() = 4), so a cap of 128 registers bought no
    // occupancy and, from round 3 on, cost a 20-byte scratch spill in the stress sweep
    // (tests/test_host.py::test_product_kernels_do_not_spill guards against the next one).
    static constexpr int MIN_WG = 2;
    static constexpr bool SCALAR_XROW = false;  // 24 doubles x 2 would not fit the SGPR file:
                                                // one per-lane load + v_readlane instead
};

// --------------------------------------------------------------------------
// cross-lane helpers (wave64, DPP; no LDS)
// --------------------------------------------------------------------------
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_get(float v) {
    return __int_as_float(
        __builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, ROW_MASK, 0xF, false));
}
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double dpp_get(double v) {
    int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, ROW_MASK, 0xF, false);
    int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, ROW_MASK, 0xF, false);
    return __hiloint2double(hi, lo);
}

// Sum over the 64 lanes; the total is valid in lanes 48..63 (we read lane 63).
// Fixed tree => bitwise deterministic.
template <typename T>
__device__ __forceinline__ T wave_sum_hi(T v) {
    v += dpp_get<0xB1, 0xF>(v);   // quad_perm [1,0,3,2]
    v += dpp_get<0x4E, 0xF>(v);   // quad_perm [2,3,0,1]
    v += dpp_get<0x141, 0xF>(v);  // row_half_mirror
    v += dpp_get<0x140, 0xF>(v);  // row_mirror
    v += dpp_get<0x142, 0xA>(v);  // row_bcast15 -> rows 1,3
    v += dpp_get<0x143, 0xC>(v);  // row_bcast31 -> rows 2,3
    return v;
}

// The same tree for three fp32 values at once, as one asm block.  Interleaving
// the three chains puts two independent VALU ops between every write of a
// register and its next DPP read, which is exactly the 2 wait states that
// hazard needs (the compiler serialises the chains and pads each step with
// s_nop), and the two row_bcast steps become single v_add_f32_dpp with a
// partial row_mask (disabled rows keep their value) instead of mov+mov+add.
// Only the leading s_nop is needed: the inputs were just written by VALU code.
__device__ __forceinline__ void wave_sum_hi3(float &a, float &b, float &c) {
    asm("s_nop 1\n\t"
        "v_add_f32_dpp %0, %0, %0 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
        "v_add_f32_dpp %1, %1, %1 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
        "v_add_f32_dpp %2, %2, %2 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
        "v_add_f32_dpp %0, %0, %0 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"
        "v_add_f32_dpp %1, %1, %1 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"
        "v_add_f32_dpp %2, %2, %2 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"
        "v_add_f32_dpp %0, %0, %0 row_half_mirror row_mask:0xf bank_mask:0xf\n\t"
        "v_add_f32_dpp %1, %1, %1 row_half_mirror row_mask:0xf bank_mask:0xf\n\t"
        "v_add_f32_dpp %2, %2, %2 row_half_mirror row_mask:0xf bank_mask:0xf\n\t"
        "v_add_f32_dpp %0, %0, %0 row_mirror row_mask:0xf bank_mask:0xf\n\t"
        "v_add_f32_dpp %1, %1, %1 row_mirror row_mask:0xf bank_mask:0xf\n\t"
        "v_add_f32_dpp %2, %2, %2 row_mirror row_mask:0xf bank_mask:0xf\n\t"
        "v_add_f32_dpp %0, %0, %0 row_bcast:15 row_mask:0xa bank_mask:0xf\n\t"
        "v_add_f32_dpp %1, %1, %1 row_bcast:15 row_mask:0xa bank_mask:0xf\n\t"
        "v_add_f32_dpp %2, %2, %2 row_bcast:15 row_mask:0xa bank_mask:0xf\n\t"
        "v_add_f32_dpp %0, %0, %0 row_bcast:31 row_mask:0xc bank_mask:0xf\n\t"
        "v_add_f32_dpp %1, %1, %1 row_bcast:31 row_mask:0xc bank_mask:0xf\n\t"
        "v_add_f32_dpp %2, %2, %2 row_bcast:31 row_mask:0xc bank_mask:0xf"
        : "+v"(a), "+v"(b), "+v"(c));
}
__device__ __forceinline__ void wave_sum_hi3(double &a, double &b, double &c) {
    a = wave_sum_hi(a);
    b = wave_sum_hi(b);
    c = wave_sum_hi(c);
}

// Value of `v` in lane `l` (compile-time l) as a wave-uniform scalar.
__device__ __forceinline__ float lane_value(float v, int l) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}
__device__ __forceinline__ double lane_value(double v, int l) {
    int lo = __builtin_amdgcn_readlane(__double2loint(v), l);
    int hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
    return __hiloint2double(hi, lo);
}

// Branch-free "lane 63 only" store of a row's three sums through a raw buffer
// descriptor: every other lane carries an out-of-range offset and the
// hardware range check drops its store.  (An `if (lane == 63)` around a plain
// store splits the unit into basic blocks, and LLVM then sinks all column-side
// accumulation below the last of them, spilling 32 pairs of forces.)
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x3 __attribute__((ext_vector_type(3)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
constexpr unsigned kDropOffset = 0x80000000u;

__device__ __forceinline__ void store_row3(__amdgpu_buffer_rsrc_t rsrc, unsigned voff, double a,
                                           double b, double c) {
    u32x4 v = {(unsigned)__double2loint(a), (unsigned)__double2hiint(a),
               (unsigned)__double2loint(b), (unsigned)__double2hiint(b)};
    u32x2 w = {(unsigned)__double2loint(c), (unsigned)__double2hiint(c)};
    __builtin_amdgcn_raw_buffer_store_b128(v, rsrc, voff, 0, 0);
    __builtin_amdgcn_raw_buffer_store_b64(w, rsrc, voff + 16, 0, 0);
}

// --------------------------------------------------------------------------
// constants host and kernels both name
// --------------------------------------------------------------------------
// What the sweep computes per pair (i, j), template parameter OP:
//   kOpStress : residual force of SPEC 2.3 -> gradient (row and column side) + stress
//   kOpMatvec2: y_i += delta_ij^2 * x_j and y_j += delta_ij^2 * x_i for three
//               right-hand sides held in the coordinate slots: Y = (D o D) X, the
//               kernel of classical-MDS / spectral initialisation
//   kOpStressW1, kOpStressW2: the weighted stress of SPEC 2.3.1, w = delta^-1 (Sammon) or
//               delta^-2 (relative stress); r = 1/delta is computed in-kernel from the delta
//               the sweep loads anyway (no extra bytes), and masked where delta = 0
enum { kOpStress = 0, kOpMatvec2 = 1, kOpStressW1 = 2, kOpStressW2 = 3 };
template <int OP>
constexpr bool is_weighted_op() { return OP == kOpStressW1 || OP == kOpStressW2; }

// What the reduce does with a block's sum (reduce_sliced_kernel, bb_solver_kernels.h)
enum ReduceMode {
    kReduceApply = 0,      // X -= lr * 2 * sum
    kReduceExchange = 1,   // exch = 2 * sum (+ stress hi/lo)
    kReduceStressOnly = 2, // stress only
    kReducePeer = 4        // 2 * sum (+ stress hi/lo) stored into this rank's slot on every peer
};

// Peer exchange (bb_solver_peer_*): where this rank's partial goes on each rank
// (its slot in that rank's receive arena, for one parity) and the flag to raise.
constexpr int kMaxPeers = 16;
template <typename T>
struct PeerTable {
    T *dst[kMaxPeers];
    unsigned long long *flag[kMaxPeers];
};
// Health of this rank's peer exchange, in device memory.  `status` is sticky: once a
// wait has failed (time limit, or a peer reported its own failure) every later launch
// of this rank leaves X alone and pushes nothing.  `verdict` is the sequence number of
// the last exchange whose R partials all arrived, `decided` that of the last launch whose
// wait has ended either way: both written by ONE wave (the first of peer_receive_kernel);
// the other workgroups of that launch poll `decided`, then read `verdict`, so a step is
// applied by all of its workgroups or by none.
struct PeerState {
    int status;
    int pad;
    unsigned long long verdict;
    unsigned long long decided;   // sequence number of the last launch whose wait has ended, either way
};
// Flag value a failed rank leaves on every peer: their waits end at once and fail too.
constexpr unsigned long long kPeerPoison = ~0ull;

// SPEC 2.4: V <- mu V - lr g ; X <- X + V   (mu = 0: X -= lr g).  The new velocity; for element
// o with the old values xo, vo at hand (the reduces load them early, independent of the sum);
// in place.  row_owner_kernel writes X to a second buffer, three elements at a time: it takes
// the velocities and stores for itself.
template <typename T>
__device__ __forceinline__ T momentum_velocity(T mu, T vo, T lr, T g) { return mu * vo - lr * g; }
template <typename T>
__device__ __forceinline__ void momentum_step(T *__restrict__ X, T *__restrict__ V, int64_t o, T xo, T vo,
                                              T mu, T lr, T g) {
    const T v = momentum_velocity(mu, vo, lr, g);
    V[o] = v;
    X[o] = xo + v;
}
template <typename T>
__device__ __forceinline__ void momentum_step(T *__restrict__ X, T *__restrict__ V, int64_t o, T mu, T lr,
                                              T g) {
    const T vo = V[o];
    momentum_step(X, V, o, X[o], vo, mu, lr, g);
}

// The sum over ranks of N elements, in rank order from 0 (part of the specification: every
// transport gives the same bits).  Eight ranks at a time: the words of all N elements are
// requested before the first add -- one memory round trip per eight ranks, not one per rank and
// element -- and a rank outside an element's mask mk[q] adds 0.  load(q, r): rank r's word of
// element q, asked for only where live[q] and the rank is in the mask.
template <int N, typename T, typename L>
__device__ __forceinline__ void rank_ordered_sums(T (&g)[N], const bool (&live)[N],
                                                  const unsigned (&mk)[N], int world, L load) {
#pragma unroll
    for (int q = 0; q < N; ++q) g[q] = T(0);
    for (int r0 = 0; r0 < world; r0 += 8) {
        T v[N][8];
#pragma unroll
        for (int q = 0; q < N; ++q)
#pragma unroll
            for (int p = 0; p < 8; ++p)
                v[q][p] = (live[q] && r0 + p < world && (mk[q] >> (r0 + p) & 1u)) ? load(q, r0 + p) : T(0);
#pragma unroll
        for (int q = 0; q < N; ++q)
#pragma unroll
            for (int p = 0; p < 8; ++p)
                if (r0 + p < world) g[q] += v[q][p];
    }
}

// The stress travels in the solver's type as a pair: hi = (T)S, lo = (T)(S - hi).
template <typename T>
__device__ __forceinline__ void split_hi_lo(double S, T &hi, T &lo) {
    hi = (T)S;
    lo = (T)(S - (double)hi);
}

// sh[0] <- sh[0] + ... + sh[n - 1] by a fixed tree (bitwise reproducible); n = the workgroup's
// threads, a power of two.  Called by every thread, behind the barrier that follows its own
// store to sh[tid].
__device__ __forceinline__ void lds_tree_fold(double *sh, int tid, int n) {
    for (int off = n >> 1; off > 0; off >>= 1) {
        if (tid < off) sh[tid] += sh[tid + off];
        __syncthreads();
    }
}

// Matrix rows are read exactly once per launch: NT = true marks the loads
// non-temporal so the stream does not evict X and the partials from L2 / MALL.
typedef float f32x4_raw __attribute__((ext_vector_type(4)));
typedef double f64x2_raw __attribute__((ext_vector_type(2)));
template <bool NT>
__device__ __forceinline__ float4 stream_load(const float4 *p) {
    if constexpr (NT) {
        const f32x4_raw v = __builtin_nontemporal_load(reinterpret_cast<const f32x4_raw *>(p));
        return make_float4(v.x, v.y, v.z, v.w);
    } else {
        return *p;
    }
}
template <bool NT>
__device__ __forceinline__ double2 stream_load(const double2 *p) {
    if constexpr (NT) {
        const f64x2_raw v = __builtin_nontemporal_load(reinterpret_cast<const f64x2_raw *>(p));
        return make_double2(v.x, v.y);
    } else {
        return *p;
    }
}

// The one-launch peer exchange (reduce_exchange_kernel, bb_solver_kernels.h): where this rank's
// words go on each rank.
template <typename T>
struct PeerTableX {
    T *dst[kMaxPeers];                       // this rank's slot in rank q's arena (one parity)
    unsigned long long *poison[kMaxPeers];   // this rank's poison word in rank q's arena
};

// What launch_anchors folds the landmark terms into (bb_anchor_kernels.h)
enum AnchorFold {
    kAnchorFoldExchange = 0,   // landmark gradients and the stress into the exchange buffer
    kAnchorFoldStress = 1,     // stress_out[0] += the anchor stress
    kAnchorFoldAlone = 2       // the anchor stress alone
};

}  // namespace
