// bb_peer_kernels.h -- device code of the peer exchange of the 3D-structure solver (gfx950
// only): what a slot word says by itself (empty / arrived), a wave's bounded wait for the
// words of every rank, and peer_receive_kernel, the receiving half of the two-launch form.
// The one-launch form, reduce_exchange_kernel, is a reduce and lives with it in
// bb_solver_kernels.h, which includes this file for the helpers; peer_receive_kernel is
// launched by bb_solver_exchange.hip alone (bb::solver::launch_peer_receive).  Tables, states
// and the fixed-order sums: bb_solver_device.h.  Design: DESIGN.md 4.3.
#pragma once

#include "bb_solver_device.h"

namespace {

__device__ __forceinline__ bool peer_word_empty(float v) { return __float_as_uint(v) == 0xffffffffu; }
__device__ __forceinline__ bool peer_word_empty(double v) { return __double_as_longlong(v) == -1ll; }
__device__ __forceinline__ float peer_empty_word(float) { return __uint_as_float(0xffffffffu); }
__device__ __forceinline__ double peer_empty_word(double) { return __longlong_as_double(-1ll); }
// what is pushed must not look empty: a sum with exactly those bits becomes the canonical NaN
template <typename T>
__device__ __forceinline__ T peer_sendable(T v) {
    return peer_word_empty(v) ? (T)__builtin_nanf("") : v;
}

// One wave's wait for `n_words` words per lane of every rank: base + r * slot_elems (+ 1 for
// the second word), r < R.  Returns true with the rank-ordered sum(s) in out0 / out1 and the
// words emptied; false after a time-out, a poison word or a set status (status set, peers
// poisoned).  `active` lanes have an element; the others only take part in the votes.
template <typename T, int NW>
__device__ __forceinline__ bool peer_wait_sum(const T *base, bool active, int R, int64_t slot_elems,
                                              const PeerTableX<T> *xt, const unsigned long long *my_poison,
                                              PeerState *state, long long limit, T &sum, double &pair_sum,
                                              unsigned mask = ~0u) {
    const int lane = threadIdx.x & 63;
    T v[NW][kMaxPeers];
    bool ok = false;
    const long long t0 = wall_clock64();
    for (;;) {
        bool missing = false;
#pragma unroll
        for (int r = 0; r < kMaxPeers; ++r) {
            if (r < R) {
                const bool sends = (mask >> r & 1u) != 0;        // (wave-uniform)
#pragma unroll
                for (int w = 0; w < NW; ++w) {
                    v[w][r] = (active && sends)
                                  ? __hip_atomic_load(base + (int64_t)r * slot_elems + w, __ATOMIC_RELAXED,
                                                      __HIP_MEMORY_SCOPE_SYSTEM)
                                  : T(0);
                    missing |= peer_word_empty(v[w][r]);
                }
            }
        }
        // lanes [0, R): rank `lane`'s poison word in this arena; lane R: this rank's status
        unsigned long long f = 0;
        if (lane < R)
            f = __hip_atomic_load(my_poison + 8 * lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        else if (lane == R)
            f = (unsigned long long)__hip_atomic_load(&state->status, __ATOMIC_RELAXED,
                                                      __HIP_MEMORY_SCOPE_AGENT);
        if (__ballot(lane < R ? f == kPeerPoison : f != 0) != 0) break;
        if (__ballot(missing) == 0) { ok = true; break; }
        if (__ballot(wall_clock64() - t0 > limit) != 0) break;      // wave-uniform exits only
        __builtin_amdgcn_s_sleep(2);
    }
    if (!ok) {
        if (lane < R)
            __hip_atomic_store(xt->poison[lane], kPeerPoison, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        if (lane == 0)
            __hip_atomic_store(&state->status, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return false;
    }
    // NW = 1: the element's sum over the ranks, in rank order, in T.  NW = 2: the words are a
    // (hi, lo) pair of one double per rank: their sum in double, rank by rank
    T s0 = T(0);
    double s2 = 0.0;
#pragma unroll
    for (int r = 0; r < kMaxPeers; ++r) {
        if (r < R) {
            s0 += v[0][r];
            if (NW > 1) s2 += (double)v[0][r] + (double)v[NW - 1][r];
            if (active && (mask >> r & 1u)) {
#pragma unroll
                for (int w = 0; w < NW; ++w)
                    __hip_atomic_store(const_cast<T *>(base) + (int64_t)r * slot_elems + w,
                                       peer_empty_word(T(0)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            }
        }
    }
    sum = s0;
    pair_sum = s2;
    return true;
}

// Peer exchange, receiving side -- one launch.  Wave 0 of workgroup 0 waits until every
// source rank's flag has reached `seq` and publishes the outcome (state->verdict = seq);
// wave 0 of every other workgroup polls that LOCAL word and the sticky status, so the
// step is applied by all workgroups or by none.  The wait is bounded: past `limit`
// ticks of the constant-rate clock -- or when a peer has left its poison flag -- the
// status word is set, the verdict is withheld, and this rank's own flag on every peer
// is poisoned so that nobody goes on consuming partials computed from coordinates that
// no longer move.  Deciding in one place is what keeps X whole: with every workgroup
// polling the remote flags for itself, some could time out while later ones saw them
// arrive.  Workgroup 0 is dispatched first, so the deciding wave is resident before any
// wave that waits for it; it waits for other devices only.
// Then X <- X + (mu V - lr * sum over ranks, in rank order).  `arena` is this parity's
// first slot; it is uncached memory, read past L1/L2.
template <typename T>
__global__ __launch_bounds__(256) void peer_receive_kernel(
    T *__restrict__ X, T *__restrict__ V, const T *arena, const unsigned long long *flags,
    unsigned long long *const *poison_flags, int world, int64_t slot_elems, int64_t n3, T lr, T mu,
    double *stress_out, unsigned long long seq, PeerState *state, long long limit,
    const unsigned *__restrict__ peer_mask, int ch) {
    const int tid = threadIdx.x;
    __shared__ int go;
    if (tid < 64) {
        bool all_ok = false;
        if (blockIdx.x == 0) {
            const int lane = tid;
            if (__hip_atomic_load(&state->status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) {
                // The whole wave polls together until EVERY flag is there: a lane whose
                // flag has arrived keeps reading it, so a poison that lands later is seen.
                const long long t0 = wall_clock64();
                for (;;) {
                    const unsigned long long f =
                        lane < world ? __hip_atomic_load(flags + 8 * lane, __ATOMIC_ACQUIRE,
                                                         __HIP_MEMORY_SCOPE_SYSTEM)
                                     : seq;
                    if (__ballot(f == kPeerPoison) != 0) break;
                    if (__ballot(f >= seq) == __ballot(1)) { all_ok = true; break; }
                    if (__ballot(wall_clock64() - t0 > limit) != 0) break;   // wave-uniform exits only
                    __builtin_amdgcn_s_sleep(4);
                }
            }
            if (all_ok) {
                if (lane == 0)
                    __hip_atomic_store(&state->verdict, seq, __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_AGENT);
            } else {
                if (lane < world)
                    __hip_atomic_store(poison_flags[lane], kPeerPoison, __ATOMIC_RELEASE,
                                       __HIP_MEMORY_SCOPE_SYSTEM);
                if (lane == 0)
                    __hip_atomic_store(&state->status, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            // one word says "this launch's wait is over": what the other workgroups poll
            if (lane == 0)
                __hip_atomic_store(&state->decided, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
        } else {
            // ends when workgroup 0 has decided, one way or the other (it always does:
            // its own wait is bounded)
            // (relaxed polls of ONE word, well apart, and ONE acquire fence at the end: an
            // acquire is a cache invalidate on this part -- 200 waves issuing one per poll
            // cost 12 us -- and a thousand waves hammering one line leave little of its
            // memory channel to the ranks that share the device in a rehearsal)
            while (__hip_atomic_load(&state->decided, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != seq)
                __builtin_amdgcn_s_sleep(32);
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            all_ok = __hip_atomic_load(&state->verdict, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == seq;
        }
        if (tid == 0) go = all_ok ? 1 : 0;
    }
    __syncthreads();
    if (!go) return;
    // The arena is read with system-scope loads, which go past L1/L2 to memory: issued
    // after the barrier they cannot be older than the flags wave 0 acquired.
    // The grid is capped (kPeerReceiveWGs workgroups, a thread takes several elements): a
    // grid the size of the update would fill every wave slot of the device with waves that
    // spin, and when several ranks share one GPU -- the test box, a rehearsal -- the kernel of
    // the rank they wait for could then not start at all (found by the four-rank test at
    // N=309,568: 3,629 workgroups waiting, nobody delivering, time-out).
    constexpr int EPT = 4;
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t base = (int64_t)blockIdx.x * 256 + tid; base < n3; base += EPT * stride) {
        // all slots of all of the thread's elements are requested before the first add; the
        // sum of an element runs in rank order (rank_ordered_sums)
        T g[EPT];
        int64_t el[EPT];
        bool live[EPT];
        unsigned mk[EPT];                       // the ranks that sent something for the element's block
#pragma unroll
        for (int q = 0; q < EPT; ++q) {
            el[q] = base + q * stride;
            live[q] = el[q] < n3;
            mk[q] = (peer_mask != nullptr && live[q]) ? peer_mask[el[q] / ch] : ~0u;
        }
        rank_ordered_sums(g, live, mk, world, [&](int q, int r) {
            return __hip_atomic_load(arena + r * slot_elems + el[q], __ATOMIC_RELAXED,
                                     __HIP_MEMORY_SCOPE_SYSTEM);
        });
#pragma unroll
        for (int q = 0; q < EPT; ++q) {
            const int64_t e = base + q * stride;
            if (e < n3) momentum_step(X, V, e, mu, lr, g[q]);
        }
    }
    if (blockIdx.x == 0 && tid == 0) {
        double S = 0.0;
        for (int r = 0; r < world; ++r)
            S += (double)__hip_atomic_load(arena + r * slot_elems + n3, __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_SYSTEM) +
                 (double)__hip_atomic_load(arena + r * slot_elems + n3 + 1, __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_SYSTEM);
        *stress_out = S;
    }
}
constexpr unsigned kPeerReceiveWGs = 256;

}  // namespace
