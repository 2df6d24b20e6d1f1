// bb_wish.h -- what becomes a wish distance (docs/SPEC.md 2.1): the ONE place that says so,
// shared by the solver's pack kernels (bb_solver_kernels.h), whose sweep derives its 0/1 weight
// from the flush, and by the shortest paths over triples (bb_triples_paths.hip), whose edge
// weights are the same distances in float64.
#pragma once

#include <hip/hip_runtime.h>

#include "blueberry_hip.h"

namespace bb {

// Wish distances below this are stored as 0 = "no constraint" by every pack kernel: far
// below the distance floor eps of SPEC 2.2 (1e-15 / 1e-150), and what lets the kernels
// turn "delta > 0" into a 0/1 weight with one clamped multiply (delta * 2^100 resp.
// 2^1000 saturates to 1 for every delta that survives the flush).
template <typename T>
__host__ __device__ constexpr double wish_floor() { return sizeof(T) == 4 ? 1e-30 : 1e-290; }
// ... and the largest one: a float64 distance far above the largest finite T would become
// +inf in the cast (1e39 as 'wish', the count 1e-120) -- a pair that counts as a constraint and
// makes every stress non-finite.  Every distance above this value AS A DOUBLE is "no
// constraint", like one below the floor: the doubles within half a float32 step above
// FLT_MAX, which the cast would round down to it, included; so is +inf (generated coordinates
// whose squared separation overflows).
template <typename T>
__host__ __device__ constexpr double wish_ceiling() {
    return sizeof(T) == 4 ? 3.4028234663852886e38 : 1.7976931348623157e308;
}

// flush_wish: a distance below the floor is 0 = "no constraint" (fp32: the kernel's 0/1 weight
// needs delta >= 2^-100; anything that small is below the distance clamp eps = 1e-15 anyway),
// and so is one above the largest finite T (wish_ceiling: the units never hold +inf).
// wish_from_value: an input value v of `kind` -- finite and positive, else no constraint;
// counts -> v^(-1/alpha) -- then the flush.
template <typename T>
__device__ __forceinline__ T flush_wish(double v) {
    return (T)((v < wish_floor<T>() || v > wish_ceiling<T>()) ? 0.0 : v);
}
template <typename T>
__device__ __forceinline__ T wish_from_value(double v, int kind, double neg_inv_alpha) {
    const bool ok = (v > 0.0) && (v <= 1.7976931348623157e308);  // finite, positive
    if (!ok)
        v = 0.0;
    else if (kind == BB_KIND_COUNTS)
        v = pow(v, neg_inv_alpha);
    return flush_wish<T>(v);
}

}  // namespace bb
