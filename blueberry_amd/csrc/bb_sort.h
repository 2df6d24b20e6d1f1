// bb_sort.h -- the library's one exclusive scan and its one stable sort of (64-bit key, payload)
// pairs on the device; both are compiled once, in bb_sort.hip, which tells how the sort works.
// The sort's users: the canonical index of resident triples (bb_triples_balance.hip: double
// payloads, the cells' values), the q-values of a list of p-values (bb_misc.hip) and the ranks of
// pair distances (bb_compare.hip): uint32_t payloads, the cells' places in the list.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bb_common.h"

namespace bb {

typedef unsigned long long sort_key;

// numpy's order of float64 as the unsigned order of 64 bits: negatives (bits inverted) below the
// zeros (both signs one key) below the positives (sign bit set), every NaN above them all
__device__ __forceinline__ sort_key order_key(double v) {
    const sort_key b = (sort_key)__double_as_longlong(v), top = (sort_key)1 << 63;
    if (v != v) return ~(sort_key)0;
    if (v == 0.0) return top;
    return (b & top) ? ~b : (b | top);
}

// out[i] = in[0] + ... + in[i - 1], i < n, on `st`.  tmp: exclusive_scan_bytes(n) bytes of device
// memory that the caller owns until the scan has run.
hipError_t exclusive_scan_bytes(size_t n, size_t *bytes);
hipError_t exclusive_scan(void *tmp, size_t tmp_bytes, const sort_key *in, sort_key *out, size_t n,
                          hipStream_t st);

// (k, v) sorted by the low `bits` bits of k, equal keys in their order; (k2, v2) are the second
// buffers.  On return k / v point at the sorted arrays and k2 / v2 at the other pair.  The
// counters (two of 256 x 8 B per tile, and the scan's temporary storage) are allocated here and
// die with the call, which ends synchronised.  V: uint32_t or double.
template <typename V>
hipError_t stable_sort_pairs(sort_key *&k, V *&v, sort_key *&k2, V *&v2, int64_t m, unsigned bits,
                             hipStream_t st);

}  // namespace bb
