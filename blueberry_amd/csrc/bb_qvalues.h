// bb_qvalues.h -- the device-pointer entries of the Benjamini-Hochberg scan and of the q-value
// rule (docs/SPEC.md 2.9.7), both defined in bb_misc.hip next to the scan's kernels.  Their users:
// bb_benjamini_hochberg and bb_q_values (host in, host out: bb_misc.hip) and bb_sig_q_values (the
// resident list of a significance call: bb_significance.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bb {

// Bytes of the scan's block summaries for d values; `work` of bh_scan_enqueue holds that many.
size_t bh_scan_work_bytes(int64_t d);

// q[i] = the BH running maximum over the d SORTED device values p with n tests (bh_*_kernel),
// enqueued on st.  p and q are distinct device arrays of d doubles; d >= 1.
hipError_t bh_scan_enqueue(const double *p, int64_t d, double n, double *q, void *work, hipStream_t st);

// The q-value rule on m device values p in list order: key, stable sort of (key, place) over all
// 64 bits, gather, BH scan with n_tests, scatter into the device array q (m doubles).  order (may
// be NULL): m uint32_t on the device, the stable sorted order.  Every buffer but q and order is
// allocated here and freed before the return, which is synchronised.  sort_ms / scan_ms (may be
// NULL): HIP-event times on st of keys + sort, and of gather + scan + scatter.  m >= 2^32 is
// BB_ERR_INVALID, an allocation that fails BB_ERR_NOMEM; m = 0 is fine.
int q_values_device(const char *who, const double *p, int64_t m, int64_t n_tests, double *q, uint32_t *order,
                    hipStream_t st, double *sort_ms, double *scan_ms);

}  // namespace bb
