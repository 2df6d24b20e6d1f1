// bb_balance_loop.h -- the balancing iteration of docs/SPEC.md 2.5.2 with the product left to the
// caller: bb_balance.hip (which owns the loop's kernels and its device-resident state) runs it on
// the banded product of a resident matrix, bb_triples_balance.hip on the product over the
// canonical index of resident triples (2.5.3).  Everything but the product is this one copy: the
// input check's verdict, min_nnz, the mask's fixed point, balance_step_kernel, the batches of
// iterations per read-back, the final scale.
#pragma once

#include <float.h>
#include <stdint.h>

#include <functional>
#include <string>

#include "bb_common.h"

namespace bb {

// y = A x under cell rule `mode` (kCellValue / kCellNonzero / kCellBad, bb_cm_internal.h),
// enqueued on the loop's stream; `stop` (may be NULL): the kernels return at once when *stop != 0.
using BalanceProduct = std::function<hipError_t(int mode, const double *x, double *y, const int *stop)>;

// The arguments bb_cm_balance and bb_triples_balance share, checked alike.
inline int balance_check_args(const char *who_, int64_t n_bins, int64_t ignore_diags, int64_t min_nnz,
                              double tol, int64_t max_iter, double row_sum, const double *bias,
                              const uint8_t *masked) {
    const std::string who(who_);
    BB_REQUIRE(bias != nullptr && masked != nullptr, who + ": NULL argument");
    BB_REQUIRE(ignore_diags >= 0 && min_nnz >= 0, who + ": ignore_diags / min_nnz is negative");
    BB_REQUIRE(tol >= 0.0 && tol <= DBL_MAX && max_iter >= 0, who + ": bad tol / max_iter");
    BB_REQUIRE(row_sum == row_sum && row_sum <= DBL_MAX, who + ": row_sum is not finite");
    BB_REQUIRE(n_bins >= 1, who + ": no bin is left to balance (the map has no bins)");
    return BB_OK;
}

// The whole of 2.5.2 over n bins on stream `st`; the messages name `who`.
int balance_loop(const char *who, int64_t n, hipStream_t st, const BalanceProduct &product,
                 int64_t min_nnz, double tol, int64_t max_iter, double row_sum, double *bias,
                 uint8_t *masked, int64_t *iterations, double *variance);

// x = 1 / bias, 0 where the bias is NaN (device vectors)
hipError_t inverse_bias_enqueue(const double *bias, double *x, int64_t n, hipStream_t st);

}  // namespace bb
