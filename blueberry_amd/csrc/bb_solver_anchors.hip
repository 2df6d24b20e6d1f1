// bb_solver_anchors.hip -- the landmark constraints of the 3D-structure solver (docs/SPEC.md
// 2.5.5): bb_solver_set_anchors and what reports on them, and launch_anchors, which the
// iterating paths of bb_solver.hip and bb_group.hip call behind their reduce.  Its kernels:
// bb_anchor_kernels.h, compiled here and nowhere else.  gfx950 only.
#include <algorithm>
#include <cmath>

#include "bb_anchor_kernels.h"
#include "bb_solver_internal.h"
#include "bb_triples.h"

using namespace bb::solver;

namespace {

// The landmark terms of SPEC 2.5.5 at the coordinates X (bb_anchor_kernels.h), behind a reduce
// that has left its result: fold = kAnchorFoldExchange adds gradient and stress to the exchange
// buffer (three launches), kAnchorFoldStress adds the stress to stress_out[0], kAnchorFoldAlone
// leaves the anchor stress in anchor_part[0] alone (two launches: no gradient is formed).
double *anchor_stress_ptr(const bb_solver *s) { return s->anchor_part.as<double>(); }
double *anchor_node_part(const bb_solver *s) { return s->anchor_part.as<double>() + 8; }
double *anchor_lm_part(const bb_solver *s) {
    return anchor_node_part(s) + bb::round_up(s->anchor_node_blocks, 8);
}

}  // namespace

namespace bb {
namespace solver {

int launch_anchors(bb_solver *s, int fold, double *stress_out) {
    return by_dtype(s, [&](auto t) {
        using T = typename decltype(t)::T;
        return with_int<1, 2, 0>(s->weight_power, [&](auto qc) -> int {
            constexpr int Q = decltype(qc)::value;
            const T *A = s->anchor_rows.as<const T>();
            const int *nodes = s->anchor_nodes.as<const int>();
            const T *bin_scale = s->d_bin_scale.as<const T>();
            T *exch = fold == kAnchorFoldExchange ? (T *)s->d_exch : nullptr;
            BB_HIP_CHECK(bb::launch(anchor_node_kernel<T, Q>, dim3((unsigned)s->anchor_node_blocks), dim3(256),
                                    0, s->stream, A, s->L.n_pad, s->L.n_bins, s->anchor_n, nodes,
                                    (const T *)s->d_X, exch, bin_scale, (T)s->anchor_weight,
                                    anchor_node_part(s)));
            if (fold == kAnchorFoldExchange)
                BB_HIP_CHECK(bb::launch(anchor_landmark_kernel<T, Q>,
                                        dim3((unsigned)s->anchor_chunks, (unsigned)s->anchor_n), dim3(256), 0,
                                        s->stream, A, s->L.n_pad, s->L.n_bins, nodes, (const T *)s->d_X,
                                        (T)s->anchor_weight, anchor_lm_part(s)));
            const unsigned fold_grid = fold == kAnchorFoldExchange ? (unsigned)s->anchor_n : 1u;
            BB_HIP_CHECK(bb::launch(anchor_fold_kernel<T>, dim3(fold_grid), dim3(256), 0, s->stream, fold,
                                    (const double *)anchor_node_part(s), s->anchor_node_blocks,
                                    (const double *)anchor_lm_part(s), s->anchor_chunks, nodes,
                                    (T *)s->d_exch, bin_scale, s->L.n_pad, anchor_stress_ptr(s), stress_out));
            return BB_OK;
        });
    });
}

}  // namespace solver
}  // namespace bb

extern "C" {

// SPEC 2.5.5: the solver's own resident copy of the kept rows of `paths`, in its dtype.  All of
// the new state is built in locals and handed to the solver at the end: a refusal or a failed
// allocation leaves the solver as it was.
int bb_solver_set_anchors(bb_solver *s, const bb_paths *paths, const uint8_t *kept, double weight) {
    const char *who = "bb_solver_set_anchors";
    BB_REQUIRE(s != nullptr, "bb_solver_set_anchors: solver is NULL");
    BB_REQUIRE(std::isfinite(weight) && weight >= 0.0,
               "bb_solver_set_anchors: the weight must be finite and not negative");
    if (s->grad_pending)
        return bb::fail(BB_ERR_STATE, "bb_solver_set_anchors: a bb_solver_grad is pending");
    BB_TRY(bb::enter_device(s->device));
    if (paths == nullptr || weight == 0.0) {       // clear: every path is the unanchored one again
        BB_HIP_CHECK(hipStreamSynchronize(s->stream));
        s->anchor_rows.reset(), s->anchor_nodes.reset(), s->anchor_part.reset();
        s->anchor_n = 0, s->anchor_weight = 0.0, s->anchor_terms = 0;
        s->anchor_chunks = s->anchor_node_blocks = 0;
        return BB_OK;
    }
    if (s->world > 1)
        return bb::fail(BB_ERR_STATE, "bb_solver_set_anchors: landmark anchors run on one rank "
                                      "(world > 1: several devices are not covered)");
    if (s->n_maps > 1)
        return bb::fail(BB_ERR_STATE, "bb_solver_set_anchors: landmark anchors are for one map, not for "
                                      "a solver of several maps (bb_solver_set_maps)");
    BB_REQUIRE(paths->n_nodes == s->L.n_bins,
               "bb_solver_set_anchors: the paths have " + std::to_string(paths->n_nodes) +
                   " nodes, the solver " + std::to_string(s->L.n_bins) + " bins (n_nodes != n_bins)");
    BB_REQUIRE(paths->device == s->device, "bb_solver_set_anchors: the paths live on another device");
    std::vector<int> col, node;
    for (int64_t a = 0; a < paths->n_sources; ++a)
        if (kept == nullptr || kept[a]) {
            col.push_back((int)a);
            node.push_back((int)paths->sources[(size_t)a]);
        }
    BB_REQUIRE(!col.empty(), "bb_solver_set_anchors: fewer than 1 kept row");
    BB_REQUIRE((int)col.size() <= kAnchorMaxRows, "bb_solver_set_anchors: too many kept rows");
    {
        std::vector<int> sorted(node);
        std::sort(sorted.begin(), sorted.end());
        BB_REQUIRE(std::adjacent_find(sorted.begin(), sorted.end()) == sorted.end(),
                   "bb_solver_set_anchors: two kept rows have the same source node");
    }
    const int n_rows = (int)col.size();
    const int64_t es = bb::elem_size(s->dtype), n_pad = s->L.n_pad;
    const int node_blocks = (int)((s->L.n_bins + 255) / 256);
    const int chunks = (int)((s->L.n_bins + kAnchorChunk - 1) / kAnchorChunk);
    const size_t rows_bytes = (size_t)n_rows * (size_t)n_pad * (size_t)es;
    const size_t idx_bytes = bb::align256((size_t)n_rows * sizeof(int)) * 2 + 256;   // nodes | columns | count
    const size_t part_bytes =
        (size_t)(8 + bb::round_up(node_blocks, 8) + (int64_t)n_rows * chunks * 3) * sizeof(double);
    size_t free_b = 0, total_b = 0;
    BB_TRY(bb::hip_status(who, hipMemGetInfo(&free_b, &total_b)));
    const std::string sizes = std::to_string(n_rows) + " rows of " + std::to_string(n_pad) + " values need " +
                              std::to_string(rows_bytes) + " B and their sums " +
                              std::to_string(part_bytes + idx_bytes) + " B; " + std::to_string(free_b) +
                              " B are free";
    if (rows_bytes + part_bytes + idx_bytes > free_b) return bb::fail(BB_ERR_NOMEM, std::string(who) + ": " + sizes);
    bb::DevBuf rows, idx, part;
    hipError_t e = rows.alloc(rows_bytes);
    if (e == hipSuccess) e = idx.alloc(idx_bytes);
    if (e == hipSuccess) e = part.alloc(part_bytes);
    if (e != hipSuccess) return bb::fail(BB_ERR_NOMEM, std::string(who) + ": hipMalloc failed: " + sizes);
    int *d_node = idx.as<int>();
    int *d_col = (int *)((char *)idx.p + bb::align256((size_t)n_rows * sizeof(int)));
    unsigned long long *d_terms = (unsigned long long *)((char *)d_col + bb::align256((size_t)n_rows * sizeof(int)));
    unsigned long long terms = 0;
    BB_HIP_CHECK(hipStreamSynchronize(s->stream));
    BB_HIP_CHECK(hipMemcpy(d_node, node.data(), (size_t)n_rows * sizeof(int), hipMemcpyHostToDevice));
    BB_HIP_CHECK(hipMemcpy(d_col, col.data(), (size_t)n_rows * sizeof(int), hipMemcpyHostToDevice));
    BB_HIP_CHECK(hipMemsetAsync(d_terms, 0, sizeof(unsigned long long), s->stream));
    BB_HIP_CHECK(hipMemsetAsync(part.p, 0, part_bytes, s->stream));
    BB_TRY(by_dtype(s, [&](auto t) -> int {
        using T = typename decltype(t)::T;
        BB_HIP_CHECK(bb::launch(anchor_rows_kernel<T>, dim3((unsigned)(n_pad / 64), (unsigned)((n_rows + 63) / 64)),
                                dim3(256), 0, s->stream, paths->D.as<const double>(), paths->ld,
                                paths->n_nodes, n_pad, (const int *)d_col, n_rows, rows.as<T>(), d_terms));
        return BB_OK;
    }));
    BB_HIP_CHECK(hipStreamSynchronize(s->stream));
    BB_HIP_CHECK(hipMemcpy(&terms, d_terms, sizeof(terms), hipMemcpyDeviceToHost));
    s->anchor_rows = std::move(rows);
    s->anchor_nodes = std::move(idx);
    s->anchor_part = std::move(part);
    s->anchor_n = n_rows;
    s->anchor_weight = weight;
    s->anchor_terms = (int64_t)terms;
    s->anchor_chunks = chunks;
    s->anchor_node_blocks = node_blocks;
    return BB_OK;
}

int bb_solver_anchor_info(const bb_solver *s, int64_t *kept_rows, int64_t *terms, int64_t *bytes) {
    BB_REQUIRE(s != nullptr, "bb_solver_anchor_info: solver is NULL");
    if (kept_rows) *kept_rows = s->anchor_n;
    if (terms) *terms = s->anchor_terms;
    if (bytes) *bytes = (int64_t)(s->anchor_rows.bytes + s->anchor_nodes.bytes + s->anchor_part.bytes);
    return BB_OK;
}

// (bb_solver_anchor_sums is in bb_solver_queries.hip, with its two kernels: see bb_query_kernels.h)

int bb_solver_anchor_stress(bb_solver *s, double *stress) {
    BB_TRY(check_ready(s, "bb_solver_anchor_stress"));
    BB_REQUIRE(stress != nullptr, "bb_solver_anchor_stress: stress is NULL");
    *stress = 0.0;
    if (s->anchor_n == 0) return BB_OK;
    BB_TRY(bb::enter_device(s->device));
    BB_TRY(launch_anchors(s, kAnchorFoldAlone));
    BB_HIP_CHECK(hipStreamSynchronize(s->stream));
    BB_HIP_CHECK(hipMemcpy(stress, anchor_stress_ptr(s), sizeof(double), hipMemcpyDeviceToHost));
    return BB_OK;
}

int bb_solver_measure_anchors(bb_solver *s, int launches, double *ms_avg) {
    BB_TRY(check_ready(s, "bb_solver_measure_anchors"));
    BB_REQUIRE(ms_avg != nullptr, "bb_solver_measure_anchors: ms_avg is NULL");
    BB_REQUIRE(launches >= 1 && launches <= 1000, "bb_solver_measure_anchors: bad launches");
    if (s->anchor_n == 0) return bb::fail(BB_ERR_STATE, "bb_solver_measure_anchors: no anchors set");
    if (s->grad_pending)
        return bb::fail(BB_ERR_STATE, "bb_solver_measure_anchors: a bb_solver_grad is pending");
    BB_TRY(bb::enter_device(s->device));
    bb::StageClock<2> clock;
    BB_HIP_CHECK(clock.start());
    // (the exchange buffer holds nothing anybody waits for: no gradient is pending)
    BB_HIP_CHECK(hipMemsetAsync(s->d_exch, 0, (size_t)(3 * s->L.n_pad + 2) * bb::elem_size(s->dtype), s->stream));
    BB_TRY(launch_anchors(s, kAnchorFoldExchange));   // warm-up
    BB_HIP_CHECK(clock.mark(0, s->stream));
    for (int k = 0; k < launches; ++k) BB_TRY(launch_anchors(s, kAnchorFoldExchange));
    BB_HIP_CHECK(clock.mark(1, s->stream));
    BB_HIP_CHECK(hipStreamSynchronize(s->stream));
    double ms = 0.0;
    BB_HIP_CHECK(clock.read(0, &ms));
    *ms_avg = ms / launches;
    return BB_OK;
}

}  // extern "C"
