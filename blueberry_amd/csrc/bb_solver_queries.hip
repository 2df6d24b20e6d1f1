// bb_solver_queries.hip -- what is asked of a solver beside its iterations: the per-bin sums a
// step is made from (degrees, weight sums, the landmark rows' sums), the score of a fit
// (bb_score.hip's passes over this rank's units), the timing getters, the measurement probes
// (event gap, HBM read ceiling) and the facts about the 24-bit stream, the iteration path and
// the traffic.  The kernels are in bb_query_kernels.h, compiled here and nowhere else.  The
// handle: bb_solver_internal.h.  gfx950 only.
//
// Specification: docs/SPEC.md 2.4.1, 2.8, 2.11.
#include <algorithm>
#include <cmath>

#include "bb_query_kernels.h"
#include "bb_score.h"
#include "bb_solver_internal.h"

using namespace bb::solver;

namespace {
// One value of type V per bin, left by `launch(d_out)` -- enqueued on the solver's stream -- in
// the staging buffer of set_coords / get_coords (3 n_pad doubles >= n_bins values, nobody
// else's while the call runs: every user of it synchronises before it returns), to `host`.
template <typename V, typename Launch>
int per_bin_query(bb_solver *s, V *host, int64_t n_bins, Launch &&launch) {
    BB_TRY(bb::enter_device(s->device));
    V *d_out = (V *)s->d_f64_tmp;
    BB_TRY(launch(d_out));
    BB_HIP_CHECK(hipStreamSynchronize(s->stream));
    BB_HIP_CHECK(hipMemcpy(host, d_out, (size_t)n_bins * sizeof(V), hipMemcpyDeviceToHost));
    return BB_OK;
}
}  // namespace

extern "C" {

int bb_solver_degrees(bb_solver *s, int64_t *degree, int64_t n_bins) {
    BB_REQUIRE(s != nullptr && degree != nullptr, "bb_solver_degrees: NULL argument");
    BB_REQUIRE(n_bins == s->L.n_bins, "bb_solver_degrees: one count per bin");
    if (!s->have_wish) return bb::fail(BB_ERR_STATE, "bb_solver_degrees: no wish distances set");
    std::vector<int> host((size_t)n_bins);
    BB_TRY(per_bin_query(s, host.data(), n_bins, [&](int *d_deg) -> int {
        BB_HIP_CHECK(hipMemsetAsync(d_deg, 0, (size_t)s->L.n_pad * sizeof(int), s->stream));
        if (s->n_local == 0) return BB_OK;
        return by_layout(s, [&](auto lay) -> int {
            using T = typename decltype(lay)::T;
            BB_HIP_CHECK(bb::launch(unit_degrees_kernel<T, decltype(lay)::W>,
                                    dim3((unsigned)((s->n_local + kDegUnits - 1) / kDegUnits)), dim3(256),
                                    0, s->stream, (const T *)s->d_units, s->d_udesc, s->n_local,
                                    s->L.n_bins, d_deg));
            return BB_OK;
        });
    }));
    for (int64_t i = 0; i < n_bins; ++i) degree[i] = host[(size_t)i];
    return BB_OK;
}

int bb_solver_weight_sums(bb_solver *s, double *sums, int64_t n_bins) {
    BB_REQUIRE(s != nullptr && sums != nullptr, "bb_solver_weight_sums: NULL argument");
    BB_REQUIRE(n_bins == s->L.n_bins, "bb_solver_weight_sums: one sum per bin");
    if (!s->have_wish) return bb::fail(BB_ERR_STATE, "bb_solver_weight_sums: no wish distances set");
    if (s->weight_power == 0 || s->n_local == 0) {      // w = 1: the degrees, as doubles
        std::vector<int64_t> deg((size_t)n_bins, 0);
        if (s->n_local > 0) BB_TRY(bb_solver_degrees(s, deg.data(), n_bins));
        for (int64_t i = 0; i < n_bins; ++i) sums[i] = (double)deg[(size_t)i];
        return BB_OK;
    }
    const dim3 grid((unsigned)((n_bins + 3) / 4));
    return per_bin_query(s, sums, n_bins, [&](double *d_sum) {
        return by_layout(s, [&](auto lay) {
            using T = typename decltype(lay)::T;
            return with_int<1, 2>(s->weight_power, [&](auto q) -> int {
                BB_HIP_CHECK(bb::launch(unit_weight_sums_kernel<T, decltype(lay)::W, decltype(q)::value>, grid,
                                        dim3(256), 0, s->stream, (const T *)s->d_units, s->d_udesc, s->n_local,
                                        s->L.n_bins, d_sum));
                return BB_OK;
            });
        });
    });
}

int bb_solver_anchor_sums(bb_solver *s, double *sums, int64_t n_bins) {
    BB_REQUIRE(s != nullptr && sums != nullptr, "bb_solver_anchor_sums: NULL argument");
    BB_REQUIRE(n_bins == s->L.n_bins, "bb_solver_anchor_sums: one sum per bin");
    if (s->anchor_n == 0) {
        std::fill(sums, sums + n_bins, 0.0);
        return BB_OK;
    }
    return per_bin_query(s, sums, n_bins, [&](double *d_sum) {
        return by_dtype(s, [&](auto t) {
            using T = typename decltype(t)::T;
            return with_int<1, 2, 0>(s->weight_power, [&](auto qc) -> int {
                constexpr int Q = decltype(qc)::value;
                BB_HIP_CHECK(bb::launch(anchor_sums_node_kernel<T, Q>, dim3((unsigned)((n_bins + 255) / 256)),
                                        dim3(256), 0, s->stream, s->anchor_rows.as<const T>(), s->L.n_pad, n_bins,
                                        s->anchor_n, s->anchor_weight, d_sum));
                BB_HIP_CHECK(bb::launch(anchor_sums_landmark_kernel<T, Q>, dim3((unsigned)s->anchor_n), dim3(256), 0,
                                        s->stream, s->anchor_rows.as<const T>(), s->L.n_pad, n_bins,
                                        s->anchor_nodes.as<const int>(), s->anchor_weight, d_sum));
                return BB_OK;
            });
        });
    });
}

// SPEC 2.8: the sums a fit is judged by, over this rank's units.  The coordinates go through the
// staging buffer of set_coords / get_coords as float64 (the caller's, or the solver's own
// widened); the pass itself is bb_score.hip's and keeps what it allocates for the call only.
// Coordinates, velocity, stress history and per-bin steps are not touched.
// (who = the entry's name; bins NULL: the log-log sums of SPEC 2.11, whose profile has 7 columns)
static int score_or_loglog(bb_solver *s, const char *who, const double *xyz, double *profile, double *bins) {
    const std::string w(who);
    if (s->n_maps > 1) return bb::fail(BB_ERR_STATE, w + ": not for a solver of several maps");
    if (!s->have_wish) return bb::fail(BB_ERR_STATE, w + ": no wish distances set");
    if (s->grad_pending) return bb::fail(BB_ERR_STATE, w + ": a bb_solver_grad is pending");
    if (xyz == nullptr && !s->have_coords)
        return bb::fail(BB_ERR_STATE, w + ": no coordinates set");
    if (xyz != nullptr)
        for (int64_t q = 0; q < s->L.n_bins * 3; ++q)
            BB_REQUIRE(std::isfinite(xyz[q]), w + ": coordinates must be finite");
    BB_TRY(bb::enter_device(s->device));
    if (xyz != nullptr) BB_HIP_CHECK(upload_padded(s, s->d_f64_tmp, xyz, s->stream));
    else BB_HIP_CHECK(widen(s, s->d_X, s->d_f64_tmp, s->L.n_pad * 3));
    bb::ScoreInput in;
    in.dtype = s->dtype, in.wide = s->wide;
    in.n_bins = s->L.n_bins, in.n_local = s->n_local;
    in.d_units = s->d_units, in.d_udesc = s->d_udesc, in.udesc = s->udesc.data();
    in.d_xyz = s->d_f64_tmp, in.stream = s->stream;
    double *ms = s->timing ? s->score_ms : nullptr;
    const int rc = bins ? bb::score_pass(in, profile, bins, ms) : bb::loglog_pass(in, profile, ms);
    // (whatever happened, nothing of the call is left on the stream: the host arrays behind the
    // upload above belong to the caller)
    if (hipStreamSynchronize(s->stream) != hipSuccess && rc == BB_OK)
        return bb::fail(BB_ERR_HIP, w + ": the stream did not drain");
    return rc;
}

int bb_solver_score(bb_solver *s, const double *xyz, double *profile, double *bins) {
    BB_REQUIRE(s != nullptr && profile != nullptr && bins != nullptr, "bb_solver_score: NULL argument");
    return score_or_loglog(s, "bb_solver_score", xyz, profile, bins);
}

// SPEC 2.11: the log-log sums over the pairs of the score pass, by its kernels (bb_score.hip).
int bb_solver_loglog(bb_solver *s, const double *xyz, double *profile) {
    BB_REQUIRE(s != nullptr && profile != nullptr, "bb_solver_loglog: NULL argument");
    return score_or_loglog(s, "bb_solver_loglog", xyz, profile, nullptr);
}

int bb_solver_get_score_timing(bb_solver *s, double *profile_ms, double *fold_ms, double *bins_ms) {
    BB_REQUIRE(s != nullptr, "bb_solver_get_score_timing: solver is NULL");
    if (profile_ms) *profile_ms = s->score_ms[0];
    if (fold_ms) *fold_ms = s->score_ms[1];
    if (bins_ms) *bins_ms = s->score_ms[2];
    return BB_OK;
}

int bb_solver_get_timing(bb_solver *s, double *grad_ms_avg, double *reduce_ms_avg,
                         int64_t *launches) {
    BB_REQUIRE(s != nullptr, "bb_solver_get_timing: solver is NULL");
    BB_TRY(bb::enter_device(s->device));
    BB_HIP_CHECK(hipStreamSynchronize(s->stream));
    double g = 0.0, r = 0.0;
    const size_t n = s->ev_used / 3;
    for (size_t k = 0; k < n; ++k) {
        float a = 0.f, b = 0.f;
        BB_HIP_CHECK(hipEventElapsedTime(&a, s->ev[3 * k], s->ev[3 * k + 1]));
        BB_HIP_CHECK(hipEventElapsedTime(&b, s->ev[3 * k + 1], s->ev[3 * k + 2]));
        g += a;
        r += b;
    }
    if (grad_ms_avg) *grad_ms_avg = n ? g / n : 0.0;
    if (reduce_ms_avg) *reduce_ms_avg = n ? r / n : 0.0;
    if (launches) *launches = (int64_t)n;
    return BB_OK;
}

int bb_solver_get_step_timing(bb_solver *s, double *step_ms_avg) {
    BB_REQUIRE(s != nullptr && step_ms_avg != nullptr, "bb_solver_get_step_timing: NULL argument");
    BB_TRY(bb::enter_device(s->device));
    BB_HIP_CHECK(hipStreamSynchronize(s->stream));
    const size_t n = s->ev_used / 3;
    double t = 0.0;
    for (size_t k = 0; k + 1 < n; ++k) {
        float a = 0.f;
        BB_HIP_CHECK(hipEventElapsedTime(&a, s->ev[3 * k], s->ev[3 * k + 3]));
        t += a;
    }
    *step_ms_avg = n > 1 ? t / (double)(n - 1) / s->timing_stride : 0.0;
    return BB_OK;
}

int bb_solver_measure_event_gap(bb_solver *s, int pairs, double *ms_avg) {
    BB_REQUIRE(s != nullptr && ms_avg != nullptr, "bb_solver_measure_event_gap: NULL argument");
    BB_REQUIRE(pairs >= 1 && pairs <= 256, "bb_solver_measure_event_gap: bad pairs");
    BB_TRY(check_ready(s, "bb_solver_measure_event_gap"));
    BB_TRY(bb::enter_device(s->device));
    std::vector<bb::StageClock<2>> gap((size_t)pairs);   // a clock per pair: its one stage is empty
    hipError_t e = hipSuccess;
    for (bb::StageClock<2> &g : gap)
        if (e == hipSuccess) e = g.start();
    for (int k = 0; k < pairs && e == hipSuccess; ++k) {
        // behind a sweep launch, as the timed intervals are (the sweep only writes partials)
        if (!s->row_owner && launch_grad(s) != BB_OK) e = hipErrorUnknown;
        if (e == hipSuccess) e = gap[(size_t)k].mark(0, s->stream);
        if (e == hipSuccess) e = gap[(size_t)k].mark(1, s->stream);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
    double t = 0.0;
    for (int k = 0; k < pairs && e == hipSuccess; ++k) {
        double a = 0.0;
        e = gap[(size_t)k].read(0, &a);
        t += a;
    }
    BB_TRY(bb::hip_status("bb_solver_measure_event_gap", e));
    *ms_avg = t / pairs;
    return BB_OK;
}

int bb_solver_measure_stream_read(bb_solver *s, int launches, double *ms_avg) {
    BB_REQUIRE(s != nullptr && ms_avg != nullptr, "bb_solver_measure_stream_read: NULL argument");
    BB_REQUIRE(launches >= 1 && launches <= 1000, "bb_solver_measure_stream_read: bad launches");
    if (!s->have_wish)
        return bb::fail(BB_ERR_STATE, "bb_solver_measure_stream_read: no wish distances set");
    BB_TRY(bb::enter_device(s->device));
    bb::StageClock<2> clock;
    BB_HIP_CHECK(clock.start());
    if (s->dtype == BB_F32) BB_TRY(ensure_pk24(s));
    auto launch = [&]() {
        // what the sweep reads: the 24-bit stream when it is in use
        if (s->pk_valid)
            return bb::launch(s->nontemporal ? stream_read_pk24_kernel<true> : stream_read_pk24_kernel<false>,
                              dim3(s->n_waves / 4), dim3(256), 0, s->stream, s->pk_stream.as<const float4>(),
                              s->pk_table.as<const int4>(), (int)s->n_local, (int)(s->pk_bytes / 1024),
                              s->chunk_q, s->chunk_r, (float *)s->d_f64_tmp);
        return bb::launch(s->nontemporal ? stream_read_kernel<true> : stream_read_kernel<false>,
                          dim3(s->n_waves / 4), dim3(256), 0, s->stream,
                          (const float4 *)s->d_units, s->chunk_q, s->chunk_r,
                          (float *)s->d_f64_tmp);
    };
    BB_HIP_CHECK(launch());  // warm-up
    BB_HIP_CHECK(clock.mark(0, s->stream));
    for (int k = 0; k < launches; ++k) BB_HIP_CHECK(launch());
    BB_HIP_CHECK(clock.mark(1, s->stream));
    BB_HIP_CHECK(hipStreamSynchronize(s->stream));
    double ms = 0.0;
    BB_HIP_CHECK(clock.read(0, &ms));
    *ms_avg = ms / launches;
    return BB_OK;
}

int bb_solver_stream_info(bb_solver *s, int64_t *packed_units, int64_t *raw_units, int64_t *stream_bytes,
                          int64_t *format_switches) {
    BB_REQUIRE(s != nullptr, "bb_solver_stream_info: solver is NULL");
    if (!s->have_wish)
        return bb::fail(BB_ERR_STATE, "bb_solver_stream_info: no wish distances set");
    BB_TRY(bb::enter_device(s->device));
    BB_TRY(ensure_pk24(s));
    if (packed_units) *packed_units = s->pk_valid ? s->pk_packed : 0;
    if (raw_units) *raw_units = s->pk_valid ? s->n_local - s->pk_packed : s->n_local;
    if (stream_bytes) *stream_bytes = s->pk_valid ? s->pk_bytes : 0;
    if (format_switches) *format_switches = s->pk_valid ? s->pk_switches : 0;
    return BB_OK;
}

int bb_solver_iteration_path(const bb_solver *s, int *row_owner, int *waves_per_row) {
    BB_REQUIRE(s != nullptr, "bb_solver_iteration_path: solver is NULL");
    if (row_owner) *row_owner = s->row_owner ? 1 : 0;
    if (waves_per_row) *waves_per_row = s->row_owner ? s->ro_wpr : 0;
    return BB_OK;
}

int bb_solver_traffic(bb_solver *s, int64_t *unit_bytes, int64_t *pairs_dense) {
    BB_REQUIRE(s != nullptr, "bb_solver_traffic: solver is NULL");
    // the bytes a stress sweep reads: those of the 24-bit stream when it is in use
    if (s->have_wish && s->dtype == BB_F32) {
        BB_TRY(bb::enter_device(s->device));
        BB_TRY(ensure_pk24(s));
    }
    if (unit_bytes) *unit_bytes = s->pk_valid && !s->pk_stale ? s->pk_bytes : s->n_local * bb::kUnitBytes;
    if (pairs_dense) *pairs_dense = s->L.n_bins * (s->L.n_bins - 1) / 2;
    return BB_OK;
}
}  // extern "C"
