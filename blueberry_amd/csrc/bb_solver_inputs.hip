// bb_solver_inputs.hip -- the input routes of the 3D-structure solver: every writer of the
// units (a dense host matrix or a block of one, a device-resident ContactMap, sparse entries,
// resident Rao-format triples, coordinates, the re-exponentiation), what all of them do once
// the units are written (inputs_done: the row-owner path's full matrix, the 24-bit stream
// marked stale), and the bb_triples handle's create / destroy / tiles.  The kernels are in
// bb_input_kernels.h, compiled here and nowhere else.  The handle: bb_solver_internal.h.
// gfx950 only.
//
// Specification: docs/SPEC.md.  Data layout: DESIGN.md 3.
#include <algorithm>
#include <cmath>
#include <memory>

#include "bb_input_kernels.h"
#include "bb_solver_internal.h"
#include "bb_triples.h"

using namespace bb::solver;

namespace bb {
namespace solver {
namespace {

// The kind / alpha rule of every set_wish_* entry point, in who's name.
int check_kind_alpha(const char *who, int kind, double alpha) {
    BB_REQUIRE(kind == BB_KIND_WISH || kind == BB_KIND_COUNTS, std::string(who) + ": bad kind");
    BB_REQUIRE(kind == BB_KIND_WISH || alpha > 0.0, std::string(who) + ": alpha must be > 0");
    return BB_OK;
}

// What both ContactMap routes begin with: the kind / alpha rule in who's name, then the map's
// device matrix m (d x d) and its device.
struct CmMatrix {
    const double *m = nullptr;
    int64_t d = 0;
    int dev = -1;
};
int cm_matrix(const char *who, const bb_cm *cm, int kind, double alpha, CmMatrix *v) {
    BB_TRY(check_kind_alpha(who, kind, alpha));
    return bb_cm_device_ptr(cm, &v->m, &v->d, &v->dev);
}

// host = the (n_sub, n_sub) matrix of the bins [off, off + n_sub) of the solver (the whole
// map: off = 0, n_sub = n_bins); only units inside that block are touched
template <typename T, bool W>
int set_wish_dense_t(LayoutTag<T, W>, bb_solver *s, const double *host, int64_t ld, int kind, double alpha,
                     int64_t off, int64_t n_sub) {
    constexpr int VW = Lay<T, W>::VW;
    const int64_t upt = s->L.units_per_tile, n = off + n_sub;
    constexpr int64_t kRunTiles = 4;  // tiles staged per copy
    bb::DevBuf stage_buf;
    BB_TRY(bb::alloc_status(stage_buf, (size_t)(kRunTiles * VW * VW) * sizeof(double)));
    double *stage = stage_buf.as<double>();
    // Copy, convert and the next copy are all enqueued on the solver's stream,
    // so one staging buffer is enough and nothing depends on null-stream rules.
    int rc = BB_OK;
    int64_t ul = 0;
    while (ul < s->n_local && rc == BB_OK) {
        // a run: consecutive local units whose rows are consecutive in one strip
        const int j0 = s->udesc[ul].y;
        const int64_t i_start = s->udesc[ul].x;
        if (j0 < off || j0 >= n || i_start < off) { ++ul; continue; }      // another map's unit
        int64_t ue = ul + 1;
        while (ue < s->n_local && ue - ul < kRunTiles * upt && s->udesc[ue].y == j0 &&
               s->udesc[ue].x == i_start + (ue - ul) * s->L.rows_per_unit)
            ++ue;
        const int64_t rows = (ue - ul) * s->L.rows_per_unit;
        const int64_t rows_valid =
            std::max<int64_t>(0, std::min<int64_t>(i_start + rows, n) - i_start);
        const int64_t cols_valid =
            std::max<int64_t>(0, std::min<int64_t>((int64_t)j0 + VW, n) - j0);
        hipError_t e = hipSuccess;
        if (rows_valid < rows || cols_valid < VW)
            e = hipMemsetAsync(stage, 0, (size_t)rows * VW * sizeof(double), s->stream);
        if (e == hipSuccess && rows_valid > 0 && cols_valid > 0)
            e = hipMemcpy2DAsync(stage, VW * sizeof(double), host + (i_start - off) * ld + (j0 - off),
                                 (size_t)ld * sizeof(double), (size_t)cols_valid * sizeof(double),
                                 (size_t)rows_valid, hipMemcpyHostToDevice, s->stream);
        if (e == hipSuccess) {
            e = bb::launch(convert_units_kernel<T, W>, dim3((unsigned)(ue - ul)), dim3(256), 0,
                           s->stream, stage, (T *)s->d_units, s->d_udesc, ul, i_start, n, kind,
                           -1.0 / alpha);
        }
        if (e != hipSuccess)
            rc = bb::hip_status("set_wish_dense", e);
        ul = ue;
    }
    hipError_t e = hipStreamSynchronize(s->stream);
    if (rc == BB_OK && e != hipSuccess)
        rc = bb::hip_status("set_wish_dense", e);
    return rc;
}

// Row-owner path: rebuild both triangles from the freshly packed units.
int refresh_full(bb_solver *s) {
    if (!s->row_owner) return BB_OK;
    const int64_t es = bb::elem_size(s->dtype);
    BB_HIP_CHECK(hipMemsetAsync(s->d_full, 0, (size_t)(s->L.n_bins * s->full_ld * es), s->stream));
    if (s->n_local > 0)
        BB_TRY(by_layout(s, [&](auto lay) -> int {
            using T = typename decltype(lay)::T;
            BB_HIP_CHECK(bb::launch(units_to_full_kernel<T, decltype(lay)::W>, dim3((unsigned)s->n_local),
                                    dim3(256), 0, s->stream, (const T *)s->d_units, s->d_udesc,
                                    (T *)s->d_full, s->full_ld, s->L.n_bins));
            return BB_OK;
        }));
    BB_HIP_CHECK(hipStreamSynchronize(s->stream));
    return BB_OK;
}

// Every set_wish_*, once the units are packed on the solver's stream: rebuild the row-owner
// path's full matrix from them and mark the wish distances set.
int inputs_done(bb_solver *s) {
    BB_HIP_CHECK(hipStreamSynchronize(s->stream));
    BB_TRY(refresh_full(s));
    s->pk_stale = true;   // (every writer has said so before its first write; once more for a new one)
    s->have_wish = true;
    return BB_OK;
}

// The units from a ContactMap's device matrix m (d x d), whose bin 0 is the solver's bin off
// (the whole map: off = 0, d = n_bins).
int pack_from_cm(bb_solver *s, const double *m, int64_t d, int64_t off, int kind, double alpha) {
    BB_TRY(bb::enter_device(s->device));
    s->pk_stale = true;   // d_units is about to be written: whatever happens, the 24-bit stream is not of it
    if (s->n_local > 0)
        BB_TRY(by_layout(s, [&](auto lay) -> int {
            using T = typename decltype(lay)::T;
            BB_HIP_CHECK(bb::launch(pack_units_from_matrix_kernel<T, decltype(lay)::W>,
                                    dim3((unsigned)s->n_local), dim3(256), 0, s->stream, m, d,
                                    (T *)s->d_units, s->d_udesc, off + d, kind, -1.0 / alpha, off));
            return BB_OK;
        }));
    return inputs_done(s);
}

// host = the dense (n_sub, n_sub) block of the bins [off, off + n_sub), row stride ld
int set_wish_dense(bb_solver *s, const double *host, int64_t ld, int kind, double alpha, int64_t off,
                   int64_t n_sub) {
    BB_TRY(bb::enter_device(s->device));
    s->pk_stale = true;   // d_units is about to be written: whatever happens, the 24-bit stream is not of it
    BB_TRY(by_layout(s, [&](auto lay) { return set_wish_dense_t(lay, s, host, ld, kind, alpha, off, n_sub); }));
    return inputs_done(s);
}

// n entries (row, column, value) into the units (scatter_entries_kernel), chunk entries at a
// time: stage(k0, m, &src) enqueues what entries [k0, k0 + m) need on the solver's stream and
// describes them in src.  Every chunk runs in three phases -- clear / find the last entry per
// cell / store it -- on top of the earlier ones, so "the last entry wins" holds across chunks.
// Errors carry the caller's name, who; the caller has entered the solver's device.
template <typename Stage>
int scatter_entries(bb_solver *s, const char *who, int64_t n, int64_t chunk, int kind, double alpha,
                    const double *KRnorm, const double *KRexpected, Stage &&stage) {
    const auto hip = [&](hipError_t e) { return bb::hip_status(who, e); };
    const int64_t nb = s->L.n_blocks;
    std::vector<int32_t> tilemap((size_t)(nb * nb), -1);
    for (size_t t = 0; t < s->tile_I.size(); ++t)
        tilemap[(size_t)s->tile_I[t] * nb + s->tile_J[t]] = (int32_t)t;
    bb::DevBuf bmap, bbad, bkr, bke;
    if (bmap.alloc(tilemap.size() * 4) != hipSuccess || bbad.alloc(sizeof(int)) != hipSuccess ||
        (KRnorm && (bkr.alloc((size_t)s->L.n_bins * 8) != hipSuccess ||
                    bke.alloc((size_t)s->L.n_bins * 8) != hipSuccess)))
        return bb::fail(BB_ERR_NOMEM, std::string(who) + ": out of device memory");
    hipStream_t st = s->stream;
    BB_TRY(hip(hipMemcpyAsync(bmap.p, tilemap.data(), tilemap.size() * 4, hipMemcpyHostToDevice, st)));
    if (KRnorm) {
        BB_TRY(hip(hipMemcpyAsync(bkr.p, KRnorm, (size_t)s->L.n_bins * 8, hipMemcpyHostToDevice, st)));
        BB_TRY(hip(hipMemcpyAsync(bke.p, KRexpected, (size_t)s->L.n_bins * 8, hipMemcpyHostToDevice, st)));
    }
    s->pk_stale = true;   // d_units is about to be written: whatever happens, the 24-bit stream is not of it
    BB_TRY(hip(hipMemsetAsync(bbad.p, 0, sizeof(int), st)));
    BB_TRY(hip(hipMemsetAsync(s->d_units, 0, (size_t)std::max<int64_t>(s->n_local, 1) * bb::kUnitBytes, st)));
    for (int64_t k0 = 0; k0 < n; k0 += chunk) {
        const int64_t m = std::min(chunk, n - k0);
        EntrySrc src;
        BB_TRY(hip(stage(k0, m, &src)));
        for (int ph = 0; ph < 3; ++ph)
            BB_TRY(hip(by_layout(s, [&](auto lay) {
                using T = typename decltype(lay)::T;
                return bb::launch(scatter_entries_kernel<T, decltype(lay)::W>, dim3((unsigned)((m + 255) / 256)),
                                  dim3(256), 0, st, src, m, (const int32_t *)bmap.p, nb, s->L.n_bins,
                                  s->u_begin, s->u_end, (T *)s->d_units, kind, -1.0 / alpha,
                                  (const double *)bkr.p, (const double *)bke.p, (int *)bbad.p, ph);
            })));
    }
    BB_TRY(hip(hipStreamSynchronize(st)));
    int bad = 0;
    BB_TRY(hip(hipMemcpy(&bad, bbad.p, sizeof(int), hipMemcpyDeviceToHost)));
    if (bad == 1)
        return bb::fail(BB_ERR_INVALID, std::string(who) + ": an index is outside [0, n_bins)");
    if (bad == 2)
        return bb::fail(BB_ERR_INVALID, std::string(who) + ": an entry falls in a tile that is not in "
                                                           "the solver's tile list");
    return inputs_done(s);
}
}  // namespace
}  // namespace solver
}  // namespace bb

extern "C" {

int bb_solver_set_wish_dense(bb_solver *s, const double *host, int64_t ld, int kind,
                             double alpha) {
    BB_REQUIRE(s != nullptr && host != nullptr, "bb_solver_set_wish_dense: NULL argument");
    BB_REQUIRE(ld >= s->L.n_bins, "bb_solver_set_wish_dense: ld < n_bins");
    BB_TRY(check_kind_alpha("bb_solver_set_wish_dense", kind, alpha));
    return set_wish_dense(s, host, ld, kind, alpha, 0, s->L.n_bins);
}

// SPEC 2.11: the units re-exponentiated in place, then what every writer of the units does.
int bb_solver_repower(bb_solver *s, double p) {
    BB_REQUIRE(s != nullptr, "bb_solver_repower: solver is NULL");
    BB_REQUIRE(std::isfinite(p) && p > 0.0, "bb_solver_repower: p must be finite and > 0");
    if (!s->have_wish) return bb::fail(BB_ERR_STATE, "bb_solver_repower: no wish distances set");
    if (s->grad_pending) return bb::fail(BB_ERR_STATE, "bb_solver_repower: a bb_solver_grad is pending");
    if (s->anchor_n > 0)
        return bb::fail(BB_ERR_STATE, "bb_solver_repower: the solver holds landmark anchors, whose "
                                      "geodesic rows are not a power of anything");
    BB_TRY(bb::enter_device(s->device));
    s->pk_stale = true;   // d_units is about to be written: whatever happens, the 24-bit stream is not of it
    if (s->n_local > 0)
        BB_TRY(by_layout(s, [&](auto lay) -> int {
            using T = typename decltype(lay)::T;
            const int64_t n_words = s->n_local * (bb::kUnitBytes / (int64_t)sizeof(T));
            const unsigned grid = (unsigned)std::min<int64_t>((n_words + 255) / 256, 256 * 64);
            BB_HIP_CHECK(bb::launch(repower_units_kernel<T>, dim3(grid), dim3(256), 0, s->stream,
                                    (T *)s->d_units, n_words, p));
            return BB_OK;
        }));
    return inputs_done(s);
}

int bb_solver_set_wish_from_cm_block(bb_solver *s, const bb_cm *cm, int64_t bin_offset, int kind,
                                     double alpha) {
    BB_REQUIRE(s != nullptr && cm != nullptr, "bb_solver_set_wish_from_cm_block: NULL argument");
    CmMatrix v;
    BB_TRY(cm_matrix("bb_solver_set_wish_from_cm_block", cm, kind, alpha, &v));
    BB_REQUIRE(v.d >= 1 && bin_offset >= 0 && bin_offset % s->L.vw == 0 && bin_offset + v.d <= s->L.n_bins,
               "bb_solver_set_wish_from_cm_block: the map does not fit the solver at that offset");
    BB_REQUIRE(v.dev == s->device,
               "bb_solver_set_wish_from_cm_block: the map lives on another device than the solver");
    return pack_from_cm(s, v.m, v.d, bin_offset, kind, alpha);
}

int bb_solver_set_wish_dense_block(bb_solver *s, const double *host, int64_t ld, int64_t n_sub,
                                   int64_t bin_offset, int kind, double alpha) {
    BB_REQUIRE(s != nullptr && host != nullptr, "bb_solver_set_wish_dense_block: NULL argument");
    BB_REQUIRE(n_sub >= 1 && bin_offset >= 0 && bin_offset + n_sub <= s->L.n_bins && ld >= n_sub,
               "bb_solver_set_wish_dense_block: the block does not fit the solver");
    BB_REQUIRE(bin_offset % s->L.vw == 0,
               "bb_solver_set_wish_dense_block: a block starts at a multiple of the tile edge");
    BB_TRY(check_kind_alpha("bb_solver_set_wish_dense_block", kind, alpha));
    return set_wish_dense(s, host, ld, kind, alpha, bin_offset, n_sub);
}

int bb_solver_set_wish_from_cm(bb_solver *s, const bb_cm *cm, int kind, double alpha) {
    BB_REQUIRE(s != nullptr && cm != nullptr, "bb_solver_set_wish_from_cm: NULL argument");
    if (s->n_maps > 1)
        return bb::fail(BB_ERR_STATE, "bb_solver_set_wish_from_cm: a solver of several maps takes "
                                      "them one by one (bb_solver_set_wish_from_cm_block)");
    CmMatrix v;
    BB_TRY(cm_matrix("bb_solver_set_wish_from_cm", cm, kind, alpha, &v));
    BB_REQUIRE(v.d == s->L.n_bins,
               "bb_solver_set_wish_from_cm: the map's edge differs from the solver's n_bins");
    if (v.dev != s->device) {
        // a map on another GPU: the pack kernel reads it over peer access where the devices
        // allow it (one member of a group per device, each packing its own units from one map)
        int can = 0;
        if (hipDeviceCanAccessPeer(&can, s->device, v.dev) != hipSuccess) {
            (void)hipGetLastError();
            can = 0;
        }
        BB_REQUIRE(can, "bb_solver_set_wish_from_cm: the map lives on another device than the "
                        "solver, without peer access to it");
        BB_TRY(bb::enter_device(v.dev));
        BB_HIP_CHECK(hipDeviceSynchronize());          // the map's last operation has landed
        BB_TRY(bb::enter_device(s->device));
        BB_TRY(enable_peer_access("bb_solver_set_wish_from_cm: peer access", v.dev));
    }
    return pack_from_cm(s, v.m, v.d, 0, kind, alpha);
}

int bb_solver_set_wish_sparse(bb_solver *s, const int64_t *rows, const int64_t *cols,
                              const double *vals, int64_t nnz, int kind, double alpha,
                              const double *KRnorm, const double *KRexpected) {
    BB_REQUIRE(s != nullptr, "bb_solver_set_wish_sparse: solver is NULL");
    BB_REQUIRE(nnz >= 0 && (nnz == 0 || (rows && cols && vals)),
               "bb_solver_set_wish_sparse: NULL entries");
    BB_TRY(check_kind_alpha("bb_solver_set_wish_sparse", kind, alpha));
    BB_REQUIRE((KRnorm == nullptr) == (KRexpected == nullptr),
               "bb_solver_set_wish_sparse: KRnorm and KRexpected go together");
    BB_TRY(bb::enter_device(s->device));
    // host entries staged through device buffers of kChunk entries; the next chunk reuses them
    // in stream order
    constexpr int64_t kChunk = 1 << 22;
    const size_t cap = (size_t)std::max<int64_t>(1, std::min(nnz, kChunk)) * 8;
    bb::DevBuf brows, bcols, bvals;
    if (brows.alloc(cap) != hipSuccess || bcols.alloc(cap) != hipSuccess || bvals.alloc(cap) != hipSuccess)
        return bb::fail(BB_ERR_NOMEM, "bb_solver_set_wish_sparse: out of device memory");
    return scatter_entries(s, "bb_solver_set_wish_sparse", nnz, kChunk, kind, alpha, KRnorm, KRexpected,
                           [&](int64_t k0, int64_t m, EntrySrc *src) {
        *src = {(const int64_t *)brows.p, (const int64_t *)bcols.p, (const double *)bvals.p, nullptr, 0, 0, 1.0};
        hipError_t e = hipMemcpyAsync(brows.p, rows + k0, (size_t)m * 8, hipMemcpyHostToDevice, s->stream);
        if (e == hipSuccess)
            e = hipMemcpyAsync(bcols.p, cols + k0, (size_t)m * 8, hipMemcpyHostToDevice, s->stream);
        if (e == hipSuccess)
            e = hipMemcpyAsync(bvals.p, vals + k0, (size_t)m * 8, hipMemcpyHostToDevice, s->stream);
        return e;
    });
}

// ---- Rao-format triples resident on the device (fit_triples without host binning) --------
// (struct bb_triples: bb_triples.h, shared with bb_triples_balance.hip)
int bb_triples_create(bb_triples **out, const double *triples, int64_t n, int32_t resolution,
                      int32_t row_major, int device) {
    BB_REQUIRE(out != nullptr, "bb_triples_create: out is NULL");
    *out = nullptr;
    BB_REQUIRE(n >= 0 && (n == 0 || triples != nullptr), "bb_triples_create: NULL triples");
    BB_REQUIRE(resolution > 0, "bb_triples_create: resolution must be positive");
    BB_TRY(bb::use_device(device));
    std::unique_ptr<bb_triples> t(new (std::nothrow) bb_triples());
    if (!t) return bb::fail(BB_ERR_NOMEM, "bb_triples_create: out of host memory");
    t->device = device;
    t->n = n;
    t->resolution = (double)resolution;
    if (row_major) { t->st = 3; t->sc = 1; } else { t->st = 1; t->sc = n; }
    BB_TRY(bb::alloc_status(t->d, (size_t)(3 * n) * sizeof(double)));
    if (n > 0)
        BB_TRY(bb::hip_status("bb_triples_create",
                              hipMemcpy(t->d.p, triples, (size_t)n * 24, hipMemcpyHostToDevice)));
    *out = t.release();
    return BB_OK;
}

int bb_triples_destroy(bb_triples *t) {
    if (!t) return BB_OK;
    hipSetDevice(t->device);
    delete t;
    (void)hipGetLastError();
    return BB_OK;
}

int bb_triples_tiles(const bb_triples *t, int64_t n_bins, int dtype, uint8_t *present,
                     int64_t n_blocks) {
    BB_REQUIRE(t != nullptr && present != nullptr, "bb_triples_tiles: NULL argument");
    bb_layout_info L;
    BB_TRY(bb_layout_dense_info(n_bins, dtype, &L));
    BB_REQUIRE(n_blocks == L.n_blocks, "bb_triples_tiles: present must hold n_blocks^2 bytes of "
                                       "the layout of (n_bins, dtype)");
    BB_TRY(bb::enter_device(t->device));
    bb::DevBuf bp, bb_;
    if (bp.alloc((size_t)(n_blocks * n_blocks)) != hipSuccess || bb_.alloc(sizeof(int)) != hipSuccess)
        return bb::fail(BB_ERR_NOMEM, "bb_triples_tiles: out of device memory");
    BB_HIP_CHECK(hipMemset(bp.p, 0, (size_t)(n_blocks * n_blocks)));
    BB_HIP_CHECK(hipMemset(bb_.p, 0, sizeof(int)));
    constexpr int64_t kChunk = (int64_t)1 << 30;
    for (int64_t k0 = 0; k0 < t->n; k0 += kChunk) {
        const int64_t m = std::min(kChunk, t->n - k0);
        const EntrySrc src = {nullptr, nullptr, nullptr, t->from(k0), t->st, t->sc, t->resolution};
        BB_HIP_CHECK(bb::launch(entries_tiles_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0,
                                (hipStream_t) nullptr, src, m, L.vw, n_blocks, n_bins,
                                (unsigned char *)bp.p, (int *)bb_.p));
    }
    int bad = 0;
    BB_HIP_CHECK(hipMemcpy(&bad, bb_.p, sizeof(int), hipMemcpyDeviceToHost));
    BB_HIP_CHECK(hipMemcpy(present, bp.p, (size_t)(n_blocks * n_blocks), hipMemcpyDeviceToHost));
    if (bad) return bb::fail(BB_ERR_INVALID, "bb_triples_tiles: an index is outside [0, n_bins)");
    return BB_OK;
}

int bb_solver_set_wish_triples(bb_solver *s, const bb_triples *t, int kind, double alpha,
                               const double *KRnorm, const double *KRexpected) {
    BB_REQUIRE(s != nullptr && t != nullptr, "bb_solver_set_wish_triples: NULL argument");
    BB_TRY(check_kind_alpha("bb_solver_set_wish_triples", kind, alpha));
    BB_REQUIRE((KRnorm == nullptr) == (KRexpected == nullptr),
               "bb_solver_set_wish_triples: KRnorm and KRexpected go together");
    BB_REQUIRE(t->device == s->device,
               "bb_solver_set_wish_triples: the triples live on another device than the solver");
    BB_TRY(bb::enter_device(s->device));
    // slices of 2^30 entries of the device copy: an fp32 cell holds the index of the entry that
    // wins it in 32 bits
    constexpr int64_t kChunk = (int64_t)1 << 30;
    return scatter_entries(s, "bb_solver_set_wish_triples", t->n, kChunk, kind, alpha, KRnorm, KRexpected,
                           [&](int64_t k0, int64_t, EntrySrc *src) {
        *src = {nullptr, nullptr, nullptr, t->from(k0), t->st, t->sc, t->resolution};
        return hipSuccess;
    });
}

int bb_solver_set_wish_from_coords(bb_solver *s, const double *xstar) {
    BB_REQUIRE(s != nullptr && xstar != nullptr, "bb_solver_set_wish_from_coords: NULL argument");
    BB_TRY(bb::enter_device(s->device));
    BB_HIP_CHECK(upload_padded(s, s->d_f64_tmp, xstar, s->stream));
    s->pk_stale = true;   // d_units is about to be written: whatever happens, the 24-bit stream is not of it
    if (s->n_local > 0)
        BB_TRY(by_layout(s, [&](auto lay) -> int {
            using T = typename decltype(lay)::T;
            BB_HIP_CHECK(bb::launch(gen_units_kernel<T, decltype(lay)::W>, dim3((unsigned)s->n_local),
                                    dim3(256), 0, s->stream, s->d_f64_tmp, (T *)s->d_units, s->d_udesc,
                                    s->L.n_bins));
            return BB_OK;
        }));
    return inputs_done(s);
}
}  // extern "C"
