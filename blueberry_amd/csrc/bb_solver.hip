// bb_solver.hip -- host side of the 3D-structure solver of libblueberry_hip.so: the
// bb_solver handle's create / destroy (the partition itself is bb_solver_plan.cpp: no device
// call), kernel launches, the input routes, the multi-rank exchanges (RCCL, peer arenas) and
// the bb_solver_* / bb_comm_* entry points of include/blueberry_hip.h.  The kernels are in
// bb_solver_kernels.h.  The handle, and the parts of the solver that have a file of their own
// (landmark constraints, spectral start, groups): bb_solver_internal.h.  The environment is
// read in solver_env().  gfx950 only.
//
// Specification: docs/SPEC.md (build-authored; the reference has no solver,
// SURVEY.md section 0).  Data layout and kernel design: DESIGN.md 3-4.
#include <math.h>
#include <stddef.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <unistd.h>

#include <algorithm>
#include <cmath>
#include <map>
#include <memory>
#include <mutex>
#include <tuple>

#include "bb_score.h"
#include "bb_solver_internal.h"
#include "bb_solver_kernels.h"
#include "bb_triples.h"

using namespace bb::solver;

namespace {
void comm_release(bb_solver *s, bool destroy);   // the communicator cache, further down
}  // namespace

namespace bb {
namespace solver {

constexpr int64_t kHistCap = 1 << 20;
constexpr size_t kMaxTimedLaunches = 4096;

// The kind / alpha rule of every set_wish_* entry point, in who's name.
int check_kind_alpha(const char *who, int kind, double alpha) {
    BB_REQUIRE(kind == BB_KIND_WISH || kind == BB_KIND_COUNTS, std::string(who) + ": bad kind");
    BB_REQUIRE(kind == BB_KIND_WISH || alpha > 0.0, std::string(who) + ": alpha must be > 0");
    return BB_OK;
}

// (n_bins, 3) float64 rows of the host -> the (n_pad, 3) device buffer dst, its padding rows
// zero; both enqueued on `stream`.
hipError_t upload_padded(const bb_solver *s, double *dst, const double *rows, hipStream_t stream) {
    const hipError_t e = hipMemsetAsync(dst, 0, (size_t)s->L.n_pad * 3 * sizeof(double), stream);
    if (e != hipSuccess) return e;
    return hipMemcpyAsync(dst, rows, (size_t)s->L.n_bins * 3 * sizeof(double), hipMemcpyHostToDevice, stream);
}

// Peer access from the current device to `device`; "already enabled" is success, and what it
// leaves in the thread's error word is consumed here.  A failure reads "<who>: <HIP's text>".
int enable_peer_access(const char *who, int device) {
    const hipError_t e = hipDeviceEnablePeerAccess(device, 0);
    if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) return bb::hip_status(who, e);
    (void)hipGetLastError();
    return BB_OK;
}

// Every environment variable the solver reads, as they stand at the time of the call: at
// bb_solver_create the knobs of the sweep plan (bb_solver_plan.h) and of the 24-bit stream, the
// row-owner limit and the descriptor form; at bb_solver_peer_connect the peer ones.  THE place
// the solver reads its environment.
struct SolverEnv {
    bb::SweepKnobs knobs;          // BB_WAVES_PER_CU, BB_PAIR, BB_REDUCE_SLICES
    int pk_mode = -1;              // BB_PACK24: 0 never, 1 whenever a unit packs, unset: the rule
    int64_t pk_min_run = bb::kPk24MinRun;           // BB_PACK24_MIN_RUN
    // Largest map (bins) that iterates on the row-owner path.  Measured on MI355X
    // (tools/small_n_timing.py, profiles/archive/r02_small_n.txt); 0 turns the path off.
    int64_t row_owner_max = bb::kRowOwnerMaxBins;   // BB_ROW_OWNER_MAX
    bool arith_desc = true;        // BB_ARITH_DESC=0: the sweep loads a wave's first descriptor
    bool peer_mask = true;         // BB_PEER_MASK=0: all ranks send all blocks
    long long peer_timeout_ms = 10000;              // BB_PEER_TIMEOUT_MS
    int peer_fused = -1;           // BB_PEER_FUSED: 0 two launches, 1 one, unset (-1): by the GPUs
};
SolverEnv solver_env() {
    SolverEnv v;
    const auto off = [](const char *name) {   // set, and to 0
        const char *e = getenv(name);
        return e && atoi(e) == 0;
    };
    if (const char *e = getenv("BB_WAVES_PER_CU")) v.knobs.waves_per_cu = std::max(1, std::min(atoi(e), 32));
    v.knobs.pair = !off("BB_PAIR");
    if (const char *e = getenv("BB_REDUCE_SLICES")) v.knobs.reduce_slices = atoi(e) == 4 ? 4 : 8;
    if (const char *e = getenv("BB_PACK24")) v.pk_mode = atoi(e) != 0 ? 1 : 0;
    if (const char *e = getenv("BB_PACK24_MIN_RUN")) v.pk_min_run = std::max<int64_t>(1, atoll(e));
    if (const char *e = getenv("BB_ROW_OWNER_MAX")) v.row_owner_max = atoll(e);
    v.arith_desc = !off("BB_ARITH_DESC");
    v.peer_mask = !off("BB_PEER_MASK");
    if (const char *e = getenv("BB_PEER_TIMEOUT_MS"))
        if (atoll(e) > 0) v.peer_timeout_ms = atoll(e);
    if (const char *e = getenv("BB_PEER_FUSED")) v.peer_fused = atoi(e) != 0 ? 1 : 0;
    return v;
}

static_assert(bb::row_trip_cols(BB_F32) == RowTrip<float>::COLS && bb::row_trip_cols(BB_F64) == RowTrip<double>::COLS,
              "the plan's full_ld is a whole number of the row-owner kernel's trips");

// Build every index the kernels need from (tile list, unit range): the plan (bb_solver_plan.h),
// its copy in the handle, then the one allocation and the uploads.
int build_indices(bb_solver *s, const bb::SweepKnobs &knobs) {
    int cus = 256;
    hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, s->device);
    bb::SweepPlan p;
    BB_TRY(bb::sweep_plan("bb_solver_create", s->L, s->dtype, s->wide, s->tile_I.data(), s->tile_J.data(), s->u_begin, s->u_end,
                          cus, knobs, &p));
    s->n_local = p.n_local, s->t_first = p.t_first, s->n_local_tiles = p.n_local_tiles;
    s->udesc = std::move(p.udesc);
    s->n_waves = p.n_waves, s->wpb = p.wpb, s->chunk_q = p.chunk_q, s->chunk_r = p.chunk_r;
    s->nontemporal = p.nontemporal;
    s->defer_cap_units = p.defer_cap_units, s->lds_wave_floats = p.lds_wave_floats;
    s->defer_lds_bytes = p.defer_lds_bytes;
    s->slot_strip = std::move(p.slot_strip), s->wave_last_strip = std::move(p.wave_last_strip);
    s->n_slots = p.n_slots, s->rowpart_elems = p.rowpart_elems, s->colpart_elems = p.colpart_elems;
    s->red_slices = p.red_slices, s->red_stride = p.red_stride;
    s->full_ld = p.full_ld, s->ro_wpr = p.ro_wpr, s->ro_blocks = p.ro_blocks;
    s->hist_cap = kHistCap;

    const int64_t es = bb::elem_size(s->dtype), nw = p.n_waves;
    {
        // ONE device allocation for everything the solver owns (the exchange buffer apart:
        // a caller may replace it).  Twenty hipMalloc + hipFree pairs were 3 of the 4.5 ms a
        // whole chr21-sized fit took (tools/small_fit_timing.py).
        std::vector<std::pair<void **, size_t>> want;
        auto add = [&](auto **ptr, int64_t count) {
            want.push_back({(void **)ptr, (size_t)std::max<int64_t>(count, 1) * sizeof(**ptr)});
        };
        add((char **)&s->d_units, std::max<int64_t>(s->n_local, 1) * bb::kUnitBytes);
        add((char **)&s->d_X, s->L.n_pad * 3 * es);
        add((char **)&s->d_V, s->L.n_pad * 3 * es);
        add((char **)&s->d_part, p.part_total * es);
        add(&s->d_udesc, (int64_t)s->udesc.size());
        add(&s->d_wave_slots, nw);
        add(&s->d_stresspart, nw);
        add(&s->d_stress_slot, std::max<int64_t>(s->n_slots, 1));
        add(&s->d_red_lists, (int64_t)p.red_lists.size());
        add(&s->d_stress_hist, kHistCap);
        add(&s->d_stress_scalar, 1);
        add(&s->d_f64_tmp, s->L.n_pad * 3);
        if (s->row_owner) {
            add((char **)&s->d_full, s->L.n_bins * s->full_ld * es);
            add((char **)&s->d_X2, s->L.n_pad * 3 * es);
            add(&s->d_ro_part, 2 * (int64_t)s->ro_blocks);
        }
        size_t total = 0;
        for (auto &w : want) total += (w.second + 255) & ~(size_t)255;
        BB_TRY(bb::alloc_status(s->d_arena, total));
        size_t off = 0;
        for (auto &w : want) {
            *w.first = s->d_arena.as<char>() + off;
            off += (w.second + 255) & ~(size_t)255;
        }
    }
    BB_TRY(bb::alloc_status(s->own_exch, (size_t)((3 * s->L.n_pad + 2) * es)));
    s->d_exch = s->own_exch.p;

    hipStream_t st = s->stream;
    BB_HIP_CHECK(hipMemcpyAsync(s->d_udesc, s->udesc.data(), s->udesc.size() * sizeof(int2),
                                hipMemcpyHostToDevice, st));
    BB_HIP_CHECK(hipMemcpyAsync(s->d_wave_slots, p.wave_slots.data(), nw * sizeof(int2),
                                hipMemcpyHostToDevice, st));
    BB_HIP_CHECK(hipMemcpyAsync(s->d_red_lists, p.red_lists.data(),
                                p.red_lists.size() * sizeof(int64_t), hipMemcpyHostToDevice, st));
    // rows of boundary tiles owned by another rank are never written: keep them 0
    BB_HIP_CHECK(hipMemsetAsync(s->d_part, 0, (size_t)p.part_total * es, st));
    BB_HIP_CHECK(hipMemsetAsync(s->d_X, 0, (size_t)(s->L.n_pad * 3 * es), st));
    BB_HIP_CHECK(hipMemsetAsync(s->d_V, 0, (size_t)(s->L.n_pad * 3 * es), st));
    if (s->row_owner)
        BB_HIP_CHECK(hipMemsetAsync(s->d_X2, 0, (size_t)(s->L.n_pad * 3 * es), st));
    BB_HIP_CHECK(hipMemsetAsync(s->d_exch, 0, (size_t)((3 * s->L.n_pad + 2) * es), st));
    BB_HIP_CHECK(hipMemsetAsync(s->d_stresspart, 0, (size_t)nw * sizeof(double), st));
    // (shared slots -- the strip a wave ENDS in -- carry no stress of their own: they stay 0)
    BB_HIP_CHECK(hipMemsetAsync(s->d_stress_slot, 0,
                                (size_t)std::max<int64_t>(s->n_slots, 1) * sizeof(double), st));
    BB_HIP_CHECK(hipStreamSynchronize(st));  // the plan's host vectors die with this scope
    return BB_OK;
}

// The stream up to date with d_units (SPEC 3.7), or pk_valid = false: the sweep then reads
// d_units.  fp32 only; by default only where the sweep streams from HBM.  One pass for the
// smallest and largest word of every unit, the run rule and the offsets on the host
// (bb::pk24_table; one D2H of 8 bytes per unit, once per map), one pass that writes the stream.
int ensure_pk24(bb_solver *s) {
    if (!s->pk_stale) return BB_OK;
    s->pk_stale = false, s->pk_valid = false;
    s->pk_packed = s->pk_bytes = s->pk_switches = 0;
    const int64_t n = s->n_local;
    // Never where ranks share a GPU (a rehearsal: peer_ranks_on_gpu > 1).  The packed sweep takes
    // the registers of the one or two waves per SIMD it runs with; beside the waiting receive
    // kernels of the other ranks its workgroups find no CU to start on, and every rank waits for
    // a partial nobody can compute (tools/world8_rehearsal.py ran into its time limit that way).
    const bool want = s->dtype == BB_F32 && n > 0 && s->pk_mode != 0 && s->peer_ranks_on_gpu <= 1 &&
                      (s->pk_mode == 1 || s->nontemporal);
    if (!want) {
        s->pk_stream.reset(), s->pk_table.reset();
        return BB_OK;
    }
    bb::DevBuf d_minmax;
    if (d_minmax.alloc((size_t)n * sizeof(uint2)) != hipSuccess) return BB_OK;   // raw: no error
    BB_HIP_CHECK(bb::launch(pk24_minmax_kernel, dim3((unsigned)n), dim3(256), 0, s->stream,
                            (const uint4 *)s->d_units, d_minmax.as<uint2>()));
    std::vector<uint2> mm((size_t)n);
    BB_HIP_CHECK(hipMemcpyAsync(mm.data(), d_minmax.p, (size_t)n * sizeof(uint2), hipMemcpyDeviceToHost,
                                s->stream));
    BB_HIP_CHECK(hipStreamSynchronize(s->stream));
    bb::Pk24Table t;
    bb::pk24_table(mm.data(), s->udesc.data(), n, s->pk_min_run, s->pk_mode, &t);
    // 8 KiB behind the last unit: no refill address a body can form lies outside
    if (!t.pays || s->pk_stream.reserve((size_t)(t.kib + bb::kPk24RawKiB) * 1024) != hipSuccess ||
        s->pk_table.reserve((size_t)n * sizeof(int4)) != hipSuccess) {
        s->pk_stream.reset(), s->pk_table.reset();
        return BB_OK;                                                              // raw: no error
    }
    BB_HIP_CHECK(hipMemcpyAsync(s->pk_table.p, t.table.data(), (size_t)n * sizeof(int4), hipMemcpyHostToDevice,
                                s->stream));
    BB_HIP_CHECK(hipMemsetAsync(s->pk_stream.as<char>() + t.kib * 1024, 0, (size_t)bb::kPk24RawKiB * 1024,
                                s->stream));
    BB_HIP_CHECK(bb::launch(pk24_pack_kernel, dim3((unsigned)n), dim3(256), 0, s->stream,
                            (const uint4 *)s->d_units, s->pk_table.as<const int4>(), s->pk_stream.as<uint4>()));
    BB_HIP_CHECK(hipStreamSynchronize(s->stream));   // the host table dies with this scope
    s->pk_valid = true;
    s->pk_packed = t.packed, s->pk_bytes = t.kib * 1024, s->pk_switches = t.switches;
    return BB_OK;
}

// One instantiation of the sweep.  Its dynamic-LDS ceiling (row-sum parking and the column
// partials) is raised once: one bit of defer_attr_done per (WPB, NT, OP, PK).  THE place that
// takes the packed instantiation (PK: the fp32 stress sweep reading the 24-bit stream) when the
// stream is valid -- for iterate, grad, the peer and RCCL paths and the stress-only sweep alike.
// The matvec and the weighted sweeps keep reading d_units.
template <bool NT, int OP, int WPB, bool PK, typename T, bool W>
int launch_sweep_pk(LayoutTag<T, W>, bb_solver *s, const void *x_in);

template <bool NT, int OP, int WPB, typename T, bool W>
int launch_sweep(LayoutTag<T, W> lay, bb_solver *s, const void *x_in) {
    if constexpr (sizeof(T) == 4 && OP == kOpStress) {
        BB_TRY(ensure_pk24(s));
        if (s->pk_valid) return launch_sweep_pk<NT, OP, WPB, true>(lay, s, x_in);
    }
    return launch_sweep_pk<NT, OP, WPB, false>(lay, s, x_in);
}

template <bool NT, int OP, int WPB, bool PK, typename T, bool W>
int launch_sweep_pk(LayoutTag<T, W>, bb_solver *s, const void *x_in) {
    const auto kern = [] {
        if constexpr (PK) return stream24_grad_kernel<T, W, NT, OP, WPB>;
        else return stress_grad_kernel<T, W, NT, OP, WPB>;
    }();
    constexpr unsigned bit = 1u << ((WPB == 8 ? 4 : 0) + (NT ? 2 : 0) + (OP == kOpMatvec2 ? 1 : 0) +
                                    (OP == kOpStressW1 ? 8 : 0) + (OP == kOpStressW2 ? 16 : 0) + (PK ? 24 : 0));
    if (s->defer_lds_bytes > 0 && !(s->defer_attr_done & bit)) {
        BB_HIP_CHECK(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize,
                                         (int)s->defer_lds_bytes));
        s->defer_attr_done |= bit;
    }
    // row partials are indexed by local unit; the buffer starts at the rank's first tile
    T *rowpart = (T *)s->d_part +
                 (s->u_begin - s->t_first * s->L.units_per_tile) * (3 * s->L.rows_per_unit);
    T *colpart = (T *)s->d_part + s->rowpart_elems;
    BB_HIP_CHECK(bb::launch(kern, dim3(s->n_waves / s->wpb), dim3(64 * s->wpb), (size_t)s->defer_lds_bytes,
                            s->stream, PK ? s->pk_stream.as<const T>() : (const T *)s->d_units,
                            (const T *)x_in, PK ? s->pk_table.as<const int2>() : s->d_udesc, s->chunk_q,
                            s->chunk_r, s->d_wave_slots, rowpart, colpart, s->d_stresspart,
                            s->defer_cap_units, s->lds_wave_floats, s->dense_u0, s->d_stress_slot));
    return BB_OK;
}

// The sweep of OP with the solver's loads (nontemporal) and workgroup size (wpb): 8 waves per
// workgroup only for the 512-wide layouts (fp32, fp64 wide).
template <int OP, typename L>
int launch_sweep_op(L lay, bb_solver *s, const void *x_in) {
    constexpr int kPairWpb = sizeof(typename L::T) == 4 || L::W ? 8 : 4;
    return with_int<1, 0>(s->nontemporal ? 1 : 0, [&](auto nt) {
        return with_int<kPairWpb, 4>(s->wpb, [&](auto wpb) {
            return launch_sweep<decltype(nt)::value != 0, OP, decltype(wpb)::value>(lay, s, x_in);
        });
    });
}

template <typename T>
void fill_reduce_params(bb_solver *s, ReduceParams<T> &p, int mode, double lr, double *stress_out,
                        double scale);

// The peer exchange in one launch (reduce_exchange_kernel): the caller has bumped peer_seq.
template <typename T, bool W>
int launch_exchange_t(LayoutTag<T, W>, bb_solver *s, double lr, double *stress_out, double scale) {
    ReduceParams<T> p;
    fill_reduce_params<T>(s, p, kReducePeer, lr, stress_out, scale);
    const int64_t es = sizeof(T);
    const unsigned segs = 3 * Lay<T, W>::VW / kRedWG;
    const dim3 grid((unsigned)s->L.n_blocks, segs);
    const PeerTableX<T> *xt = s->d_peer_table_x.as<const PeerTableX<T>>() + (s->peer_seq & 1);
    const char *base = s->peer_arena.as<const char>();
    const T *arena = (const T *)(base + (int64_t)(s->peer_seq & 1) * s->world * s->peer_slot_elems * es);
    const unsigned long long *my_poison = (const unsigned long long *)(base + peer_xpoison_offset(s));
    return with_int<4, 8>(s->red_slices, [&](auto slices) -> int {
        constexpr int S = decltype(slices)::value;
        BB_HIP_CHECK(bb::launch(reduce_exchange_kernel<T, W, S>, grid, dim3(128 * S), 0, s->stream, p,
                                (const int64_t *)s->d_red_lists, s->red_stride, xt, arena, my_poison,
                                s->peer_slot_elems, s->d_peer_state.as<PeerState>(),
                                s->peer_limit_ticks));
        return BB_OK;
    });
}

template <typename T>
void fill_reduce_params(bb_solver *s, ReduceParams<T> &p, int mode, double lr, double *stress_out,
                        double scale) {
    p.part = (const T *)s->d_part;
    p.stresspart = s->d_stresspart;
    p.X = s->sum_target ? (T *)s->sum_target : (T *)s->d_X;
    p.V = (T *)s->d_V;
    p.mu = s->sum_target ? T(0) : (T)s->momentum;
    p.scale = (T)scale;
    p.exch = (T *)s->d_exch;
    p.stress_out = stress_out;
    p.n_pad = s->L.n_pad;
    p.n_waves = s->n_waves;
    p.lr = s->sum_target ? T(-1) : (T)lr;
    p.peer = nullptr;
    p.peer_counter = s->d_peer_counter.as<unsigned>();
    p.peer_state = s->d_peer_state.as<PeerState>();
    p.seq = 0;
    p.n_peers = 0;
    if (mode == kReducePeer) {
        // the caller has bumped peer_seq: iteration k (1-based) uses parity k & 1
        p.peer = s->d_peer_table.as<const PeerTable<T>>() + (s->peer_seq & 1);
        p.seq = s->peer_seq;
        p.n_peers = s->world;
    }
    p.mode = mode;
    p.stress_slot = s->d_stress_slot;
    p.n_slots = s->n_slots;
    // (a plain sum -- the matvec, the spectral start's products -- is never scaled)
    p.bin_scale = scale == kScalePlainSum ? nullptr : s->d_bin_scale.as<const T>();
    p.map_ptr = s->d_map_ptr.as<int>();
    p.map_idx = s->d_map_idx.as<int>();
    p.n_maps = s->n_maps;
    p.peer_mask = s->d_peer_mask.as<unsigned>();
    p.rank = s->rank;
}

template <typename T, bool W>
int launch_reduce_t(LayoutTag<T, W>, bb_solver *s, int mode, double lr, double *stress_out, double scale) {
    ReduceParams<T> p;
    fill_reduce_params<T>(s, p, mode, lr, stress_out, scale);
    const unsigned segs = 3 * Lay<T, W>::VW / kRedWG;   // workgroups per block of 3*vw elements
    // one launch: every list whole, 128 elements x 4 or 8 slices per workgroup
    const dim3 grid = mode == kReduceStressOnly ? dim3((unsigned)s->n_maps, 1)
                                                : dim3((unsigned)s->L.n_blocks, segs);
    return with_int<4, 8>(s->red_slices, [&](auto slices) -> int {
        constexpr int S = decltype(slices)::value;
        BB_HIP_CHECK(bb::launch(reduce_sliced_kernel<T, W, S>, grid, dim3(128 * S), 0, s->stream,
                                p, (const int64_t *)s->d_red_lists, s->red_stride));
        return BB_OK;
    });
}

int launch_grad(bb_solver *s, int op, const void *x_in) {
    if (!x_in) x_in = s->d_X;
    // the stress and its gradient: weighted (SPEC 2.3.1) once a weight power is set
    if (op == kOpStress && s->weight_power != 0)
        op = s->weight_power == 1 ? kOpStressW1 : kOpStressW2;
    return by_layout(s, [&](auto lay) {
        return with_int<kOpMatvec2, kOpStressW1, kOpStressW2, kOpStress>(op, [&](auto opc) {
            return launch_sweep_op<decltype(opc)::value>(lay, s, x_in);
        });
    });
}
int launch_reduce(bb_solver *s, int mode, double lr, double *stress_out, double scale) {
    return by_layout(s, [&](auto lay) { return launch_reduce_t(lay, s, mode, lr, stress_out, scale); });
}
int launch_exchange(bb_solver *s, double lr, double *stress_out, double scale) {
    return by_layout(s, [&](auto lay) { return launch_exchange_t(lay, s, lr, stress_out, scale); });
}

// X <- X + V, V <- mu V - lr * exchange[0 : 3 n_pad]; the stress of the buffer to stress_out.
int launch_apply(bb_solver *s, double lr, double *stress_out) {
    const int64_t n3 = s->L.n_pad * 3;
    return by_dtype(s, [&](auto t) -> int {
        using T = typename decltype(t)::T;
        BB_HIP_CHECK(bb::launch(apply_kernel<T>, dim3((unsigned)((n3 + 255) / 256)), dim3(256), 0, s->stream,
                                (T *)s->d_X, (T *)s->d_V, (const T *)s->d_exch, n3, (T)lr, (T)s->momentum,
                                stress_out));
        return BB_OK;
    });
}

int check_ready(const bb_solver *s, const char *who) {
    if (!s) return bb::fail(BB_ERR_INVALID, std::string(who) + ": solver is NULL");
    if (!s->have_wish)
        return bb::fail(BB_ERR_STATE, std::string(who) + ": no wish distances set");
    if (!s->have_coords)
        return bb::fail(BB_ERR_STATE, std::string(who) + ": no coordinates set");
    return BB_OK;
}

// What every entry point that iterates checks before it enqueues anything: the solver is
// ready, iters >= 0, and the stress history (n_maps values per iteration) has room for all of
// the call -- (hist_n + iters) * n_maps <= hist_cap, in a form that cannot overflow.
int check_iterate(const bb_solver *s, int64_t iters, const char *who) {
    BB_TRY(check_ready(s, who));
    BB_REQUIRE(iters >= 0, std::string(who) + ": iters < 0");
    if (iters > s->hist_cap / s->n_maps - s->hist_n)
        return bb::fail(BB_ERR_STATE, std::string(who) + ": stress history full");
    return BB_OK;
}

// f64 <-> solver dtype conversions of n elements on the solver's stream.
hipError_t widen(bb_solver *s, const void *in_T, double *out_f64, int64_t n) {
    return by_dtype(s, [&](auto t) {
        using T = typename decltype(t)::T;
        return bb::launch(T_to_f64_kernel<T>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s->stream,
                          (const T *)in_T, out_f64, n);
    });
}
hipError_t narrow(bb_solver *s, const double *in_f64, void *out_T, int64_t n) {
    return by_dtype(s, [&](auto t) {
        using T = typename decltype(t)::T;
        return bb::launch(f64_to_T_kernel<T>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s->stream,
                          in_f64, (T *)out_T, n);
    });
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

// n_pad factors (float64 on the host) -> d_bin_scale in the solver's type.
int upload_bin_scale(bb_solver *s, const double *padded) {
    const int64_t n = s->L.n_pad, es = bb::elem_size(s->dtype);
    std::vector<char> host((size_t)(n * es));
    for (int64_t i = 0; i < n; ++i) {
        if (s->dtype == BB_F32) ((float *)host.data())[i] = (float)padded[i];
        else ((double *)host.data())[i] = padded[i];
    }
    BB_HIP_CHECK(hipStreamSynchronize(s->stream));
    if (!s->d_bin_scale) BB_TRY(bb::alloc_status(s->d_bin_scale, (size_t)(n * es)));
    BB_HIP_CHECK(hipMemcpy(s->d_bin_scale.p, host.data(), host.size(), hipMemcpyHostToDevice));
    return BB_OK;
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

// One row-owner launch: iteration `hist_n` (reads d_X, writes d_X2, swaps them) and the
// fold of the previous launch's stress into hist[hist_n - 1] when `fold_prev`.
// update = false: fold only (after the last iteration of a call).
int launch_row_owner(bb_solver *s, double lr, bool fold_prev, bool update) {
    const int par = (int)(s->ro_launches & 1);
    const double *prev = s->d_ro_part + (int64_t)(par ^ 1) * s->ro_blocks;
    double *out = s->d_ro_part + (int64_t)par * s->ro_blocks;
    double *hist_prev = fold_prev ? s->d_stress_hist + (s->hist_n - 1) : nullptr;
    // fold only: a grid of one workgroup, which is then the "last" = the fold workgroup
    const unsigned grid = update ? (unsigned)s->ro_blocks + 1u : 1u;
    // waves per row 4, 2 or 1; weight power q = 1, 2 or 0
    BB_TRY(by_dtype(s, [&](auto t) {
        using T = typename decltype(t)::T;
        return with_int<4, 2, 1>(s->ro_wpr, [&](auto wpr) {
            return with_int<1, 2, 0>(s->weight_power, [&](auto q) -> int {
                BB_HIP_CHECK(bb::launch(row_owner_kernel<T, decltype(wpr)::value, decltype(q)::value>,
                                        dim3(grid), dim3(256), 0, s->stream, (const T *)s->d_full,
                                        s->full_ld, (int)s->L.n_bins, (const T *)s->d_X, (T *)s->d_X2,
                                        (T *)s->d_V, (T)lr, (T)s->momentum, prev, s->ro_blocks, hist_prev,
                                        out, s->d_bin_scale.as<const T>()));
                return BB_OK;
            });
        });
    }));
    if (update) {
        std::swap(s->d_X, s->d_X2);
        s->ro_launches++;
    }
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

}  // namespace solver
}  // namespace bb

// ---- peer exchange ---------------------------------------------------------
namespace bb {
namespace solver {

// What travels between ranks: the IPC handle of the arena plus what is needed to
// check that both sides agree on its shape (and to short-cut ranks that live in
// the same process, where an IPC handle cannot be opened).
struct PeerHandle {
    hipIpcMemHandle_t ipc;   // 64 bytes
    uint64_t magic;
    int64_t arena_bytes, slot_elems;
    int64_t pid;
    uint64_t raw;            // the exporter's own pointer (same-process ranks only)
    int32_t rank, world, dtype, device;
    uint64_t pci;            // PCI domain << 32 | bus << 16 | device: which GPU, whatever its index
};
static_assert(sizeof(PeerHandle) <= BB_PEER_HANDLE_BYTES, "handle blob too small");
static_assert(offsetof(PeerTable<float>, flag) == kMaxPeers * sizeof(void *) &&
                  offsetof(PeerTable<double>, flag) == kMaxPeers * sizeof(void *),
              "peer_receive_kernel takes the flag pointers as the second half of a PeerTable");
constexpr uint64_t kPeerMagic = 0x6262706565723031ull;  // "bbpeer01"

// Block b -> bit q set when rank q of `world` holds a unit of a tile in block row or column b:
// the ranks whose partial for b is not zero by construction.  Every rank derives it alike from
// the tile list and the partition; the peer exchange and a group's group_apply_kernel both
// read it, and the two stay bit-identical only through this one table.
int contributor_mask(const bb_solver *s, std::vector<unsigned> *mask) {
    mask->assign((size_t)s->L.n_blocks, 0u);
    const int64_t upt = s->L.units_per_tile;
    for (int q = 0; q < s->world; ++q) {
        int64_t ub = 0, ue = 0;
        BB_TRY(bb_layout_rank_units(s->L.n_units, q, s->world, &ub, &ue));
        if (ue <= ub) continue;
        for (int64_t t = ub / upt; t <= (ue - 1) / upt; ++t) {
            (*mask)[(size_t)s->tile_I[(size_t)t]] |= 1u << q;
            (*mask)[(size_t)s->tile_J[(size_t)t]] |= 1u << q;
        }
    }
    return BB_OK;
}

template <typename T>
int build_peer_tables(TypeTag<T>, bb_solver *s) {
    PeerTable<T> tab[2];
    memset(tab, 0, sizeof(tab));
    const int64_t foff = peer_flags_offset(s);
    for (int par = 0; par < 2; ++par)
        for (int q = 0; q < s->world; ++q) {
            char *base = (char *)s->peer_mapped[q];
            tab[par].dst[q] = (T *)base + ((int64_t)par * s->world + s->rank) * s->peer_slot_elems;
            tab[par].flag[q] = (unsigned long long *)(base + foff) + 8 * s->rank;
        }
    BB_TRY(bb::alloc_status(s->d_peer_table, sizeof(tab)));
    BB_HIP_CHECK(hipMemcpy(s->d_peer_table.p, tab, sizeof(tab), hipMemcpyHostToDevice));
    PeerTableX<T> tx[2];
    memset(tx, 0, sizeof(tx));
    for (int par = 0; par < 2; ++par)
        for (int q = 0; q < s->world; ++q) {
            char *base = (char *)s->peer_mapped[q];
            tx[par].dst[q] = tab[par].dst[q];
            tx[par].poison[q] = (unsigned long long *)(base + peer_xpoison_offset(s)) + 8 * s->rank;
        }
    BB_TRY(bb::alloc_status(s->d_peer_table_x, sizeof(tx)));
    BB_HIP_CHECK(hipMemcpy(s->d_peer_table_x.p, tx, sizeof(tx), hipMemcpyHostToDevice));
    return BB_OK;
}

}  // namespace solver
}  // namespace bb

extern "C" {

int bb_solver_create(bb_solver **out, int64_t n_bins, int dtype, int device, int rank, int world,
                     const int32_t *tile_I, const int32_t *tile_J, int64_t n_tiles) {
    BB_REQUIRE(out != nullptr, "bb_solver_create: out is NULL");
    *out = nullptr;
    BB_REQUIRE(dtype == BB_F32 || dtype == BB_F64, "bb_solver_create: bad dtype");
    BB_REQUIRE(n_bins >= 2, "bb_solver_create: n_bins must be >= 2");
    BB_REQUIRE(n_bins <= (int64_t)700000000, "bb_solver_create: n_bins too large");
    BB_REQUIRE(world >= 1 && rank >= 0 && rank < world, "bb_solver_create: bad rank/world");
    BB_REQUIRE((tile_I == nullptr) == (tile_J == nullptr) && (tile_I != nullptr || n_tiles == 0),
               "bb_solver_create: tile_I/tile_J/n_tiles inconsistent");
    BB_TRY(bb::use_device(device));

    bb_solver *s = new (std::nothrow) bb_solver();
    if (!s) return bb::fail(BB_ERR_NOMEM, "bb_solver_create: out of host memory");
    s->dtype = dtype;
    s->device = device;
    s->rank = rank;
    s->world = world;
    int rc = bb_layout_dense_info(n_bins, dtype, &s->L);
    s->wide = bb::wide_layout(dtype, n_bins);
    const SolverEnv env = solver_env();
    s->row_owner = s->row_owner_built = world == 1 && n_bins <= env.row_owner_max;
    s->pk_mode = env.pk_mode, s->pk_min_run = env.pk_min_run;
    if (rc == BB_OK) {
        if (tile_I == nullptr) {
            s->tile_I.resize((size_t)s->L.n_tiles);
            s->tile_J.resize((size_t)s->L.n_tiles);
            rc = bb_layout_dense_tiles(n_bins, dtype, s->tile_I.data(), s->tile_J.data(),
                                       s->L.n_tiles);
        } else {
            rc = bb::check_tile_list("bb_solver_create", s->L, tile_I, tile_J, n_tiles);
            s->tile_I.assign(tile_I, tile_I + n_tiles);
            s->tile_J.assign(tile_J, tile_J + n_tiles);
            s->L.n_tiles = n_tiles;
            s->L.n_units = n_tiles * s->L.units_per_tile;
        }
    }
    if (rc == BB_OK) rc = bb_layout_rank_units(s->L.n_units, rank, world, &s->u_begin, &s->u_end);
    if (rc == BB_OK && tile_I == nullptr && s->u_end < ((int64_t)1 << 31) && env.arith_desc)
        s->dense_u0 = (int)s->u_begin;
    if (rc == BB_OK) {
        hipError_t e = bb::acquire_stream(device, &s->stream);
        if (e != hipSuccess)
            rc = bb::hip_status("hipStreamCreate", e);
        else
            s->own_stream = true;
    }
    if (rc == BB_OK) {
        bb::SweepKnobs knobs = env.knobs;
        knobs.row_owner = s->row_owner;
        rc = build_indices(s, knobs);
    }
    if (rc != BB_OK) return failed_create(rc, [&] { bb_solver_destroy(s); });
    *out = s;
    return BB_OK;
}

int bb_solver_destroy(bb_solver *s) {
    if (!s) return BB_OK;
    hipSetDevice(s->device);
    if (!s->stream_stuck && (s->stream || !s->own_stream)) hipStreamSynchronize(s->stream);
    if (s->comm) {
        bb::Rccl::Comm c = s->comm;
        const bool cached = s->comm_cached, suspect = s->comm_suspect;
        comm_release(s, /*destroy=*/false);  // a cached communicator goes back to the cache ...
        if (suspect) {                       // ... unless a collective on it failed: out of the
            if (bb::rccl().CommAbort) bb::rccl().CommAbort(c);   // cache (comm_release) and ended
        } else if (!cached) {
            bb::rccl().CommDestroy(c);
        }
    }
    for (void *m : s->peer_opened) hipIpcCloseMemHandle(m);
    // buffers and events go with the handle, the stream back to the pool after them (one
    // abandoned behind a hung collective does not: the pool synchronises what it takes back)
    const int device = s->device;
    hipStream_t pooled = s->own_stream && !s->stream_stuck ? s->stream : nullptr;
    delete s;
    if (pooled) bb::release_stream(device, pooled);
    // tear-down is best effort (a free can fail when a peer process has already gone
    // away): whatever it left in the thread's error word is consumed here
    (void)hipGetLastError();
    return BB_OK;
}

int bb_solver_set_stream(bb_solver *s, void *hip_stream) {
    BB_REQUIRE(s != nullptr, "bb_solver_set_stream: solver is NULL");
    BB_TRY(bb::enter_device(s->device));
    BB_HIP_CHECK(hipStreamSynchronize(s->stream));
    if (s->own_stream && s->stream) bb::release_stream(s->device, s->stream);
    s->stream = (hipStream_t)hip_stream;
    s->own_stream = false;
    return BB_OK;
}

int bb_solver_layout(const bb_solver *s, bb_layout_info *info, int64_t *u_begin, int64_t *u_end) {
    BB_REQUIRE(s != nullptr, "bb_solver_layout: solver is NULL");
    if (info) *info = s->L;
    if (u_begin) *u_begin = s->u_begin;
    if (u_end) *u_end = s->u_end;
    return BB_OK;
}

int bb_solver_set_wish_dense(bb_solver *s, const double *host, int64_t ld, int kind,
                             double alpha) {
    BB_REQUIRE(s != nullptr && host != nullptr, "bb_solver_set_wish_dense: NULL argument");
    BB_REQUIRE(ld >= s->L.n_bins, "bb_solver_set_wish_dense: ld < n_bins");
    BB_TRY(check_kind_alpha("bb_solver_set_wish_dense", kind, alpha));
    return set_wish_dense(s, host, ld, kind, alpha, 0, s->L.n_bins);
}

int bb_solver_set_maps(bb_solver *s, int n_maps, const int64_t *bin_begin, const double *lr_scale) {
    BB_REQUIRE(s != nullptr && bin_begin != nullptr && lr_scale != nullptr,
               "bb_solver_set_maps: NULL argument");
    BB_REQUIRE(n_maps >= 1 && n_maps <= s->L.n_blocks, "bb_solver_set_maps: bad n_maps");
    if (s->anchor_n > 0)
        return bb::fail(BB_ERR_STATE, "bb_solver_set_maps: the solver holds landmark anchors, which are "
                                      "for one map (clear them with bb_solver_set_anchors first)");
    if (s->world != 1)
        return bb::fail(BB_ERR_STATE, "bb_solver_set_maps: one rank only (on several GPUs give every "
                                      "rank maps of its own)");
    const int64_t vw = s->L.vw, nb = s->L.n_blocks;
    BB_REQUIRE(bin_begin[0] == 0 && bin_begin[n_maps] == s->L.n_bins,
               "bb_solver_set_maps: bin_begin must run from 0 to n_bins");
    for (int m = 0; m < n_maps; ++m)
        BB_REQUIRE(bin_begin[m] % vw == 0 && bin_begin[m + 1] > bin_begin[m],
                   "bb_solver_set_maps: every map starts at a multiple of the tile edge and is not empty");
    BB_TRY(bb::enter_device(s->device));
    std::vector<int> map_of_block((size_t)nb, 0);
    for (int m = 0, b = 0; b < nb; ++b) {
        while (m + 1 < n_maps && (int64_t)b * vw >= bin_begin[m + 1]) ++m;
        map_of_block[(size_t)b] = m;
    }
    for (size_t t = 0; t < s->tile_I.size(); ++t)
        BB_REQUIRE(map_of_block[(size_t)s->tile_I[t]] == map_of_block[(size_t)s->tile_J[t]],
                   "bb_solver_set_maps: a tile of the solver's list joins two maps");
    // per bin: its map's step; per map: its stress partials (wave w's own, index w, belongs
    // to the strip the wave ends in; slot q's, index n_waves + q, to the slot's strip)
    std::vector<double> scale((size_t)s->L.n_pad);
    for (int64_t i = 0; i < s->L.n_pad; ++i) scale[(size_t)i] = lr_scale[map_of_block[(size_t)(i / vw)]];
    std::vector<std::vector<int>> lists((size_t)n_maps);
    for (int w = 0; w < s->n_waves; ++w)
        if (s->wave_last_strip[(size_t)w] >= 0)
            lists[(size_t)map_of_block[(size_t)s->wave_last_strip[(size_t)w]]].push_back(w);
    for (int q = 0; q < s->n_slots; ++q)
        lists[(size_t)map_of_block[(size_t)s->slot_strip[(size_t)q]]].push_back(s->n_waves + q);
    std::vector<int> ptr(1, 0), idx;
    for (auto &l : lists) {
        idx.insert(idx.end(), l.begin(), l.end());
        ptr.push_back((int)idx.size());
    }
    if (idx.empty()) idx.push_back(0);
    s->d_bin_scale.reset(); s->d_map_ptr.reset(); s->d_map_idx.reset(); s->d_map_scalar.reset();
    s->bin_steps = false;          // (the maps' steps replace a bb_solver_set_bin_steps)
    s->n_maps = 1;                 // (what holds if an allocation below fails: one map, no tables)
    s->map_begin.clear();
    BB_TRY(upload_bin_scale(s, scale.data()));
    BB_TRY(bb::alloc_status(s->d_map_ptr, ptr.size() * sizeof(int)));
    BB_TRY(bb::alloc_status(s->d_map_idx, idx.size() * sizeof(int)));
    BB_TRY(bb::alloc_status(s->d_map_scalar, (size_t)n_maps * sizeof(double)));
    BB_HIP_CHECK(hipMemcpy(s->d_map_ptr.p, ptr.data(), ptr.size() * sizeof(int), hipMemcpyHostToDevice));
    BB_HIP_CHECK(hipMemcpy(s->d_map_idx.p, idx.data(), idx.size() * sizeof(int), hipMemcpyHostToDevice));
    // (a map that is never set carries no constraint)
    s->pk_stale = true;   // d_units is about to be written: whatever happens, the 24-bit stream is not of it
    BB_HIP_CHECK(hipMemsetAsync(s->d_units, 0, (size_t)std::max<int64_t>(s->n_local, 1) * bb::kUnitBytes,
                                s->stream));
    BB_HIP_CHECK(hipStreamSynchronize(s->stream));
    s->n_maps = n_maps;
    s->map_begin.assign(bin_begin, bin_begin + n_maps + 1);
    s->row_owner = false;          // the sweep: its reduce knows the maps
    s->hist_n = 0;
    return BB_OK;
}

int bb_solver_set_bin_steps(bb_solver *s, const double *scale, int64_t n_bins) {
    BB_REQUIRE(s != nullptr, "bb_solver_set_bin_steps: solver is NULL");
    if (s->n_maps > 1 && scale == nullptr)
        return bb::fail(BB_ERR_STATE, "bb_solver_set_bin_steps: a solver of several maps always has "
                                      "factors (bb_solver_set_maps sets each map's; pass new ones)");
    if (s->grad_pending)
        return bb::fail(BB_ERR_STATE, "bb_solver_set_bin_steps: a bb_solver_grad is pending");
    BB_TRY(bb::enter_device(s->device));
    if (scale == nullptr) {                       // back to one step for all
        BB_HIP_CHECK(hipStreamSynchronize(s->stream));
        s->d_bin_scale.reset();
        s->bin_steps = false;
        return BB_OK;
    }
    BB_REQUIRE(n_bins == s->L.n_bins, "bb_solver_set_bin_steps: one factor per bin");
    std::vector<double> padded((size_t)s->L.n_pad, 1.0);
    for (int64_t i = 0; i < n_bins; ++i) {
        BB_REQUIRE(std::isfinite(scale[i]) && scale[i] > 0.0,
                   "bb_solver_set_bin_steps: factors must be finite and positive");
        padded[(size_t)i] = scale[i];
    }
    BB_TRY(upload_bin_scale(s, padded.data()));
    s->bin_steps = true;           // (the sweep's reduce and the row-owner kernel both know them)
    return BB_OK;
}

int bb_solver_set_block_steps(bb_solver *s, const double *scale, int64_t n_blocks) {
    BB_REQUIRE(s != nullptr, "bb_solver_set_block_steps: solver is NULL");
    if (scale == nullptr) return bb_solver_set_bin_steps(s, nullptr, 0);
    BB_REQUIRE(n_blocks == s->L.n_blocks, "bb_solver_set_block_steps: one factor per block of the "
                                          "layout (bb_solver_layout: n_blocks)");
    std::vector<double> per_bin((size_t)s->L.n_bins);
    for (int64_t i = 0; i < s->L.n_bins; ++i) per_bin[(size_t)i] = scale[i / s->L.vw];
    return bb_solver_set_bin_steps(s, per_bin.data(), s->L.n_bins);
}

int bb_solver_degrees(bb_solver *s, int64_t *degree, int64_t n_bins) {
    BB_REQUIRE(s != nullptr && degree != nullptr, "bb_solver_degrees: NULL argument");
    BB_REQUIRE(n_bins == s->L.n_bins, "bb_solver_degrees: one count per bin");
    if (!s->have_wish) return bb::fail(BB_ERR_STATE, "bb_solver_degrees: no wish distances set");
    BB_TRY(bb::enter_device(s->device));
    // (the staging buffer of set_coords / get_coords serves: 3 n_pad doubles, nobody else's
    // while this call runs -- every user of it synchronises before it returns)
    int *d_deg = (int *)s->d_f64_tmp;
    BB_HIP_CHECK(hipMemsetAsync(d_deg, 0, (size_t)s->L.n_pad * sizeof(int), s->stream));
    if (s->n_local > 0)
        BB_TRY(by_layout(s, [&](auto lay) -> int {
            using T = typename decltype(lay)::T;
            BB_HIP_CHECK(bb::launch(unit_degrees_kernel<T, decltype(lay)::W>,
                                    dim3((unsigned)((s->n_local + kDegUnits - 1) / kDegUnits)), dim3(256),
                                    0, s->stream, (const T *)s->d_units, s->d_udesc, s->n_local,
                                    s->L.n_bins, d_deg));
            return BB_OK;
        }));
    std::vector<int> host((size_t)n_bins);
    BB_HIP_CHECK(hipStreamSynchronize(s->stream));
    BB_HIP_CHECK(hipMemcpy(host.data(), d_deg, (size_t)n_bins * sizeof(int), hipMemcpyDeviceToHost));
    for (int64_t i = 0; i < n_bins; ++i) degree[i] = host[(size_t)i];
    return BB_OK;
}

int bb_solver_set_weight_power(bb_solver *s, int q) {
    BB_REQUIRE(s != nullptr, "bb_solver_set_weight_power: solver is NULL");
    BB_REQUIRE(q >= 0 && q <= 2, "bb_solver_set_weight_power: q must be 0, 1 or 2");
    if (s->grad_pending)
        return bb::fail(BB_ERR_STATE, "bb_solver_set_weight_power: a bb_solver_grad is pending");
    s->weight_power = q;           // (the stress history is kept: each entry is the S_q of its step)
    return BB_OK;
}

int bb_solver_weight_sums(bb_solver *s, double *sums, int64_t n_bins) {
    BB_REQUIRE(s != nullptr && sums != nullptr, "bb_solver_weight_sums: NULL argument");
    BB_REQUIRE(n_bins == s->L.n_bins, "bb_solver_weight_sums: one sum per bin");
    if (!s->have_wish) return bb::fail(BB_ERR_STATE, "bb_solver_weight_sums: no wish distances set");
    BB_TRY(bb::enter_device(s->device));
    if (s->weight_power == 0 || s->n_local == 0) {      // w = 1: the degrees, as doubles
        std::vector<int64_t> deg((size_t)n_bins, 0);
        if (s->n_local > 0) BB_TRY(bb_solver_degrees(s, deg.data(), n_bins));
        for (int64_t i = 0; i < n_bins; ++i) sums[i] = (double)deg[(size_t)i];
        return BB_OK;
    }
    // (the staging buffer of set_coords / get_coords: 3 n_pad doubles >= n_bins; see degrees)
    double *d_sum = s->d_f64_tmp;
    const dim3 grid((unsigned)((n_bins + 3) / 4));
    BB_TRY(by_layout(s, [&](auto lay) {
        using T = typename decltype(lay)::T;
        return with_int<1, 2>(s->weight_power, [&](auto q) -> int {
            BB_HIP_CHECK(bb::launch(unit_weight_sums_kernel<T, decltype(lay)::W, decltype(q)::value>, grid,
                                    dim3(256), 0, s->stream, (const T *)s->d_units, s->d_udesc, s->n_local,
                                    s->L.n_bins, d_sum));
            return BB_OK;
        });
    }));
    BB_HIP_CHECK(hipStreamSynchronize(s->stream));
    BB_HIP_CHECK(hipMemcpy(sums, d_sum, (size_t)n_bins * sizeof(double), hipMemcpyDeviceToHost));
    return BB_OK;
}

int bb_solver_anchor_sums(bb_solver *s, double *sums, int64_t n_bins) {
    BB_REQUIRE(s != nullptr && sums != nullptr, "bb_solver_anchor_sums: NULL argument");
    BB_REQUIRE(n_bins == s->L.n_bins, "bb_solver_anchor_sums: one sum per bin");
    if (s->anchor_n == 0) {
        std::fill(sums, sums + n_bins, 0.0);
        return BB_OK;
    }
    BB_TRY(bb::enter_device(s->device));
    // (the staging buffer of set_coords / get_coords: 3 n_pad doubles >= n_bins; see degrees)
    double *d_sum = s->d_f64_tmp;
    BB_TRY(by_dtype(s, [&](auto t) {
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
    }));
    BB_HIP_CHECK(hipStreamSynchronize(s->stream));
    BB_HIP_CHECK(hipMemcpy(sums, d_sum, (size_t)n_bins * sizeof(double), hipMemcpyDeviceToHost));
    return BB_OK;
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

int bb_solver_get_score_timing(bb_solver *s, double *profile_ms, double *fold_ms, double *bins_ms) {
    BB_REQUIRE(s != nullptr, "bb_solver_get_score_timing: solver is NULL");
    if (profile_ms) *profile_ms = s->score_ms[0];
    if (fold_ms) *fold_ms = s->score_ms[1];
    if (bins_ms) *bins_ms = s->score_ms[2];
    return BB_OK;
}

int bb_solver_set_wish_from_cm_block(bb_solver *s, const bb_cm *cm, int64_t bin_offset, int kind,
                                     double alpha) {
    BB_REQUIRE(s != nullptr && cm != nullptr, "bb_solver_set_wish_from_cm_block: NULL argument");
    BB_TRY(check_kind_alpha("bb_solver_set_wish_from_cm_block", kind, alpha));
    const double *m = nullptr;
    int64_t d = 0;
    int dev = -1;
    BB_TRY(bb_cm_device_ptr(cm, &m, &d, &dev));
    BB_REQUIRE(d >= 1 && bin_offset >= 0 && bin_offset % s->L.vw == 0 && bin_offset + d <= s->L.n_bins,
               "bb_solver_set_wish_from_cm_block: the map does not fit the solver at that offset");
    BB_REQUIRE(dev == s->device,
               "bb_solver_set_wish_from_cm_block: the map lives on another device than the solver");
    return pack_from_cm(s, m, d, bin_offset, kind, alpha);
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
    BB_TRY(check_kind_alpha("bb_solver_set_wish_from_cm", kind, alpha));
    const double *m = nullptr;
    int64_t d = 0;
    int dev = -1;
    BB_TRY(bb_cm_device_ptr(cm, &m, &d, &dev));
    BB_REQUIRE(d == s->L.n_bins,
               "bb_solver_set_wish_from_cm: the map's edge differs from the solver's n_bins");
    if (dev != s->device) {
        // a map on another GPU: the pack kernel reads it over peer access where the devices
        // allow it (one member of a group per device, each packing its own units from one map)
        int can = 0;
        if (hipDeviceCanAccessPeer(&can, s->device, dev) != hipSuccess) {
            (void)hipGetLastError();
            can = 0;
        }
        BB_REQUIRE(can, "bb_solver_set_wish_from_cm: the map lives on another device than the "
                        "solver, without peer access to it");
        BB_TRY(bb::enter_device(dev));
        BB_HIP_CHECK(hipDeviceSynchronize());          // the map's last operation has landed
        BB_TRY(bb::enter_device(s->device));
        BB_TRY(enable_peer_access("bb_solver_set_wish_from_cm: peer access", dev));
    }
    return pack_from_cm(s, m, d, 0, kind, alpha);
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

int bb_solver_set_coords(bb_solver *s, const double *xyz) {
    BB_REQUIRE(s != nullptr && xyz != nullptr, "bb_solver_set_coords: NULL argument");
    BB_TRY(bb::enter_device(s->device));
    const int64_t n3 = s->L.n_pad * 3;
    BB_HIP_CHECK(upload_padded(s, s->d_f64_tmp, xyz, s->stream));
    BB_HIP_CHECK(narrow(s, s->d_f64_tmp, s->d_X, n3));
    BB_HIP_CHECK(hipMemsetAsync(s->d_V, 0, (size_t)n3 * bb::elem_size(s->dtype), s->stream));
    BB_HIP_CHECK(hipStreamSynchronize(s->stream));
    s->have_coords = true;
    s->hist_n = 0;
    s->grad_pending = false;
    return BB_OK;
}

int bb_solver_get_coords(bb_solver *s, double *xyz) {
    BB_REQUIRE(s != nullptr && xyz != nullptr, "bb_solver_get_coords: NULL argument");
    if (!s->have_coords) return bb::fail(BB_ERR_STATE, "bb_solver_get_coords: no coordinates set");
    BB_TRY(bb::enter_device(s->device));
    const int64_t n3 = s->L.n_pad * 3;
    BB_HIP_CHECK(widen(s, s->d_X, s->d_f64_tmp, n3));
    BB_HIP_CHECK(hipStreamSynchronize(s->stream));
    BB_HIP_CHECK(hipMemcpy(xyz, s->d_f64_tmp, (size_t)s->L.n_bins * 3 * sizeof(double),
                           hipMemcpyDeviceToHost));
    return BB_OK;
}

int bb_solver_set_momentum(bb_solver *s, double mu) {
    BB_REQUIRE(s != nullptr, "bb_solver_set_momentum: solver is NULL");
    BB_REQUIRE(mu >= 0.0 && mu < 1.0, "bb_solver_set_momentum: need 0 <= mu < 1");
    s->momentum = mu;
    return BB_OK;
}

int bb_solver_iterate(bb_solver *s, int64_t iters, double lr) {
    BB_TRY(check_iterate(s, iters, "bb_solver_iterate"));
    if (s->world != 1)
        return bb::fail(BB_ERR_STATE,
                        "bb_solver_iterate: world > 1 needs bb_solver_grad / all-reduce / "
                        "bb_solver_apply");
    BB_TRY(bb::enter_device(s->device));
    if (s->anchor_n > 0) {
        // SPEC 2.5.5: the path bb_solver_grad / bb_solver_apply form, the landmark terms added to
        // the exchange buffer between them (maps of the row-owner path too, while anchors are set)
        for (int64_t k = 0; k < iters; ++k) {
            BB_TRY(timed_step(s, [&] { return launch_grad(s); }, [&] {
                BB_TRY(launch_reduce(s, kReduceExchange, 0.0, nullptr));
                BB_TRY(launch_anchors(s, kAnchorFoldExchange));
                return launch_apply(s, lr, s->d_stress_hist + s->hist_n);
            }));
            s->hist_n++;
        }
        return BB_OK;
    }
    if (s->row_owner) {
        // one launch per iteration; launch k also folds the stress of launch k-1
        for (int64_t k = 0; k < iters; ++k) {
            BB_TRY(timed_step(s, [&] { return launch_row_owner(s, lr, k > 0, true); },
                              [] { return (int)BB_OK; }));
            s->hist_n++;
        }
        if (iters > 0) BB_TRY(launch_row_owner(s, lr, true, false));
        return BB_OK;
    }
    for (int64_t k = 0; k < iters; ++k) {
        BB_TRY(timed_step(s, [&] { return launch_grad(s); }, [&] {
            return launch_reduce(s, kReduceApply, lr, s->d_stress_hist + s->hist_n * s->n_maps);
        }));
        s->hist_n++;
    }
    return BB_OK;
}

int bb_solver_grad(bb_solver *s) {
    BB_TRY(check_ready(s, "bb_solver_grad"));
    if (s->n_maps > 1)
        return bb::fail(BB_ERR_STATE, "bb_solver_grad: a solver of several maps (bb_solver_set_maps) "
                                      "iterates with bb_solver_iterate only");
    BB_TRY(bb::enter_device(s->device));
    BB_TRY(timed_step(s, [&] { return launch_grad(s); },
                      [&] { return launch_reduce(s, kReduceExchange, 0.0, nullptr); }));
    if (s->anchor_n > 0) BB_TRY(launch_anchors(s, kAnchorFoldExchange));
    s->grad_pending = true;
    return BB_OK;
}

int bb_solver_apply(bb_solver *s, double lr) {
    BB_TRY(check_ready(s, "bb_solver_apply"));
    if (!s->grad_pending)
        return bb::fail(BB_ERR_STATE, "bb_solver_apply: no bb_solver_grad pending");
    if (s->hist_n + 1 > s->hist_cap)
        return bb::fail(BB_ERR_STATE, "bb_solver_apply: stress history full");
    BB_TRY(bb::enter_device(s->device));
    BB_TRY(launch_apply(s, lr, s->d_stress_hist + s->hist_n));
    s->hist_n++;
    s->grad_pending = false;
    return BB_OK;
}

int bb_comm_unique_id(void *id_out) {
    BB_REQUIRE(id_out != nullptr, "bb_comm_unique_id: id_out is NULL");
    const bb::Rccl &R = bb::rccl();
    if (!R.ok) return bb::fail(BB_ERR_HIP, "bb_comm_unique_id: librccl is not loadable");
    bb::Rccl::UniqueId id;
    const int rc = R.GetUniqueId(&id);
    if (rc != bb::Rccl::kSuccess)
        return bb::fail(BB_ERR_HIP, std::string("ncclGetUniqueId: ") + R.GetErrorString(rc));
    memcpy(id_out, id.internal, bb::kUniqueIdBytes);
    return BB_OK;
}

// The library's communicators outlive the solvers that use them: ncclCommInitRank costs
// 0.1-1 s and every multi-rank fit() used to pay it (round 2 made a fresh communicator per
// fit and destroyed it with the solver).  One communicator per (device, rank, world) is
// kept for the life of the process; a solver borrows it (bb_solver_comm_attach) and gives
// it back when it is destroyed.  While one solver holds it, another one gets a
// communicator of its own (a communicator must not serve two streams at once).
namespace {
struct CachedComm {
    bb::Rccl::Comm comm = nullptr;
    bool in_use = false;
    // Which ncclCommInitRank made it: a hash of the 128-byte unique id, the same on every rank
    // of that call and on no other.  The key (device, rank, world) alone cannot tell two
    // communicators of different jobs -- or of different generations of one job -- apart; the
    // ranks compare this before anybody attaches (bb_comm_cached_generation, solver.comm_reuse).
    uint64_t generation = 0;
};
uint64_t comm_generation_of(const void *unique_id) {
    uint64_t h = 1469598103934665603ull;             // FNV-1a over the id
    const unsigned char *b = (const unsigned char *)unique_id;
    for (size_t i = 0; i < bb::kUniqueIdBytes; ++i) h = (h ^ b[i]) * 1099511628211ull;
    return h ? h : 1;                                // 0 = "none"
}
std::mutex g_comm_mu;
std::map<std::tuple<int, int, int>, CachedComm> g_comm_cache;

// The cache's entry of (device, rank, world) if it is there, holds a communicator and is
// free, else NULL.  The caller holds g_comm_mu.
CachedComm *cached_comm(int device, int rank, int world) {
    auto it = g_comm_cache.find(std::make_tuple(device, rank, world));
    return it != g_comm_cache.end() && it->second.comm && !it->second.in_use ? &it->second : nullptr;
}

void comm_release(bb_solver *s, bool destroy) {
    if (!s->comm) return;
    std::lock_guard<std::mutex> lock(g_comm_mu);
    if (s->comm_cached) {
        auto it = g_comm_cache.find(std::make_tuple(s->device, s->rank, s->world));
        if (it != g_comm_cache.end() && it->second.comm == s->comm) {
            if (destroy || s->comm_suspect)
                g_comm_cache.erase(it);       // a suspect communicator is not handed out again
            else
                it->second.in_use = false;
        }
    }
    s->comm = nullptr;
    s->comm_cached = false;
    s->comm_suspect = false;
}
}  // namespace

int bb_comm_cached_generation(int device, int rank, int world, int *available,
                              uint64_t *generation) {
    BB_REQUIRE(available != nullptr && generation != nullptr,
               "bb_comm_cached_generation: NULL argument");
    std::lock_guard<std::mutex> lock(g_comm_mu);
    const CachedComm *c = cached_comm(device, rank, world);
    *available = c ? 1 : 0;
    *generation = c ? c->generation : 0;
    return BB_OK;
}

int bb_comm_cached(int device, int rank, int world, int *available) {
    BB_REQUIRE(available != nullptr, "bb_comm_cached: available is NULL");
    uint64_t generation = 0;
    return bb_comm_cached_generation(device, rank, world, available, &generation);
}

int bb_solver_comm_attach(bb_solver *s) {
    BB_REQUIRE(s != nullptr, "bb_solver_comm_attach: solver is NULL");
    if (s->comm) return bb::fail(BB_ERR_STATE, "bb_solver_comm_attach: communicator already made");
    std::lock_guard<std::mutex> lock(g_comm_mu);
    CachedComm *c = cached_comm(s->device, s->rank, s->world);
    if (!c) return bb::fail(BB_ERR_STATE, "bb_solver_comm_attach: no free cached communicator");
    c->in_use = true;
    s->comm = c->comm;
    s->comm_cached = true;
    return BB_OK;
}

int bb_solver_comm_detach(bb_solver *s) {
    BB_REQUIRE(s != nullptr, "bb_solver_comm_detach: solver is NULL");
    if (s->comm && !s->comm_cached)
        return bb::fail(BB_ERR_STATE, "bb_solver_comm_detach: the communicator is the solver's own");
    comm_release(s, /*destroy=*/false);
    return BB_OK;
}

int bb_comm_cache_clear(void) {
    const bb::Rccl &R = bb::rccl();
    std::lock_guard<std::mutex> lock(g_comm_mu);
    for (auto it = g_comm_cache.begin(); it != g_comm_cache.end();) {
        if (it->second.in_use) { ++it; continue; }
        if (it->second.comm && R.ok) R.CommDestroy(it->second.comm);
        it = g_comm_cache.erase(it);
    }
    return BB_OK;
}

int bb_solver_comm_init(bb_solver *s, const void *unique_id) {
    BB_REQUIRE(s != nullptr && unique_id != nullptr, "bb_solver_comm_init: NULL argument");
    if (s->comm) return bb::fail(BB_ERR_STATE, "bb_solver_comm_init: communicator already made");
    const bb::Rccl &R = bb::rccl();
    if (!R.ok) return bb::fail(BB_ERR_HIP, "bb_solver_comm_init: librccl is not loadable");
    BB_TRY(bb::enter_device(s->device));
    bb::Rccl::UniqueId id;
    memcpy(id.internal, unique_id, bb::kUniqueIdBytes);
    const int rc = R.CommInitRank(&s->comm, s->world, id, s->rank);
    if (rc != bb::Rccl::kSuccess) {
        s->comm = nullptr;
        return bb::fail(BB_ERR_HIP, std::string("ncclCommInitRank: ") + R.GetErrorString(rc));
    }
    {
        // into the cache, unless another solver holds this key's entry right now
        std::lock_guard<std::mutex> lock(g_comm_mu);
        CachedComm &c = g_comm_cache[std::make_tuple(s->device, s->rank, s->world)];
        if (!c.in_use) {
            if (c.comm && c.comm != s->comm) R.CommDestroy(c.comm);   // a stale one: replaced
            c.comm = s->comm;
            c.in_use = true;
            c.generation = comm_generation_of(unique_id);
            s->comm_cached = true;
        }
    }
    return BB_OK;
}

int bb_solver_comm_abort(bb_solver *s) {
    BB_REQUIRE(s != nullptr, "bb_solver_comm_abort: solver is NULL");
    if (!s->comm) return BB_OK;
    const bb::Rccl &R = bb::rccl();
    bb::Rccl::Comm c = s->comm;
    comm_release(s, /*destroy=*/true);       // out of the cache: it is not handed out again
    s->grad_pending = false;
    if (!R.CommAbort) {
        // No ncclCommAbort in this librccl.  ncclCommDestroy waits for the communicator's
        // outstanding work -- on a communicator that may sit in a collective a peer never
        // joined that is for ever, which is exactly what this call exists to end.  The
        // communicator is leaked instead and the solver's stream is marked stuck: nothing
        // synchronises on it any more (bb_solver_destroy, the stream pool).
        s->stream_stuck = true;
        return bb::fail(BB_ERR_STATE,
                        "bb_solver_comm_abort: this librccl has no ncclCommAbort; the "
                        "communicator was leaked and the solver's stream abandoned");
    }
    // ncclCommAbort ends the communicator's in-flight kernels, so a stream that is
    // stuck behind a collective a peer never joined drains again
    const int rc = R.CommAbort(c);
    if (rc != bb::Rccl::kSuccess)
        return bb::fail(BB_ERR_HIP, std::string("ncclCommAbort: ") + R.GetErrorString(rc));
    return BB_OK;
}

int bb_solver_comm_world(const bb_solver *s, int *world) {
    BB_REQUIRE(s != nullptr && world != nullptr, "bb_solver_comm_world: NULL argument");
    *world = 0;
    if (!s->comm) return bb::fail(BB_ERR_STATE, "bb_solver_comm_world: no communicator");
    const bb::Rccl &R = bb::rccl();
    if (!R.CommCount) return bb::fail(BB_ERR_HIP, "bb_solver_comm_world: ncclCommCount missing");
    const int rc = R.CommCount(s->comm, world);
    if (rc != bb::Rccl::kSuccess)
        return bb::fail(BB_ERR_HIP, std::string("ncclCommCount: ") + R.GetErrorString(rc));
    return BB_OK;
}

namespace {
int enqueue_allreduce(bb_solver *s) {
    const bb::Rccl &R = bb::rccl();
    const int rc = R.AllReduce(s->d_exch, s->d_exch, (size_t)(3 * s->L.n_pad + 2),
                               s->dtype == BB_F32 ? bb::Rccl::kFloat32 : bb::Rccl::kFloat64,
                               bb::Rccl::kSum, s->comm, s->stream);
    if (rc != bb::Rccl::kSuccess) {
        s->comm_suspect = true;      // its peers may now sit in a collective this rank left
        return bb::fail(BB_ERR_HIP, std::string("ncclAllReduce: ") + R.GetErrorString(rc));
    }
    return BB_OK;
}
}  // namespace

int bb_solver_allreduce(bb_solver *s) {
    BB_REQUIRE(s != nullptr, "bb_solver_allreduce: solver is NULL");
    if (!s->comm) return bb::fail(BB_ERR_STATE, "bb_solver_allreduce: no communicator");
    if (!s->grad_pending) return bb::fail(BB_ERR_STATE, "bb_solver_allreduce: no bb_solver_grad pending");
    BB_TRY(bb::enter_device(s->device));
    return enqueue_allreduce(s);
}

int bb_solver_iterate_dist(bb_solver *s, int64_t iters, double lr) {
    BB_TRY(check_iterate(s, iters, "bb_solver_iterate_dist"));
    for (int64_t k = 0; k < iters; ++k) {
        BB_TRY(bb_solver_grad(s));
        BB_TRY(bb_solver_allreduce(s));
        BB_TRY(bb_solver_apply(s, lr));
    }
    return BB_OK;
}

}  // extern "C"

namespace bb {
namespace solver {
// The receiving half of the two-launch peer exchange (peer_receive_kernel): wait for every
// rank's flag of exchange `peer_seq`, X <- X + (mu V - lr * sum over the ranks in rank order).
int launch_peer_receive(bb_solver *s, void *X, double lr, double mu, double *stress_out) {
    const int64_t n3 = s->L.n_pad * 3, es = bb::elem_size(s->dtype);
    // Ranks that share a GPU (a rehearsal) share its wave slots too: the receive kernels of ALL
    // of them wait at once, and eight times 256 workgroups of 4 waves are every slot the chip
    // has -- nobody's sweep could start (found by tools/world8_rehearsal.py).  The cap is
    // divided among them; a thread then takes more elements.
    const int64_t cap = std::max<int64_t>(8, (int64_t)kPeerReceiveWGs / (s->peer_ranks_on_gpu > 2 ? s->peer_ranks_on_gpu / 2 : 1));
    const unsigned grid = (unsigned)std::min<int64_t>((n3 + 255) / 256, cap);
    const char *arena = s->peer_arena.as<const char>() +
                        (int64_t)(s->peer_seq & 1) * s->world * s->peer_slot_elems * es;
    const unsigned long long *flags =
        (const unsigned long long *)(s->peer_arena.as<const char>() + peer_flags_offset(s));
    // the flag pointers are the second half of a PeerTable (same for both parities)
    unsigned long long *const *poison =
        (unsigned long long *const *)(s->d_peer_table.as<const char>() + kMaxPeers * sizeof(void *));
    return by_dtype(s, [&](auto t) -> int {
        using T = typename decltype(t)::T;
        BB_HIP_CHECK(bb::launch(peer_receive_kernel<T>, dim3(grid), dim3(256), 0, s->stream, (T *)X,
                                (T *)s->d_V, (const T *)arena, flags, poison, s->world, s->peer_slot_elems,
                                n3, (T)lr, (T)mu, stress_out, s->peer_seq, s->d_peer_state.as<PeerState>(),
                                s->peer_limit_ticks, s->d_peer_mask.as<const unsigned>(), (int)(3 * s->L.vw)));
        return BB_OK;
    });
}

// The plain SUM over the ranks of what the last sweep left in the partials (scale 1: a
// matvec, not a gradient), into the exchange buffer [0, 3 n_pad) of every rank, enqueued on
// the solver's stream: the reduce alone on one rank; the peer exchange (either form; the
// ranks' partials are added in rank order, so every rank holds the same bits) when the
// arenas are connected; else the library's RCCL communicator.  The step-taking kernels are
// used as they are -- see bb_solver::sum_target.  d_V is left holding the sum as well.
int exchange_sum(bb_solver *s) {
    const int64_t n3 = s->L.n_pad * 3, es = bb::elem_size(s->dtype);
    if (s->peer_connected) {        // (also a one-rank solver that pushes to itself: a rehearsal)
        BB_HIP_CHECK(hipMemsetAsync(s->d_exch, 0, (size_t)(n3 * es), s->stream));
        s->peer_seq++;
        s->sum_target = s->d_exch;
        int rc;
        if (s->peer_fused) {
            rc = launch_exchange(s, -1.0, s->d_stress_scalar, kScalePlainSum);
        } else {
            rc = launch_reduce(s, kReducePeer, 0.0, nullptr, kScalePlainSum);
            if (rc == BB_OK) rc = launch_peer_receive(s, s->d_exch, -1.0, 0.0, s->d_stress_scalar);
        }
        s->sum_target = nullptr;
        return rc;
    }
    if (s->comm) {
        BB_TRY(launch_reduce(s, kReduceExchange, 0.0, nullptr, kScalePlainSum));
        return enqueue_allreduce(s);
    }
    if (s->world == 1) return launch_reduce(s, kReduceExchange, 0.0, nullptr, kScalePlainSum);
    return bb::fail(BB_ERR_STATE, "no exchange between the ranks is set up (bb_solver_peer_connect "
                                  "or bb_solver_comm_init / _attach first)");
}
}  // namespace solver
}  // namespace bb

extern "C" {

int bb_solver_peer_export(bb_solver *s, void *handle_out) {
    BB_REQUIRE(s != nullptr && handle_out != nullptr, "bb_solver_peer_export: NULL argument");
    BB_REQUIRE(s->world <= kMaxPeers, "bb_solver_peer_export: world > 16");
    if (s->peer_arena) return bb::fail(BB_ERR_STATE, "bb_solver_peer_export: already exported");
    BB_TRY(bb::enter_device(s->device));
    const int64_t es = bb::elem_size(s->dtype);
    s->peer_slot_elems = bb::round_up(3 * s->L.n_pad + 2, 256 / es);
    s->peer_arena_bytes = peer_arena_size(s);
    // Uncached: written by the peers' kernels while ours is running, so nothing of
    // it may live in this GPU's L2.  (RCCL allocates its own buffers the same way.)
    void *arena = nullptr;
    hipError_t e = hipExtMallocWithFlags(&arena, (size_t)s->peer_arena_bytes, hipDeviceMallocUncached);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        e = hipExtMallocWithFlags(&arena, (size_t)s->peer_arena_bytes, hipDeviceMallocFinegrained);
    }
    if (e != hipSuccess) {
        return bb::fail(BB_ERR_NOMEM, std::string("bb_solver_peer_export: arena: ") +
                                          hipGetErrorString(e));
    }
    // every data word starts out EMPTY (all bits set: reduce_exchange_kernel), flags and poison
    // words at 0
    s->peer_arena.adopt(arena, (size_t)s->peer_arena_bytes);
    BB_HIP_CHECK(hipMemset(s->peer_arena.p, 0xff, (size_t)peer_flags_offset(s)));
    BB_HIP_CHECK(hipMemset(s->peer_arena.as<char>() + peer_flags_offset(s), 0,
                           (size_t)(s->peer_arena_bytes - peer_flags_offset(s))));
    BB_HIP_CHECK(hipDeviceSynchronize());
    PeerHandle h;
    memset(&h, 0, sizeof(h));
    e = hipIpcGetMemHandle(&h.ipc, s->peer_arena.p);
    if (e != hipSuccess) {
        s->peer_arena.reset();
        return bb::fail(BB_ERR_HIP, std::string("bb_solver_peer_export: hipIpcGetMemHandle: ") +
                                        hipGetErrorString(e));
    }
    h.magic = kPeerMagic;
    h.arena_bytes = s->peer_arena_bytes;
    h.slot_elems = s->peer_slot_elems;
    h.pid = (int64_t)getpid();
    h.raw = (uint64_t)(uintptr_t)s->peer_arena.p;
    h.rank = s->rank;
    h.world = s->world;
    h.dtype = s->dtype;
    h.device = s->device;
    {
        int dom = 0, bus = 0, dev = 0;
        if (hipDeviceGetAttribute(&dom, hipDeviceAttributePciDomainID, s->device) != hipSuccess ||
            hipDeviceGetAttribute(&bus, hipDeviceAttributePciBusId, s->device) != hipSuccess ||
            hipDeviceGetAttribute(&dev, hipDeviceAttributePciDeviceId, s->device) != hipSuccess) {
            (void)hipGetLastError();
            dom = bus = dev = 0;       // unknown: ranks then count as sharing one GPU (the safe side)
        }
        h.pci = ((uint64_t)(uint32_t)dom << 32) | ((uint64_t)(bus & 0xffff) << 16) | (uint64_t)(dev & 0xffff);
    }
    memset(handle_out, 0, BB_PEER_HANDLE_BYTES);
    memcpy(handle_out, &h, sizeof(h));
    return BB_OK;
}

int bb_solver_peer_connect(bb_solver *s, const void *handles) {
    BB_REQUIRE(s != nullptr && handles != nullptr, "bb_solver_peer_connect: NULL argument");
    if (!s->peer_arena) return bb::fail(BB_ERR_STATE, "bb_solver_peer_connect: export first");
    if (s->peer_connected) return bb::fail(BB_ERR_STATE, "bb_solver_peer_connect: already connected");
    BB_TRY(bb::enter_device(s->device));
    const SolverEnv env = solver_env();
    s->peer_mapped.assign((size_t)s->world, nullptr);
    std::map<uint64_t, int> ranks_on_gpu;      // how many ranks sit on each GPU of the node
    int most_on_one_gpu = 1;
    for (int r = 0; r < s->world; ++r) {
        PeerHandle h;
        memcpy(&h, (const char *)handles + (size_t)r * BB_PEER_HANDLE_BYTES, sizeof(h));
        most_on_one_gpu = std::max(most_on_one_gpu, ++ranks_on_gpu[h.pci]);
        if (h.magic != kPeerMagic || h.rank != r || h.world != s->world || h.dtype != s->dtype ||
            h.arena_bytes != s->peer_arena_bytes || h.slot_elems != s->peer_slot_elems)
            return bb::fail(BB_ERR_INVALID, "bb_solver_peer_connect: handle " + std::to_string(r) +
                                                " does not match this solver (rank order, world, "
                                                "dtype and n_bins must agree)");
        if (r == s->rank) {
            s->peer_mapped[r] = s->peer_arena.p;
        } else if (h.pid == (int64_t)getpid()) {
            // same process: the exporter's pointer is valid here, but only from the
            // same device or with peer access
            if (h.device != s->device)
                BB_TRY(enable_peer_access("bb_solver_peer_connect: peer access", h.device));
            s->peer_mapped[r] = (void *)(uintptr_t)h.raw;
        } else {
            void *ptr = nullptr;
            hipError_t e = hipIpcOpenMemHandle(&ptr, h.ipc, hipIpcMemLazyEnablePeerAccess);
            if (e != hipSuccess)
                return bb::fail(BB_ERR_HIP, "bb_solver_peer_connect: hipIpcOpenMemHandle(rank " +
                                                std::to_string(r) + "): " + hipGetErrorString(e));
            s->peer_mapped[r] = ptr;
            s->peer_opened.push_back(ptr);
        }
    }
    BB_TRY(by_dtype(s, [&](auto t) { return build_peer_tables(t, s); }));
    {
        // Who sends what: rank q's units lie in tiles (I, J) and carry gradient for the bins of
        // blocks I and J only; for every other block its partial is zero by construction.  Every
        // rank computes the same table from the tile list and the partition, so senders and
        // receivers agree without a word exchanged.  Dense N=50,000 on 8 ranks: rank 0 touches
        // a third of the blocks (28 % fewer bytes on the links over all ranks); the whole genome
        // as blocks: a rank touches the blocks of a few chromosomes (BB_PEER_MASK=0: all send all).
        s->d_peer_mask.reset();
        if (env.peer_mask && s->world <= 32) {
            std::vector<unsigned> mask;
            BB_TRY(contributor_mask(s, &mask));
            BB_TRY(bb::alloc_status(s->d_peer_mask, mask.size() * sizeof(unsigned)));
            BB_HIP_CHECK(hipMemcpy(s->d_peer_mask.p, mask.data(), mask.size() * sizeof(unsigned),
                                   hipMemcpyHostToDevice));
        }
    }
    BB_TRY(bb::alloc_status(s->d_peer_state, sizeof(PeerState)));
    // the top counter + one per block on a line of its own (reduce_sliced_kernel's two-level
    // check-in)
    const int64_t n_counters = 32 * (s->L.n_blocks + 1);
    BB_TRY(bb::alloc_status(s->d_peer_counter, (size_t)n_counters * sizeof(unsigned)));
    BB_HIP_CHECK(hipMemset(s->d_peer_state.p, 0, sizeof(PeerState)));
    BB_HIP_CHECK(hipMemset(s->d_peer_counter.p, 0, (size_t)n_counters * sizeof(unsigned)));
    // ticks of wall_clock64(): ask the runtime, fall back to gfx9's 100 MHz.  The query
    // is allowed to fail (older runtimes); its error is consumed here, on the spot.
    int khz = 0;
    if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, s->device) != hipSuccess) {
        (void)hipGetLastError();
        khz = 0;
    }
    s->peer_clock_khz = khz > 0 ? khz : 100000;
    s->peer_limit_ticks = env.peer_timeout_ms * s->peer_clock_khz;
    s->peer_seq = 0;
    {
        // The one-launch exchange (reduce_exchange_kernel) has every workgroup wait for its
        // peers' copies of itself: fine with one rank per GPU (workgroups are dispatched in
        // order and push before they wait), not when ranks SHARE a GPU and the waiting
        // workgroups of some can keep the sweep of another off the device (three ranks at
        // N=7,000 fp64 on one GPU: every CU held a waiting workgroup and 16 KB of its LDS, the
        // third rank's sweep wants 150 KB per workgroup, time-out).  Every rank sees every
        // handle (PCI ids), so all of them decide alike: any GPU with two ranks on it -- a
        // rehearsal -- and it is the two-launch form.  BB_PEER_FUSED=0|1 overrides (the same
        // on every rank; small problems on a shared GPU do run in one launch).
        s->peer_fused = env.peer_fused >= 0 ? env.peer_fused != 0 : most_on_one_gpu == 1;
        s->peer_ranks_on_gpu = most_on_one_gpu;
        if (most_on_one_gpu > 1) s->pk_stale = true;   // a stream built before this goes (ensure_pk24)
    }
    s->peer_connected = true;
    BB_HIP_CHECK(hipDeviceSynchronize());
    return BB_OK;
}

int bb_solver_peer_set_timeout(bb_solver *s, int64_t milliseconds) {
    BB_REQUIRE(s != nullptr, "bb_solver_peer_set_timeout: solver is NULL");
    BB_REQUIRE(milliseconds > 0 && milliseconds <= 3600000,
               "bb_solver_peer_set_timeout: need 0 < ms <= 3600000");
    if (!s->peer_connected)
        return bb::fail(BB_ERR_STATE, "bb_solver_peer_set_timeout: not connected");
    s->peer_limit_ticks = (long long)milliseconds * s->peer_clock_khz;
    return BB_OK;
}

int bb_solver_peer_set_form(bb_solver *s, int one_launch) {
    BB_REQUIRE(s != nullptr, "bb_solver_peer_set_form: solver is NULL");
    if (!s->peer_connected)
        return bb::fail(BB_ERR_STATE, "bb_solver_peer_set_form: not connected");
    // the one-launch form reads "empty" in every slot word it has not been sent: it can only
    // be chosen while no exchange has run (the two-launch form leaves its partials in the slots)
    if (s->peer_seq != 0)
        return bb::fail(BB_ERR_STATE, "bb_solver_peer_set_form: exchanges have already run");
    s->peer_fused = one_launch != 0;
    return BB_OK;
}

int bb_solver_peer_form(bb_solver *s, int *one_launch) {
    BB_REQUIRE(s != nullptr && one_launch != nullptr, "bb_solver_peer_form: NULL argument");
    if (!s->peer_connected) return bb::fail(BB_ERR_STATE, "bb_solver_peer_form: not connected");
    *one_launch = s->peer_fused ? 1 : 0;
    return BB_OK;
}

int bb_solver_peer_status(bb_solver *s, int *status) {
    BB_REQUIRE(s != nullptr, "bb_solver_peer_status: solver is NULL");
    if (!s->peer_connected) return bb::fail(BB_ERR_STATE, "bb_solver_peer_status: not connected");
    BB_TRY(bb::enter_device(s->device));
    PeerState st;
    memset(&st, 0, sizeof(st));
    BB_HIP_CHECK(hipStreamSynchronize(s->stream));
    BB_HIP_CHECK(hipMemcpy(&st, s->d_peer_state.p, sizeof(st), hipMemcpyDeviceToHost));
    if (status) *status = st.status;
    if (st.status != 0) {
        const bool one = s->peer_fused;
        return bb::fail(BB_ERR_STATE,
                        std::string("peer exchange: a rank did not deliver its partial within the "
                                    "time limit (BB_PEER_TIMEOUT_MS), or reported its own failure; ") +
                            (one ? "the last exchange this rank completed whole was "
                                 : "this rank's coordinates were left at its last completed step (") +
                            std::to_string(st.verdict) + " of " + std::to_string(s->peer_seq) +
                            (one ? " (the one after it may be applied in part: the coordinates of "
                                   "this solver are not a result)"
                                 : " exchanges)") +
                            " and every peer has been told to stop");
    }
    return BB_OK;
}

int bb_solver_iterate_peer(bb_solver *s, int64_t iters, double lr) {
    BB_TRY(check_iterate(s, iters, "bb_solver_iterate_peer"));
    // (its kernels step from the reduce itself: nothing could add the landmark terms in between)
    if (s->anchor_n > 0)
        return bb::fail(BB_ERR_STATE, "bb_solver_iterate_peer: a solver with landmark anchors iterates "
                                      "with bb_solver_iterate");
    if (!s->peer_connected)
        return bb::fail(BB_ERR_STATE, "bb_solver_iterate_peer: bb_solver_peer_connect first");
    if (s->grad_pending)
        return bb::fail(BB_ERR_STATE, "bb_solver_iterate_peer: a bb_solver_grad is pending");
    // (the exchange kernels fold one stress per iteration into the history)
    if (s->n_maps > 1)
        return bb::fail(BB_ERR_STATE, "bb_solver_iterate_peer: a solver of several maps "
                                      "(bb_solver_set_maps) iterates with bb_solver_iterate only");
    BB_TRY(bb::enter_device(s->device));
    for (int64_t k = 0; k < iters; ++k) {
        double *hist = s->d_stress_hist + s->hist_n;
        // one launch: reduce, push, wait, sum, update (reduce_exchange_kernel); else the reduce
        // pushes and peer_receive_kernel waits, sums and updates
        BB_TRY(timed_step(s, [&] { return launch_grad(s); }, [&] {
            s->peer_seq++;
            return s->peer_fused ? launch_exchange(s, lr, hist) : launch_reduce(s, kReducePeer, 0.0, nullptr);
        }));
        if (!s->peer_fused) BB_TRY(launch_peer_receive(s, s->d_X, lr, s->momentum, hist));
        s->hist_n++;
    }
    return BB_OK;
}

int bb_solver_exchange_size(const bb_solver *s, int64_t *n_elems) {
    BB_REQUIRE(s != nullptr && n_elems != nullptr, "bb_solver_exchange_size: NULL argument");
    *n_elems = 3 * s->L.n_pad + 2;
    return BB_OK;
}

int bb_solver_get_exchange_buffer(bb_solver *s, void **dev_ptr) {
    BB_REQUIRE(s != nullptr && dev_ptr != nullptr, "bb_solver_get_exchange_buffer: NULL argument");
    *dev_ptr = s->d_exch;
    return BB_OK;
}

int bb_solver_set_exchange_buffer(bb_solver *s, void *dev_ptr) {
    BB_REQUIRE(s != nullptr && dev_ptr != nullptr, "bb_solver_set_exchange_buffer: NULL argument");
    BB_TRY(bb::enter_device(s->device));
    BB_HIP_CHECK(hipStreamSynchronize(s->stream));
    s->own_exch.reset();
    s->d_exch = dev_ptr;
    return BB_OK;
}

int bb_solver_read_exchange(bb_solver *s, double *host, int64_t n) {
    BB_REQUIRE(s != nullptr && host != nullptr, "bb_solver_read_exchange: NULL argument");
    BB_REQUIRE(n == 3 * s->L.n_pad + 2, "bb_solver_read_exchange: n != exchange size");
    BB_TRY(bb::enter_device(s->device));
    bb::DevBuf buf;
    BB_TRY(bb::alloc_status(buf, (size_t)n * sizeof(double)));
    double *tmp = buf.as<double>();
    hipError_t e = widen(s, s->d_exch, tmp, n);
    if (e == hipSuccess)
        e = hipMemcpyAsync(host, tmp, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, s->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
    return bb::hip_status("bb_solver_read_exchange", e);
}

int bb_solver_write_exchange(bb_solver *s, const double *host, int64_t n) {
    BB_REQUIRE(s != nullptr && host != nullptr, "bb_solver_write_exchange: NULL argument");
    BB_REQUIRE(n == 3 * s->L.n_pad + 2, "bb_solver_write_exchange: n != exchange size");
    BB_TRY(bb::enter_device(s->device));
    bb::DevBuf buf;
    BB_TRY(bb::alloc_status(buf, (size_t)n * sizeof(double)));
    double *tmp = buf.as<double>();
    hipError_t e = hipMemcpyAsync(tmp, host, (size_t)n * sizeof(double), hipMemcpyHostToDevice,
                                  s->stream);
    if (e == hipSuccess) e = narrow(s, tmp, s->d_exch, n);
    if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
    return bb::hip_status("bb_solver_write_exchange", e);
}

int bb_solver_matvec_sq(bb_solver *s, const double *x, double *y) {
    BB_REQUIRE(s != nullptr && x != nullptr && y != nullptr, "bb_solver_matvec_sq: NULL argument");
    if (!s->have_wish) return bb::fail(BB_ERR_STATE, "bb_solver_matvec_sq: no wish distances set");
    if (s->n_maps > 1)
        return bb::fail(BB_ERR_STATE, "bb_solver_matvec_sq: not for a solver of several maps");
    if (s->grad_pending)
        return bb::fail(BB_ERR_STATE, "bb_solver_matvec_sq: a bb_solver_grad is pending");
    BB_TRY(bb::enter_device(s->device));
    const int64_t n3 = s->L.n_pad * 3, es = bb::elem_size(s->dtype);
    // (a spectral start calls this ~40 times: the buffer is allocated once and kept)
    if (!s->d_mv_in) BB_TRY(bb::alloc_status(s->d_mv_in, (size_t)(n3 * es)));
    void *d_in = s->d_mv_in.p;
    hipError_t e = upload_padded(s, s->d_f64_tmp, x, s->stream);
    if (e == hipSuccess) e = narrow(s, s->d_f64_tmp, d_in, n3);
    int rc = BB_OK;
    if (e != hipSuccess) rc = bb::hip_status("bb_solver_matvec_sq", e);
    if (rc == BB_OK) rc = launch_grad(s, kOpMatvec2, d_in);
    if (rc == BB_OK) rc = launch_reduce(s, kReduceExchange, 0.0, nullptr, kScalePlainSum);
    if (rc == BB_OK) {
        e = widen(s, s->d_exch, s->d_f64_tmp, n3);
        if (e == hipSuccess)
            e = hipMemcpyAsync(y, s->d_f64_tmp, (size_t)s->L.n_bins * 24, hipMemcpyDeviceToHost,
                               s->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
        if (e != hipSuccess)
            rc = bb::hip_status("bb_solver_matvec_sq", e);
    }
    if (hipStreamSynchronize(s->stream) != hipSuccess && rc == BB_OK)
        rc = bb::fail(BB_ERR_HIP, "bb_solver_matvec_sq: the stream did not drain");
    return rc;
}

int bb_solver_stress(bb_solver *s, double *stress) {
    BB_TRY(check_ready(s, "bb_solver_stress"));
    BB_REQUIRE(stress != nullptr, "bb_solver_stress: stress is NULL");
    // the sum over the maps, in index order (one map: its value as it is)
    std::vector<double> per((size_t)s->n_maps);
    BB_TRY(bb_solver_stress_maps(s, per.data(), s->n_maps));
    *stress = per[0];
    for (size_t m = 1; m < per.size(); ++m) *stress += per[m];
    return BB_OK;
}

int bb_solver_stress_maps(bb_solver *s, double *stress, int n_maps) {
    BB_TRY(check_ready(s, "bb_solver_stress_maps"));
    BB_REQUIRE(stress != nullptr && n_maps == s->n_maps, "bb_solver_stress_maps: bad argument");
    BB_TRY(bb::enter_device(s->device));
    BB_TRY(launch_grad(s));
    double *out = s->n_maps > 1 ? s->d_map_scalar.as<double>() : s->d_stress_scalar;
    BB_TRY(launch_reduce(s, kReduceStressOnly, 0.0, out));
    if (s->anchor_n > 0) BB_TRY(launch_anchors(s, kAnchorFoldStress, out));   // (one map: SPEC 2.5.5's total)
    BB_HIP_CHECK(hipStreamSynchronize(s->stream));
    BB_HIP_CHECK(hipMemcpy(stress, out, (size_t)s->n_maps * sizeof(double), hipMemcpyDeviceToHost));
    return BB_OK;
}

int bb_solver_get_stress_history(bb_solver *s, double *out, int64_t cap, int64_t *n) {
    BB_REQUIRE(s != nullptr && n != nullptr, "bb_solver_get_stress_history: NULL argument");
    BB_TRY(bb::enter_device(s->device));
    BB_HIP_CHECK(hipStreamSynchronize(s->stream));
    // (several maps: iteration-major, n_maps values per iteration)
    *n = s->hist_n * s->n_maps;
    const int64_t m = std::min(cap, s->hist_n * s->n_maps);
    if (out && m > 0)
        BB_HIP_CHECK(hipMemcpy(out, s->d_stress_hist, (size_t)m * sizeof(double),
                               hipMemcpyDeviceToHost));
    return BB_OK;
}

int bb_solver_sync(bb_solver *s) {
    BB_REQUIRE(s != nullptr, "bb_solver_sync: solver is NULL");
    BB_TRY(bb::enter_device(s->device));
    BB_HIP_CHECK(hipStreamSynchronize(s->stream));
    return BB_OK;
}

int bb_solver_sync_timeout(bb_solver *s, int64_t milliseconds) {
    BB_REQUIRE(s != nullptr, "bb_solver_sync_timeout: solver is NULL");
    BB_REQUIRE(milliseconds >= 0, "bb_solver_sync_timeout: milliseconds < 0");
    BB_TRY(bb::enter_device(s->device));
    timespec t0;
    clock_gettime(CLOCK_MONOTONIC, &t0);
    for (;;) {
        const hipError_t e = hipStreamQuery(s->stream);
        if (e == hipSuccess) return BB_OK;
        if (e != hipErrorNotReady)
            return bb::hip_status("hipStreamQuery", e);
        (void)hipGetLastError();   // "not ready" is an answer, not a failure
        timespec t;
        clock_gettime(CLOCK_MONOTONIC, &t);
        const int64_t ms = (t.tv_sec - t0.tv_sec) * 1000 + (t.tv_nsec - t0.tv_nsec) / 1000000;
        if (ms >= milliseconds)
            return bb::fail(BB_ERR_STATE, "bb_solver_sync_timeout: the stream did not drain within " +
                                              std::to_string(milliseconds) + " ms");
        usleep(50);
    }
}

int bb_solver_set_timing(bb_solver *s, int enabled) {
    BB_REQUIRE(s != nullptr, "bb_solver_set_timing: solver is NULL");
    BB_TRY(bb::enter_device(s->device));
    BB_HIP_CHECK(hipStreamSynchronize(s->stream));
    if (enabled && s->ev.empty()) {
        s->ev.resize(3 * kMaxTimedLaunches);
        for (bb::Event &e : s->ev) BB_HIP_CHECK(e.create());
    }
    s->timing = enabled != 0;
    s->timing_stride = enabled > 1 ? enabled : 1;
    s->timing_iter = 0;
    s->ev_used = 0;
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
