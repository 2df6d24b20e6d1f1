// bb_solver.hip -- host side of the 3D-structure solver of libblueberry_hip.so: the
// bb_solver handle's create / destroy (the partition itself is bb_solver_plan.cpp: no device
// call), the launch layer -- every launch of the sweep, the reduce, the one-launch exchange,
// the apply and the row-owner kernel, for all files of the solver -- and the entry points that
// set coordinates, steps and maps, iterate, and read the stress.  The kernels are in
// bb_solver_kernels.h, compiled here and nowhere else.  The handle, and the parts of the
// solver that have a file of their own (input routes, exchanges between ranks, queries,
// landmark constraints, spectral start, groups): bb_solver_internal.h.  The environment is
// read in solver_env().  gfx950 only.
//
// Specification: docs/SPEC.md (build-authored; the reference has no solver,
// SURVEY.md section 0).  Data layout and kernel design: DESIGN.md 3-4.
#include <math.h>
#include <stdlib.h>
#include <time.h>
#include <unistd.h>

#include <algorithm>
#include <cmath>

#include "bb_solver_internal.h"
#include "bb_solver_kernels.h"

using namespace bb::solver;

namespace bb {
namespace solver {

constexpr int64_t kHistCap = 1 << 20;
constexpr size_t kMaxTimedLaunches = 4096;

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

// THE place the solver reads its environment (SolverEnv: bb_solver_internal.h).
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
    // Never where ranks share a GPU (a rehearsal: peer.ranks_on_gpu > 1).  The packed sweep takes
    // the registers of the one or two waves per SIMD it runs with; beside the waiting receive
    // kernels of the other ranks its workgroups find no CU to start on, and every rank waits for
    // a partial nobody can compute (tools/world8_rehearsal.py ran into its time limit that way).
    const bool want = s->dtype == BB_F32 && n > 0 && s->pk_mode != 0 && s->peer.ranks_on_gpu <= 1 &&
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

// The peer exchange in one launch (reduce_exchange_kernel): the caller has bumped peer.seq.
template <typename T, bool W>
int launch_exchange_t(LayoutTag<T, W>, bb_solver *s, double lr, double *stress_out, double scale) {
    ReduceParams<T> p;
    fill_reduce_params<T>(s, p, kReducePeer, lr, stress_out, scale);
    const int64_t es = sizeof(T);
    const unsigned segs = 3 * Lay<T, W>::VW / kRedWG;
    const dim3 grid((unsigned)s->L.n_blocks, segs);
    const PeerTableX<T> *xt = s->peer.d_table_x.as<const PeerTableX<T>>() + (s->peer.seq & 1);
    const char *base = s->peer.arena.as<const char>();
    const T *arena = (const T *)(base + (int64_t)(s->peer.seq & 1) * s->world * s->peer.slot_elems * es);
    const unsigned long long *my_poison = (const unsigned long long *)(base + s->peer.xpoison_offset());
    return with_int<4, 8>(s->red_slices, [&](auto slices) -> int {
        constexpr int S = decltype(slices)::value;
        BB_HIP_CHECK(bb::launch(reduce_exchange_kernel<T, W, S>, grid, dim3(128 * S), 0, s->stream, p,
                                (const int64_t *)s->d_red_lists, s->red_stride, xt, arena, my_poison,
                                s->peer.slot_elems, s->peer.d_state.as<PeerState>(),
                                s->peer.limit_ticks));
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
    p.peer_counter = s->peer.d_counter.as<unsigned>();
    p.peer_state = s->peer.d_state.as<PeerState>();
    p.seq = 0;
    p.n_peers = 0;
    if (mode == kReducePeer) {
        // the caller has bumped peer.seq: iteration k (1-based) uses parity k & 1
        p.peer = s->peer.d_table.as<const PeerTable<T>>() + (s->peer.seq & 1);
        p.seq = s->peer.seq;
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
    p.peer_mask = s->peer.d_mask.as<unsigned>();
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
    // the communicator, the peers' arenas, buffers and events go with the handle, in that order;
    // the stream back to the pool after them (one abandoned behind a hung collective does not:
    // the pool synchronises what it takes back)
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

int bb_solver_set_weight_power(bb_solver *s, int q) {
    BB_REQUIRE(s != nullptr, "bb_solver_set_weight_power: solver is NULL");
    BB_REQUIRE(q >= 0 && q <= 2, "bb_solver_set_weight_power: q must be 0, 1 or 2");
    if (s->grad_pending)
        return bb::fail(BB_ERR_STATE, "bb_solver_set_weight_power: a bb_solver_grad is pending");
    s->weight_power = q;           // (the stress history is kept: each entry is the S_q of its step)
    return BB_OK;
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

}  // extern "C"
