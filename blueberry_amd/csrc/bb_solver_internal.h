// bb_solver_internal.h -- what the translation units of the 3D-structure solver share on the
// host: the bb_solver handle, the layout / dtype dispatchers, and the helpers that cross files.
//   bb_solver.hip           the handle, the sweep plan's device half, the launch layer, iterate
//   bb_solver_inputs.hip    every writer of the units, and the resident triples' handle
//   bb_solver_exchange.hip  the exchanges between ranks: RCCL (over bb_comm_cache.h), peer arenas
//   bb_solver_queries.hip   degrees and weight sums, the score, timing getters, probes
//   bb_solver_anchors.hip   landmark constraints
//   bb_solver_spectral.hip  the spectral start
//   bb_group.hip            several solvers of one process
// The library is built with hidden visibility: bb::solver:: names are external to a file, not
// to the library.
//
// Who owns what: every device allocation and event of a handle (bb_solver, bb_triples, bb_group)
// is a bb::DevBuf / bb::Event member of it (bb_common.h) and goes with the handle, or earlier
// by reset(); a staging buffer is such an owner as a local.  Plain pointers are views: into the
// solver's arena, or -- d_exch -- of own_exch or of a caller's memory.  The communicator is a
// bb::CommLease (bb_comm_cache.h: the cache's, or the solver's own) and what the peer exchange
// made a bb::solver::PeerLink; both are members and end with the handle like the rest.  The
// destroy functions keep only what has an order: the stream (the pool's), drained before the
// members go and given back after them.
#pragma once

#include <string>
#include <type_traits>
#include <vector>

#include "bb_comm.h"
#include "bb_common.h"
#include "bb_solver_device.h"
#include "bb_solver_plan.h"

namespace bb {
namespace solver {

// Everything bb_solver_peer_export and bb_solver_peer_connect make.  The arena's layout: 2
// parities x world slots of data | per-rank flags | poison words.
struct PeerLink {
    bb::DevBuf arena;                  // this rank's receive arena (uncached)
    int world = 1;                     // the solver's, as of the export: the arena's shape
    int64_t elem_bytes = 4, slot_elems = 0, arena_bytes = 0;
    std::vector<void *> mapped;        // arenas of all ranks as mapped here (own = arena)
    std::vector<void *> opened;        // the ones that came from hipIpcOpenMemHandle
    bb::DevBuf d_table;                // PeerTable<T>[2], one per parity
    bb::DevBuf d_table_x;              // PeerTableX<T>[2]: the one-launch exchange
    bool fused = true;                 // reduce_exchange_kernel (BB_PEER_FUSED=0: two launches)
    bb::DevBuf d_state;                // PeerState: sticky failure flag + last complete exchange
    int clock_khz = 100000;            // constant-rate clock behind wall_clock64()
    int ranks_on_gpu = 1;              // most ranks of the job on one GPU (a rehearsal: > 1)
    bb::DevBuf d_mask;                 // unsigned per block: the ranks whose units touch it (bit r)
    bb::DevBuf d_counter;              // unsigned: the reduce's two-level check-in
    unsigned long long seq = 0;        // iterations exchanged so far
    long long limit_ticks = 0;
    bool connected = false;

    PeerLink() = default;
    PeerLink(const PeerLink &) = delete;
    PeerLink &operator=(const PeerLink &) = delete;
    // the peers' arenas are closed before this rank's own buffers go (the members, after this)
    ~PeerLink() {
        for (void *m : opened) hipIpcCloseMemHandle(m);
    }

    int64_t flags_offset() const { return 2 * (int64_t)world * slot_elems * elem_bytes; }
    // the one-launch exchange (reduce_exchange_kernel): one poison word per source rank behind
    // the per-rank flags of the two-launch form (its data words say by themselves whether they
    // have arrived)
    int64_t xpoison_offset() const { return flags_offset() + bb::round_up((int64_t)world * 64, 256); }
    int64_t arena_size() const { return xpoison_offset() + bb::round_up((int64_t)world * 64, 256); }
};

}  // namespace solver
}  // namespace bb

struct bb_solver {
    int dtype = BB_F32, device = 0, rank = 0, world = 1;
    bool wide = true;  // unit shape (Lay<T, wide>): false only for small fp64 problems
    bb_layout_info L{};
    std::vector<int32_t> tile_I, tile_J;  // global tile list (device order)
    int64_t u_begin = 0, u_end = 0, n_local = 0;
    int64_t t_first = 0, n_local_tiles = 0;
    std::vector<int2> udesc;  // host copy

    hipStream_t stream = nullptr;
    bool own_stream = false;
    bool stream_stuck = false;     // behind a collective that cannot be aborted: never waited on again

    void *d_units = nullptr, *d_X = nullptr, *d_V = nullptr, *d_part = nullptr;
    // the exchange buffer: a view of own_exch, or -- own_exch empty -- the memory a caller gave
    // (bb_solver_set_exchange_buffer), which is never freed here
    void *d_exch = nullptr;
    bb::DevBuf own_exch;
    double momentum = 0.0;
    int2 *d_udesc = nullptr;
    int chunk_q = 0, chunk_r = 0;  // units per wave: n_local = n_waves * q + r
    bool nontemporal = true;
    bb::DevBuf d_arena;            // the one allocation behind every plain d_* pointer here (views of it)
    int2 *d_wave_slots = nullptr;  // per wave {first private slot, the workgroup's shared slot}
    int lds_wave_floats = 0;       // LDS region per wave of the sweep, in 4-byte words
    double *d_stresspart = nullptr;
    double *d_stress_slot = nullptr;     // one per column slot: the stress of a strip a wave left
    std::vector<int32_t> slot_strip;     // strip (block column) of every column slot
    std::vector<int32_t> wave_last_strip;  // strip each wave ends in, -1: no units
    // several maps in one solver (bb_solver_set_maps)
    int n_maps = 1;
    bb::DevBuf d_bin_scale;              // T per bin (n_pad): the factor on its gradient
    bb::DevBuf d_map_ptr, d_map_idx;     // int: the maps' lists of stress partials (CSR)
    bb::DevBuf d_map_scalar;             // double: per-map stress of bb_solver_stress_maps
    std::vector<int64_t> map_begin;      // first bin of every map, + n_bins
    int64_t *d_red_lists = nullptr;   // reduce_sliced_kernel: one padded chunk list per block
    int red_stride = 0, red_slices = 0;   // entries per block (multiple of 16 * slices); 4 or 8 slices
    double *d_stress_hist = nullptr, *d_stress_scalar = nullptr;
    double *d_f64_tmp = nullptr;  // (n_pad,3) staging for coordinate I/O
    bb::DevBuf d_mv_in;           // (n_pad,3) right-hand sides of bb_solver_matvec_sq, kept
    int64_t rowpart_elems = 0, colpart_elems = 0;
    int n_waves = 0, n_slots = 0;
    int wpb = 4;                   // waves per workgroup of the sweep: 4, or 8 (paired, see kernel)
    int dense_u0 = -1;             // dense tile list: this rank's first global unit (the kernel then
                                   // computes a wave's first descriptor), else -1
    int defer_cap_units = 0;       // fp32 / fp64 wide: units of row sums a wave can park in LDS
    int64_t defer_lds_bytes = 0;   // dynamic LDS per workgroup of the sweep
    unsigned defer_attr_done = 0;  // sweep instantiations whose dynamic-LDS ceiling was raised
    int64_t hist_cap = 0, hist_n = 0;
    bool have_wish = false, have_coords = false, grad_pending = false;
    // exchange_sum(): while set, the reduce / exchange kernels leave the plain sum over the
    // ranks HERE instead of stepping the coordinates (X := this buffer, zeroed; V := d_V;
    // mu = 0, lr = -1: 0 + (0 * v - (-1) * sum) is the sum, exactly)
    void *sum_target = nullptr;

    // row-owner path (small maps, world = 1): both triangles resident, one launch per
    // iteration (row_owner_kernel); the units stay resident too and serve every other
    // entry point (grad / apply, stress, matvec)
    bool row_owner = false;
    bool row_owner_built = false;        // created with the row-owner buffers (bb_solver_set_maps
                                         // switches row_owner off)
    bool bin_steps = false;              // d_bin_scale set by bb_solver_set_bin_steps / _block_steps
    int weight_power = 0;                // SPEC 2.3.1: w = delta^-q, q in {0, 1, 2}
    void *d_full = nullptr, *d_X2 = nullptr;
    int64_t full_ld = 0;
    double *d_ro_part = nullptr;   // 2 x ro_blocks per-workgroup stress sums (ping-pong)
    int ro_blocks = 0, ro_wpr = 1;  // workgroups holding rows; waves per row (1, 2, 4)
    int64_t ro_launches = 0;       // row-owner launches so far (parity of the ping-pong)

    // the 24-bit stream of the fp32 sweep (SPEC 3.7): derived from d_units, rebuilt by
    // ensure_pk24() before the first sweep after a writer of d_units (pk_stale)
    int pk_mode = -1;              // BB_PACK24 at create: 0 never, 1 whenever a unit packs, else the rule
    int64_t pk_min_run = 64;       // BB_PACK24_MIN_RUN at create: shortest run of units stored packed
    bool pk_stale = true, pk_valid = false;
    bb::DevBuf pk_stream, pk_table;   // outside the arena: the solver runs raw without them
    int64_t pk_packed = 0, pk_bytes = 0, pk_switches = 0;

    // landmark constraints (bb_solver_set_anchors, SPEC 2.5.5): the solver's own copy of the kept
    // rows in its dtype; anchor_n = 0: none, and every path is the one it was without them
    int anchor_n = 0;                    // kept rows L'
    double anchor_weight = 0.0;          // lambda
    int64_t anchor_terms = 0;            // values > 0 among the rows
    int anchor_chunks = 0, anchor_node_blocks = 0;
    bb::DevBuf anchor_rows;              // T (anchor_n, n_pad)
    bb::DevBuf anchor_nodes;             // int per kept row: its landmark's node
    bb::DevBuf anchor_part;              // double: anchor stress | per-workgroup stress | (a, chunk, 3)

    bool timing = false;
    int timing_stride = 1;      // events on every timing_stride-th iteration
    int64_t timing_iter = 0;    // iterations seen since timing was (re-)enabled
    std::vector<bb::Event> ev;   // triples: start, after grad, after reduce
    size_t ev_used = 0;
    double score_ms[3] = {0.0, 0.0, 0.0};   // the last timed bb_solver_score: profile, fold, per bin

    // the exchanges between ranks, declared last so that they end first: the communicator, then
    // the peers' arenas, then every buffer above
    bb::solver::PeerLink peer;      // peer exchange (bb_solver_peer_*)
    bb::CommLease comm;             // direct RCCL path (bb_solver_comm_init / _attach), else empty
};

namespace bb {
namespace solver {

// Which instantiation a launch takes.  The kernels exist for three layouts, (float, wide),
// (double, wide) and (double, narrow) (bb::wide_layout): by_layout(s, f) calls
// f(LayoutTag<T, W>{}) with the solver's, by_dtype(s, f) calls f(TypeTag<T>{}) where only the
// element type matters.  with_int<V...>(v, f) calls f(std::integral_constant<int, V>{}) for
// the first V equal to v, the last V standing for every other value.
template <typename TT>
struct TypeTag {
    using T = TT;
};
template <typename TT, bool WW>
struct LayoutTag {
    using T = TT;
    static constexpr bool W = WW;
};

template <typename F>
decltype(auto) by_layout(const bb_solver *s, F &&f) {
    if (s->dtype == BB_F32) return f(LayoutTag<float, true>{});
    if (s->wide) return f(LayoutTag<double, true>{});
    return f(LayoutTag<double, false>{});
}

template <typename F>
decltype(auto) by_dtype(const bb_solver *s, F &&f) {
    if (s->dtype == BB_F32) return f(TypeTag<float>{});
    return f(TypeTag<double>{});
}

template <int V, int... Rest, typename F>
decltype(auto) with_int(int v, F &&f) {
    if constexpr (sizeof...(Rest) == 0) return f(std::integral_constant<int, V>{});
    else return v == V ? f(std::integral_constant<int, V>{}) : with_int<Rest...>(v, f);
}

// A create that failed with rc: tear down what there is, the failure's text staying the last
// error across the tear-down.
template <typename TearDown>
int failed_create(int rc, TearDown &&tear_down) {
    const std::string keep = bb_last_error();
    tear_down();
    bb::set_error(keep);
    return rc;
}

// What the reduce multiplies the summed partials by: 2 for the gradient (SPEC 2.3: the sweep
// leaves half of it), 1 for a plain sum (the matvec of the spectral start) -- and only a
// gradient takes the per-bin step factors (fill_reduce_params).
constexpr double kScaleGradient = 2.0, kScalePlainSum = 1.0;

// Every environment variable the solver reads, as they stand at the time of the call: at
// bb_solver_create the knobs of the sweep plan (bb_solver_plan.h) and of the 24-bit stream, the
// row-owner limit and the descriptor form; at bb_solver_peer_connect the peer ones.  THE place
// the solver reads its environment is solver_env() (bb_solver.hip).
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

// ---- bb_solver.hip ----
SolverEnv solver_env();
int check_ready(const bb_solver *s, const char *who);
int check_iterate(const bb_solver *s, int64_t iters, const char *who);
hipError_t upload_padded(const bb_solver *s, double *dst, const double *rows, hipStream_t stream);
hipError_t widen(bb_solver *s, const void *in_T, double *out_f64, int64_t n);
hipError_t narrow(bb_solver *s, const double *in_f64, void *out_T, int64_t n);
int ensure_pk24(bb_solver *s);
int launch_grad(bb_solver *s, int op = kOpStress, const void *x_in = nullptr);
int launch_reduce(bb_solver *s, int mode, double lr, double *stress_out, double scale = kScaleGradient);
int launch_exchange(bb_solver *s, double lr, double *stress_out, double scale = kScaleGradient);
int launch_apply(bb_solver *s, double lr, double *stress_out);
int enable_peer_access(const char *who, int device);
// ---- bb_solver_anchors.hip ----
int launch_anchors(bb_solver *s, int fold, double *stress_out = nullptr);
// ---- bb_solver_exchange.hip ----
int launch_peer_receive(bb_solver *s, void *X, double lr, double mu, double *stress_out);
int contributor_mask(const bb_solver *s, std::vector<unsigned> *mask);
int exchange_sum(bb_solver *s);

// One iteration's two halves, sweep() and reduce(), with the timing events around them on
// every timing_stride-th iteration while timing is on: ev[0] sweep ev[1] reduce ev[2].
template <typename Sweep, typename Reduce>
int timed_step(bb_solver *s, Sweep &&sweep, Reduce &&reduce) {
    bb::Event *ev = nullptr;
    if (s->timing && s->timing_iter++ % s->timing_stride == 0 && s->ev_used + 3 <= s->ev.size()) {
        ev = &s->ev[s->ev_used];
        s->ev_used += 3;
    }
    if (ev) BB_HIP_CHECK(hipEventRecord(ev[0], s->stream));
    BB_TRY(sweep());
    if (ev) BB_HIP_CHECK(hipEventRecord(ev[1], s->stream));
    BB_TRY(reduce());
    if (ev) BB_HIP_CHECK(hipEventRecord(ev[2], s->stream));
    return BB_OK;
}

}  // namespace solver
}  // namespace bb
