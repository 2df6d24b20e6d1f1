// bb_solver_exchange.hip -- the exchanges between the ranks of the 3D-structure solver: the
// library's RCCL communicator (the bb_comm_* / bb_solver_comm_* entry points over the cache and
// the lease of bb_comm_cache.h, the all-reduce, bb_solver_iterate_dist), the peer arenas
// (bb_solver_peer_*: export, connect, the form and the status, bb_solver_iterate_peer), the
// plain sum over the ranks the spectral start takes (exchange_sum) and the exchange-buffer
// entry points.  peer_receive_kernel (bb_peer_kernels.h) is compiled here and nowhere else;
// every other launch goes through the launch layer of bb_solver.hip.  The handle:
// bb_solver_internal.h.  gfx950 only.
//
// Specification: docs/SPEC.md.  Design of the exchanges: DESIGN.md 4.3.
#include <stddef.h>
#include <string.h>
#include <unistd.h>

#include <algorithm>
#include <map>

#include "bb_peer_kernels.h"
#include "bb_solver_internal.h"

using namespace bb::solver;

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
    const int64_t foff = s->peer.flags_offset();
    for (int par = 0; par < 2; ++par)
        for (int q = 0; q < s->world; ++q) {
            char *base = (char *)s->peer.mapped[q];
            tab[par].dst[q] = (T *)base + ((int64_t)par * s->world + s->rank) * s->peer.slot_elems;
            tab[par].flag[q] = (unsigned long long *)(base + foff) + 8 * s->rank;
        }
    BB_TRY(bb::alloc_status(s->peer.d_table, sizeof(tab)));
    BB_HIP_CHECK(hipMemcpy(s->peer.d_table.p, tab, sizeof(tab), hipMemcpyHostToDevice));
    PeerTableX<T> tx[2];
    memset(tx, 0, sizeof(tx));
    for (int par = 0; par < 2; ++par)
        for (int q = 0; q < s->world; ++q) {
            char *base = (char *)s->peer.mapped[q];
            tx[par].dst[q] = tab[par].dst[q];
            tx[par].poison[q] = (unsigned long long *)(base + s->peer.xpoison_offset()) + 8 * s->rank;
        }
    BB_TRY(bb::alloc_status(s->peer.d_table_x, sizeof(tx)));
    BB_HIP_CHECK(hipMemcpy(s->peer.d_table_x.p, tx, sizeof(tx), hipMemcpyHostToDevice));
    return BB_OK;
}

namespace {
// The "not connected" check of the small peer entry points, in who's name.
int check_connected(const bb_solver *s, const char *who) {
    if (!s->peer.connected) return bb::fail(BB_ERR_STATE, std::string(who) + ": not connected");
    return BB_OK;
}

int enqueue_allreduce(bb_solver *s) {
    const bb::Rccl &R = bb::rccl();
    const int rc = R.AllReduce(s->d_exch, s->d_exch, (size_t)(3 * s->L.n_pad + 2),
                               s->dtype == BB_F32 ? bb::Rccl::kFloat32 : bb::Rccl::kFloat64,
                               bb::Rccl::kSum, s->comm.comm(), s->stream);
    if (rc != bb::Rccl::kSuccess) {
        s->comm.mark_suspect();      // its peers may now sit in a collective this rank left
        return bb::fail(BB_ERR_HIP, std::string("ncclAllReduce: ") + R.GetErrorString(rc));
    }
    return BB_OK;
}
}  // namespace

// The receiving half of the two-launch peer exchange (peer_receive_kernel): wait for every
// rank's flag of exchange `peer.seq`, X <- X + (mu V - lr * sum over the ranks in rank order).
int launch_peer_receive(bb_solver *s, void *X, double lr, double mu, double *stress_out) {
    const int64_t n3 = s->L.n_pad * 3, es = bb::elem_size(s->dtype);
    // Ranks that share a GPU (a rehearsal) share its wave slots too: the receive kernels of ALL
    // of them wait at once, and eight times 256 workgroups of 4 waves are every slot the chip
    // has -- nobody's sweep could start (found by tools/world8_rehearsal.py).  The cap is
    // divided among them; a thread then takes more elements.
    const int64_t cap = std::max<int64_t>(8, (int64_t)kPeerReceiveWGs / (s->peer.ranks_on_gpu > 2 ? s->peer.ranks_on_gpu / 2 : 1));
    const unsigned grid = (unsigned)std::min<int64_t>((n3 + 255) / 256, cap);
    const char *arena = s->peer.arena.as<const char>() +
                        (int64_t)(s->peer.seq & 1) * s->world * s->peer.slot_elems * es;
    const unsigned long long *flags =
        (const unsigned long long *)(s->peer.arena.as<const char>() + s->peer.flags_offset());
    // the flag pointers are the second half of a PeerTable (same for both parities)
    unsigned long long *const *poison =
        (unsigned long long *const *)(s->peer.d_table.as<const char>() + kMaxPeers * sizeof(void *));
    return by_dtype(s, [&](auto t) -> int {
        using T = typename decltype(t)::T;
        BB_HIP_CHECK(bb::launch(peer_receive_kernel<T>, dim3(grid), dim3(256), 0, s->stream, (T *)X,
                                (T *)s->d_V, (const T *)arena, flags, poison, s->world, s->peer.slot_elems,
                                n3, (T)lr, (T)mu, stress_out, s->peer.seq, s->peer.d_state.as<PeerState>(),
                                s->peer.limit_ticks, s->peer.d_mask.as<const unsigned>(), (int)(3 * s->L.vw)));
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
    if (s->peer.connected) {        // (also a one-rank solver that pushes to itself: a rehearsal)
        BB_HIP_CHECK(hipMemsetAsync(s->d_exch, 0, (size_t)(n3 * es), s->stream));
        s->peer.seq++;
        s->sum_target = s->d_exch;
        int rc;
        if (s->peer.fused) {
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

int bb_comm_cached_generation(int device, int rank, int world, int *available,
                              uint64_t *generation) {
    BB_REQUIRE(available != nullptr && generation != nullptr,
               "bb_comm_cached_generation: NULL argument");
    bool have = false;
    bb::comm_cache().peek(device, rank, world, &have, generation);
    *available = have ? 1 : 0;
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
    s->comm = bb::comm_cache().attach(s->device, s->rank, s->world);
    if (!s->comm) return bb::fail(BB_ERR_STATE, "bb_solver_comm_attach: no free cached communicator");
    return BB_OK;
}

int bb_solver_comm_detach(bb_solver *s) {
    BB_REQUIRE(s != nullptr, "bb_solver_comm_detach: solver is NULL");
    if (!s->comm.detach())
        return bb::fail(BB_ERR_STATE, "bb_solver_comm_detach: the communicator is the solver's own");
    return BB_OK;
}

int bb_comm_cache_clear(void) {
    bb::comm_cache().clear();
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
    bb::Rccl::Comm c = nullptr;
    const int rc = R.CommInitRank(&c, s->world, id, s->rank);
    if (rc != bb::Rccl::kSuccess)
        return bb::fail(BB_ERR_HIP, std::string("ncclCommInitRank: ") + R.GetErrorString(rc));
    // into the cache, unless another solver holds this key's entry right now
    s->comm = bb::comm_cache().adopt(s->device, s->rank, s->world, c, unique_id);
    return BB_OK;
}

int bb_solver_comm_abort(bb_solver *s) {
    BB_REQUIRE(s != nullptr, "bb_solver_comm_abort: solver is NULL");
    if (!s->comm) return BB_OK;
    // out of the cache -- it is not handed out again -- and aborted: ncclCommAbort ends the
    // communicator's in-flight kernels, so a stream that is stuck behind a collective a peer
    // never joined drains again
    int rc = bb::Rccl::kSuccess;
    const bool leaked = s->comm.abort(&rc) != nullptr;
    s->grad_pending = false;
    if (leaked) {
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
    if (rc != bb::Rccl::kSuccess)
        return bb::fail(BB_ERR_HIP, std::string("ncclCommAbort: ") + bb::rccl().GetErrorString(rc));
    return BB_OK;
}

int bb_solver_comm_world(const bb_solver *s, int *world) {
    BB_REQUIRE(s != nullptr && world != nullptr, "bb_solver_comm_world: NULL argument");
    *world = 0;
    if (!s->comm) return bb::fail(BB_ERR_STATE, "bb_solver_comm_world: no communicator");
    const bb::Rccl &R = bb::rccl();
    if (!R.CommCount) return bb::fail(BB_ERR_HIP, "bb_solver_comm_world: ncclCommCount missing");
    const int rc = R.CommCount(s->comm.comm(), world);
    if (rc != bb::Rccl::kSuccess)
        return bb::fail(BB_ERR_HIP, std::string("ncclCommCount: ") + R.GetErrorString(rc));
    return BB_OK;
}

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

int bb_solver_peer_export(bb_solver *s, void *handle_out) {
    BB_REQUIRE(s != nullptr && handle_out != nullptr, "bb_solver_peer_export: NULL argument");
    BB_REQUIRE(s->world <= kMaxPeers, "bb_solver_peer_export: world > 16");
    if (s->peer.arena) return bb::fail(BB_ERR_STATE, "bb_solver_peer_export: already exported");
    BB_TRY(bb::enter_device(s->device));
    const int64_t es = bb::elem_size(s->dtype);
    s->peer.world = s->world, s->peer.elem_bytes = es;
    s->peer.slot_elems = bb::round_up(3 * s->L.n_pad + 2, 256 / es);
    s->peer.arena_bytes = s->peer.arena_size();
    // Uncached: written by the peers' kernels while ours is running, so nothing of
    // it may live in this GPU's L2.  (RCCL allocates its own buffers the same way.)
    void *arena = nullptr;
    hipError_t e = hipExtMallocWithFlags(&arena, (size_t)s->peer.arena_bytes, hipDeviceMallocUncached);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        e = hipExtMallocWithFlags(&arena, (size_t)s->peer.arena_bytes, hipDeviceMallocFinegrained);
    }
    if (e != hipSuccess) {
        return bb::fail(BB_ERR_NOMEM, std::string("bb_solver_peer_export: arena: ") +
                                          hipGetErrorString(e));
    }
    // every data word starts out EMPTY (all bits set: reduce_exchange_kernel), flags and poison
    // words at 0
    s->peer.arena.adopt(arena, (size_t)s->peer.arena_bytes);
    BB_HIP_CHECK(hipMemset(s->peer.arena.p, 0xff, (size_t)s->peer.flags_offset()));
    BB_HIP_CHECK(hipMemset(s->peer.arena.as<char>() + s->peer.flags_offset(), 0,
                           (size_t)(s->peer.arena_bytes - s->peer.flags_offset())));
    BB_HIP_CHECK(hipDeviceSynchronize());
    PeerHandle h;
    memset(&h, 0, sizeof(h));
    e = hipIpcGetMemHandle(&h.ipc, s->peer.arena.p);
    if (e != hipSuccess) {
        s->peer.arena.reset();
        return bb::fail(BB_ERR_HIP, std::string("bb_solver_peer_export: hipIpcGetMemHandle: ") +
                                        hipGetErrorString(e));
    }
    h.magic = kPeerMagic;
    h.arena_bytes = s->peer.arena_bytes;
    h.slot_elems = s->peer.slot_elems;
    h.pid = (int64_t)getpid();
    h.raw = (uint64_t)(uintptr_t)s->peer.arena.p;
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
    if (!s->peer.arena) return bb::fail(BB_ERR_STATE, "bb_solver_peer_connect: export first");
    if (s->peer.connected) return bb::fail(BB_ERR_STATE, "bb_solver_peer_connect: already connected");
    BB_TRY(bb::enter_device(s->device));
    const SolverEnv env = solver_env();
    s->peer.mapped.assign((size_t)s->world, nullptr);
    std::map<uint64_t, int> ranks_on_gpu;      // how many ranks sit on each GPU of the node
    int most_on_one_gpu = 1;
    for (int r = 0; r < s->world; ++r) {
        PeerHandle h;
        memcpy(&h, (const char *)handles + (size_t)r * BB_PEER_HANDLE_BYTES, sizeof(h));
        most_on_one_gpu = std::max(most_on_one_gpu, ++ranks_on_gpu[h.pci]);
        if (h.magic != kPeerMagic || h.rank != r || h.world != s->world || h.dtype != s->dtype ||
            h.arena_bytes != s->peer.arena_bytes || h.slot_elems != s->peer.slot_elems)
            return bb::fail(BB_ERR_INVALID, "bb_solver_peer_connect: handle " + std::to_string(r) +
                                                " does not match this solver (rank order, world, "
                                                "dtype and n_bins must agree)");
        if (r == s->rank) {
            s->peer.mapped[r] = s->peer.arena.p;
        } else if (h.pid == (int64_t)getpid()) {
            // same process: the exporter's pointer is valid here, but only from the
            // same device or with peer access
            if (h.device != s->device)
                BB_TRY(enable_peer_access("bb_solver_peer_connect: peer access", h.device));
            s->peer.mapped[r] = (void *)(uintptr_t)h.raw;
        } else {
            void *ptr = nullptr;
            hipError_t e = hipIpcOpenMemHandle(&ptr, h.ipc, hipIpcMemLazyEnablePeerAccess);
            if (e != hipSuccess)
                return bb::fail(BB_ERR_HIP, "bb_solver_peer_connect: hipIpcOpenMemHandle(rank " +
                                                std::to_string(r) + "): " + hipGetErrorString(e));
            s->peer.mapped[r] = ptr;
            s->peer.opened.push_back(ptr);
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
        s->peer.d_mask.reset();
        if (env.peer_mask && s->world <= 32) {
            std::vector<unsigned> mask;
            BB_TRY(contributor_mask(s, &mask));
            BB_TRY(bb::alloc_status(s->peer.d_mask, mask.size() * sizeof(unsigned)));
            BB_HIP_CHECK(hipMemcpy(s->peer.d_mask.p, mask.data(), mask.size() * sizeof(unsigned),
                                   hipMemcpyHostToDevice));
        }
    }
    BB_TRY(bb::alloc_status(s->peer.d_state, sizeof(PeerState)));
    // the top counter + one per block on a line of its own (reduce_sliced_kernel's two-level
    // check-in)
    const int64_t n_counters = 32 * (s->L.n_blocks + 1);
    BB_TRY(bb::alloc_status(s->peer.d_counter, (size_t)n_counters * sizeof(unsigned)));
    BB_HIP_CHECK(hipMemset(s->peer.d_state.p, 0, sizeof(PeerState)));
    BB_HIP_CHECK(hipMemset(s->peer.d_counter.p, 0, (size_t)n_counters * sizeof(unsigned)));
    // ticks of wall_clock64(): ask the runtime, fall back to gfx9's 100 MHz.  The query
    // is allowed to fail (older runtimes); its error is consumed here, on the spot.
    int khz = 0;
    if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, s->device) != hipSuccess) {
        (void)hipGetLastError();
        khz = 0;
    }
    s->peer.clock_khz = khz > 0 ? khz : 100000;
    s->peer.limit_ticks = env.peer_timeout_ms * s->peer.clock_khz;
    s->peer.seq = 0;
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
        s->peer.fused = env.peer_fused >= 0 ? env.peer_fused != 0 : most_on_one_gpu == 1;
        s->peer.ranks_on_gpu = most_on_one_gpu;
        if (most_on_one_gpu > 1) s->pk_stale = true;   // a stream built before this goes (ensure_pk24)
    }
    s->peer.connected = true;
    BB_HIP_CHECK(hipDeviceSynchronize());
    return BB_OK;
}

int bb_solver_peer_set_timeout(bb_solver *s, int64_t milliseconds) {
    BB_REQUIRE(s != nullptr, "bb_solver_peer_set_timeout: solver is NULL");
    BB_REQUIRE(milliseconds > 0 && milliseconds <= 3600000,
               "bb_solver_peer_set_timeout: need 0 < ms <= 3600000");
    BB_TRY(check_connected(s, "bb_solver_peer_set_timeout"));
    s->peer.limit_ticks = (long long)milliseconds * s->peer.clock_khz;
    return BB_OK;
}

int bb_solver_peer_set_form(bb_solver *s, int one_launch) {
    BB_REQUIRE(s != nullptr, "bb_solver_peer_set_form: solver is NULL");
    BB_TRY(check_connected(s, "bb_solver_peer_set_form"));
    // the one-launch form reads "empty" in every slot word it has not been sent: it can only
    // be chosen while no exchange has run (the two-launch form leaves its partials in the slots)
    if (s->peer.seq != 0)
        return bb::fail(BB_ERR_STATE, "bb_solver_peer_set_form: exchanges have already run");
    s->peer.fused = one_launch != 0;
    return BB_OK;
}

int bb_solver_peer_form(bb_solver *s, int *one_launch) {
    BB_REQUIRE(s != nullptr && one_launch != nullptr, "bb_solver_peer_form: NULL argument");
    BB_TRY(check_connected(s, "bb_solver_peer_form"));
    *one_launch = s->peer.fused ? 1 : 0;
    return BB_OK;
}

int bb_solver_peer_status(bb_solver *s, int *status) {
    BB_REQUIRE(s != nullptr, "bb_solver_peer_status: solver is NULL");
    BB_TRY(check_connected(s, "bb_solver_peer_status"));
    BB_TRY(bb::enter_device(s->device));
    PeerState st;
    memset(&st, 0, sizeof(st));
    BB_HIP_CHECK(hipStreamSynchronize(s->stream));
    BB_HIP_CHECK(hipMemcpy(&st, s->peer.d_state.p, sizeof(st), hipMemcpyDeviceToHost));
    if (status) *status = st.status;
    if (st.status != 0) {
        const bool one = s->peer.fused;
        return bb::fail(BB_ERR_STATE,
                        std::string("peer exchange: a rank did not deliver its partial within the "
                                    "time limit (BB_PEER_TIMEOUT_MS), or reported its own failure; ") +
                            (one ? "the last exchange this rank completed whole was "
                                 : "this rank's coordinates were left at its last completed step (") +
                            std::to_string(st.verdict) + " of " + std::to_string(s->peer.seq) +
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
    if (!s->peer.connected)
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
            s->peer.seq++;
            return s->peer.fused ? launch_exchange(s, lr, hist) : launch_reduce(s, kReducePeer, 0.0, nullptr);
        }));
        if (!s->peer.fused) BB_TRY(launch_peer_receive(s, s->d_X, lr, s->momentum, hist));
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
}  // extern "C"
