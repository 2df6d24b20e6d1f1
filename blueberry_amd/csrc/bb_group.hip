// bb_group.hip -- groups of 3D-structure solvers that one process drives on several devices
// (bb_group_*), one host thread each, and the one kernel that is theirs.  A member's sweep,
// reduce and landmark terms are the solver's own (bb_solver_internal.h).  gfx950 only.
#include <condition_variable>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "bb_group_barrier.h"
#include "bb_solver_internal.h"

using namespace bb::solver;

namespace {

// ---- the event-ordered exchange of a group (bb_group_*: several solvers of ONE process) ----
// src[r] (a device-side table, local or peer pointers) is member r's exchange buffer
// [g (n_pad,3) | stress hi | lo], left there by bb_solver_grad's reduce: the same partial the
// peer-mode reduce pushes (scale and per-bin factor applied the same way).  The host has
// ordered this launch behind every member's grad by events, so nothing here waits or polls.
// Per element: the sum over members is peer_receive_kernel's (rank_ordered_sums: member order
// from 0, a masked-out member adds 0), then V <- mu V - lr g, X <- X + V.  The stress: (hi, lo)
// summed in double, in order.
template <typename T>
__global__ __launch_bounds__(256) void group_apply_kernel(
    T *__restrict__ X, T *__restrict__ V, const T *const *__restrict__ src, int world, int64_t n3,
    T lr, T mu, double *__restrict__ stress_out, const unsigned *__restrict__ peer_mask, int ch) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e < n3) {
        const unsigned mk[1] = {peer_mask != nullptr ? peer_mask[e / ch] : ~0u};
        const bool live[1] = {true};
        T g[1];
        rank_ordered_sums(g, live, mk, world, [&](int, int r) { return src[r][e]; });
        momentum_step(X, V, e, mu, lr, g[0]);
    }
    if (e == 0) {
        double S = 0.0;
        for (int r = 0; r < world; ++r) S += (double)src[r][n3] + (double)src[r][n3 + 1];
        *stress_out = S;
    }
}

}  // namespace

// ---- groups: several solvers of ONE process, one host thread each (bb_group_*) ----------
// The exchange of a group is ordered by HIP events alone: no kernel waits for another, so
// members may share a GPU (and its hardware queues) in any number.  DESIGN.md 6.9.
namespace {

constexpr int kGroupAborted = -1;   // a member that left because another one failed

}  // namespace

struct bb_group {
    std::vector<bb_solver *> m;         // member r = rank r of world m.size()
    std::vector<void *> exch;           // the members' exchange buffers the tables point to
    std::vector<bb::DevBuf> d_src;      // per member, on its device: the R exchange pointers
    std::vector<bb::DevBuf> d_mask;     // per member, on its device: block -> contributing ranks (unsigned)
    std::vector<bb::Event> ready, applied;
    std::vector<std::thread> threads;
    // one job at a time, handed to the threads under `mu`
    std::mutex mu;
    std::condition_variable cv_job, cv_done;
    uint64_t job = 0;
    int done = 0;
    bool quit = false;
    int64_t iters = 0;
    double lr = 0.0;
    bb::GroupBarrier bar;
    std::vector<int> rc;
    std::vector<std::string> err;
};

namespace {

// Steps 1-2 of an iteration on member r's stream: wait until every member has applied the
// previous step (its group_apply_kernel read this member's partial: WAR), grad, "ready".
int group_grad(bb_group *g, int r) {
    bb_solver *s = g->m[(size_t)r];
    for (const bb::Event &e : g->applied) BB_HIP_CHECK(hipStreamWaitEvent(s->stream, e, 0));
    BB_TRY(launch_grad(s));
    BB_TRY(launch_reduce(s, kReduceExchange, 0.0, nullptr));
    if (s->anchor_n > 0) BB_TRY(launch_anchors(s, kAnchorFoldExchange));   // (a group of one: world 1)
    BB_HIP_CHECK(hipEventRecord(g->ready[(size_t)r], s->stream));
    return BB_OK;
}

// Step 4: wait for every member's partial, sum in rank order and step, "applied".
int group_apply(bb_group *g, int r) {
    bb_solver *s = g->m[(size_t)r];
    for (const bb::Event &e : g->ready) BB_HIP_CHECK(hipStreamWaitEvent(s->stream, e, 0));
    const int64_t n3 = s->L.n_pad * 3;
    const dim3 grid((unsigned)((n3 + 255) / 256)), block(256);
    const int world = (int)g->m.size(), ch = (int)(3 * s->L.vw);
    double *hist = s->d_stress_hist + s->hist_n;
    BB_TRY(by_dtype(s, [&](auto t) -> int {
        using T = typename decltype(t)::T;
        BB_HIP_CHECK(bb::launch(group_apply_kernel<T>, grid, block, 0, s->stream, (T *)s->d_X, (T *)s->d_V,
                                g->d_src[(size_t)r].as<const T *const>(), world, n3, (T)g->lr, (T)s->momentum,
                                hist, g->d_mask[(size_t)r].as<unsigned>(), ch));
        return BB_OK;
    }));
    BB_HIP_CHECK(hipEventRecord(g->applied[(size_t)r], s->stream));
    s->hist_n++;
    return BB_OK;
}

// One member's share of a bb_group_iterate.  The barriers put every record of an event before
// every wait that refers to it; a member that fails to enqueue makes all of them leave at the
// next barrier, before anybody waits on something it will not record.
int group_run(bb_group *g, int r) {
    static_assert(BB_OK == 0, "bb::group_steps takes 0 for success");
    return bb::group_steps(g->bar, g->iters, bb::enter_device(g->m[(size_t)r]->device),
                           kGroupAborted, [&](int64_t) { return group_grad(g, r); },
                           [&](int64_t) { return group_apply(g, r); });
}

void group_worker(bb_group *g, int r) {
    (void)hipSetDevice(g->m[(size_t)r]->device);
    uint64_t seen = 0;
    for (;;) {
        {
            std::unique_lock<std::mutex> lk(g->mu);
            g->cv_job.wait(lk, [&] { return g->quit || g->job != seen; });
            if (g->quit) return;
            seen = g->job;
        }
        const int rc = group_run(g, r);
        std::lock_guard<std::mutex> lk(g->mu);
        g->rc[(size_t)r] = rc;
        g->err[(size_t)r] = rc > 0 ? std::string(bb_last_error()) : std::string();
        if (++g->done == (int)g->m.size()) g->cv_done.notify_all();
    }
}

void group_free(bb_group *g) {
    {
        std::lock_guard<std::mutex> lk(g->mu);
        g->quit = true;
    }
    g->cv_job.notify_all();
    for (std::thread &t : g->threads) t.join();
    for (size_t r = 0; r < g->m.size(); ++r) {
        hipSetDevice(g->m[r]->device);
        hipStreamSynchronize(g->m[r]->stream);
        // (each is made or empty: a setup that failed half way leaves the rest empty)
        g->ready[r].reset();
        g->applied[r].reset();
        g->d_src[r].reset();
        g->d_mask[r].reset();
    }
    delete g;
    (void)hipGetLastError();
}

int group_setup(bb_group *g) {
    const int n = (int)g->m.size();
    // peer access between every pair of DISTINCT devices (a repeated device needs none)
    for (int a = 0; a < n; ++a)
        for (int b = 0; b < n; ++b) {
            const int da = g->m[(size_t)a]->device, db = g->m[(size_t)b]->device;
            if (da == db) continue;
            int can = 0;
            BB_HIP_CHECK(hipDeviceCanAccessPeer(&can, da, db));
            if (!can)
                return bb::fail(BB_ERR_HIP, "bb_group_create: device " + std::to_string(da) +
                                                " has no peer access to device " + std::to_string(db));
            BB_TRY(bb::enter_device(da));
            BB_TRY(enable_peer_access("bb_group_create: hipDeviceEnablePeerAccess", db));
        }
    std::vector<unsigned> mask;
    BB_TRY(contributor_mask(g->m[0], &mask));
    for (int r = 0; r < n; ++r) {
        bb_solver *s = g->m[(size_t)r];
        BB_TRY(bb::enter_device(s->device));
        BB_HIP_CHECK(hipStreamSynchronize(s->stream));
        BB_TRY(bb::alloc_status(g->d_src[(size_t)r], n * sizeof(void *)));
        BB_HIP_CHECK(hipMemcpy(g->d_src[(size_t)r].p, g->exch.data(), n * sizeof(void *),
                               hipMemcpyHostToDevice));
        BB_TRY(bb::alloc_status(g->d_mask[(size_t)r], mask.size() * sizeof(unsigned)));
        BB_HIP_CHECK(hipMemcpy(g->d_mask[(size_t)r].p, mask.data(), mask.size() * sizeof(unsigned),
                               hipMemcpyHostToDevice));
        BB_HIP_CHECK(g->ready[(size_t)r].create(hipEventDisableTiming));
        BB_HIP_CHECK(g->applied[(size_t)r].create(hipEventDisableTiming));
        // recorded once, so that the first iteration's waits refer to a completed record
        BB_HIP_CHECK(hipEventRecord(g->applied[(size_t)r], s->stream));
        BB_HIP_CHECK(hipEventRecord(g->ready[(size_t)r], s->stream));
    }
    for (int r = 0; r < n; ++r) {
        try {
            g->threads.emplace_back(group_worker, g, r);
        } catch (...) {
            return bb::fail(BB_ERR_NOMEM, "bb_group_create: cannot start a host thread");
        }
    }
    return BB_OK;
}

}  // namespace

extern "C" {

int bb_group_create(bb_group **out, bb_solver *const *members, int n) {
    BB_REQUIRE(out != nullptr && members != nullptr, "bb_group_create: NULL argument");
    *out = nullptr;
    BB_REQUIRE(n >= 1 && n <= kMaxPeers, "bb_group_create: need 1 <= n <= 16 members");
    for (int r = 0; r < n; ++r) {
        const bb_solver *s = members[r];
        const bb_solver *s0 = members[0];
        if (!s) return bb::fail(BB_ERR_INVALID, "bb_group_create: member " + std::to_string(r) + " is NULL");
        if (s->rank != r || s->world != n)
            return bb::fail(BB_ERR_INVALID, "bb_group_create: member " + std::to_string(r) +
                                                " is rank " + std::to_string(s->rank) + " of world " +
                                                std::to_string(s->world) + "; member r must be rank r "
                                                "of world " + std::to_string(n));
        if (s->L.n_bins != s0->L.n_bins)
            return bb::fail(BB_ERR_INVALID, "bb_group_create: member " + std::to_string(r) +
                                                " has n_bins " + std::to_string(s->L.n_bins) +
                                                ", member 0 " + std::to_string(s0->L.n_bins));
        if (s->dtype != s0->dtype)
            return bb::fail(BB_ERR_INVALID, "bb_group_create: member " + std::to_string(r) +
                                                " has another dtype than member 0");
        if (s->tile_I != s0->tile_I || s->tile_J != s0->tile_J)
            return bb::fail(BB_ERR_INVALID, "bb_group_create: member " + std::to_string(r) +
                                                " has another tile list than member 0");
        if (s->n_maps > 1)
            return bb::fail(BB_ERR_INVALID, "bb_group_create: member " + std::to_string(r) +
                                                " is a solver of several maps");
    }
    bb_group *g = new (std::nothrow) bb_group();
    if (!g) return bb::fail(BB_ERR_NOMEM, "bb_group_create: out of host memory");
    g->m.assign(members, members + n);
    for (bb_solver *s : g->m) g->exch.push_back(s->d_exch);
    g->d_src.resize((size_t)n);
    g->d_mask.resize((size_t)n);
    g->ready.resize((size_t)n);
    g->applied.resize((size_t)n);
    g->rc.assign((size_t)n, BB_OK);
    g->err.assign((size_t)n, std::string());
    g->bar.n = n;
    const int rc = group_setup(g);
    if (rc != BB_OK) return failed_create(rc, [&] { group_free(g); });
    *out = g;
    return BB_OK;
}

int bb_group_iterate(bb_group *g, int64_t iters, double lr) {
    BB_REQUIRE(g != nullptr, "bb_group_iterate: group is NULL");
    for (size_t r = 0; r < g->m.size(); ++r) {
        bb_solver *s = g->m[r];
        BB_TRY(check_iterate(s, iters, "bb_group_iterate"));
        if (s->grad_pending)
            return bb::fail(BB_ERR_STATE, "bb_group_iterate: member " + std::to_string(r) +
                                              " has a bb_solver_grad pending");
        if (s->d_exch != g->exch[r])
            return bb::fail(BB_ERR_STATE, "bb_group_iterate: member " + std::to_string(r) +
                                              " changed its exchange buffer after bb_group_create");
    }
    if (iters == 0) return BB_OK;
    std::unique_lock<std::mutex> lk(g->mu);
    g->iters = iters;
    g->lr = lr;
    g->done = 0;
    std::fill(g->rc.begin(), g->rc.end(), BB_OK);
    ++g->job;
    g->cv_job.notify_all();
    g->cv_done.wait(lk, [&] { return g->done == (int)g->m.size(); });
    for (size_t r = 0; r < g->m.size(); ++r)
        if (g->rc[r] > 0)
            return bb::fail(g->rc[r], "bb_group_iterate: member " + std::to_string(r) + ": " + g->err[r]);
    return BB_OK;
}

int bb_group_destroy(bb_group *g) {
    if (!g) return BB_OK;
    group_free(g);
    return BB_OK;
}

}  // extern "C"
