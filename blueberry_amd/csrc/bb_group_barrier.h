// bb_group_barrier.h -- the host-side synchronisation of a group of solvers (bb_group_*):
// a reusable barrier of n threads and the two-barrier loop every member thread runs.  Plain
// C++17 (no HIP), so that tests/test_group_barrier_cpu.py can drive it on the host with
// injected failures.
#pragma once

#include <stdint.h>

#include <condition_variable>
#include <mutex>

namespace bb {

// A reusable barrier of n host threads (C++17 has no std::barrier).  Every thread arrives with
// its own outcome; all of them leave a phase with "every thread arrived with success".  The
// releasing thread stores that verdict once per phase and the waiters return the stored value:
// it cannot change before each of them has read it, since the next phase is not released
// without them.  (Reading a sticky flag after waking instead would let a waiter of phase p see a
// failure of phase p + 1 and leave while the others wait at p + 1 for it.)
struct GroupBarrier {
    std::mutex mu;
    std::condition_variable cv;
    int n = 0, arrived = 0;
    uint64_t phase = 0;
    bool failed_now = false;    // a thread of the current phase arrived with a failure
    bool released_ok = true;    // the verdict of the last released phase
    bool arrive(bool ok) {
        std::unique_lock<std::mutex> lk(mu);
        if (!ok) failed_now = true;
        if (++arrived == n) {
            arrived = 0;
            released_ok = !failed_now;
            failed_now = false;
            ++phase;
            cv.notify_all();
            return released_ok;
        }
        const uint64_t p = phase;
        cv.wait(lk, [&] { return phase != p; });
        return released_ok;
    }
};

// One member's share of `iters` iterations: grad(k), barrier, apply(k), barrier.  `rc` is the
// outcome of the member's set-up (0 = success); a member that fails -- there or at any step --
// arrives with the failure and EVERY member leaves at that same barrier: the failing one with
// its code, the others with `aborted`.  Nobody is left waiting at a later one.
template <typename Grad, typename Apply>
int group_steps(GroupBarrier &bar, int64_t iters, int rc, int aborted, Grad grad, Apply apply) {
    for (int64_t k = 0; k < iters; ++k) {
        if (rc == 0) rc = grad(k);
        if (!bar.arrive(rc == 0)) return rc != 0 ? rc : aborted;
        rc = apply(k);
        if (!bar.arrive(rc == 0)) return rc != 0 ? rc : aborted;
    }
    return rc;
}

}  // namespace bb
