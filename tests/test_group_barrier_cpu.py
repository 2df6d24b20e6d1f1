"""CPU: the host barrier of a group (blueberry_amd/csrc/bb_group_barrier.h), compiled on its own
with the host C++ compiler and driven by threads that stand in for the members: one of them
fails at a random step (its "enqueue" returns an error), and every thread must leave -- the
failing one with its code, the others as aborted -- with nobody left waiting at a later
barrier.  A hang is caught by a watchdog inside the driver and by the subprocess time limit."""
import os
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DRIVER = r"""
#include <stdio.h>
#include <stdlib.h>
#include <unistd.h>
#include <atomic>
#include <chrono>
#include <random>
#include <thread>
#include <vector>
#include "bb_group_barrier.h"

int main() {
    std::atomic<int> finished{0};
    const int trials = 3000;
    std::thread([&] {                  // watchdog: a trial that hangs ends the process
        int last = -1;
        for (;;) {
            std::this_thread::sleep_for(std::chrono::seconds(5));
            const int now = finished.load();
            if (now == trials) return;
            if (now == last) { printf("HANG in trial %d\n", now); fflush(stdout); _exit(2); }
            last = now;
        }
    }).detach();
    std::mt19937 rng(7);
    for (int t = 0; t < trials; ++t) {
        const int n = 2 + (int)(rng() % 7);                     // 2..8 members
        const int64_t iters = 1 + (int64_t)(rng() % 4);
        // the failing member and the call it fails at (setup, a grad or an apply); -1: none
        const int bad = (int)(rng() % (n + 1)) - 1;
        const int bad_at = (int)(rng() % (2 * iters + 1)) - 1;  // -1 = at set-up
        bb::GroupBarrier bar;
        bar.n = n;
        std::vector<int> rc((size_t)n, 12345);
        std::vector<std::thread> th;
        for (int r = 0; r < n; ++r)
            th.emplace_back([&, r] {
                auto fail = [&](int call) { return r == bad && call == bad_at ? 7 : 0; };
                rc[(size_t)r] = bb::group_steps(
                    bar, iters, fail(-1), -1, [&](int64_t k) { return fail((int)(2 * k)); },
                    [&](int64_t k) { return fail((int)(2 * k + 1)); });
            });
        for (auto &x : th) x.join();
        for (int r = 0; r < n; ++r) {
            const int want = bad < 0 ? 0 : (r == bad ? 7 : -1);
            if (rc[(size_t)r] != want) {
                printf("trial %d: member %d of %d returned %d, expected %d\n", t, r, n,
                       rc[(size_t)r], want);
                return 1;
            }
        }
        finished.store(t + 1);
    }
    printf("ok %d trials\n", trials);
    return 0;
}
"""


def test_group_barrier_leaves_nobody_waiting():
    cxx = shutil.which("c++") or shutil.which("g++")
    if cxx is None:
        pytest.fail("no host C++ compiler (c++ / g++) to build the barrier driver")
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "driver.cpp"), os.path.join(tmp, "driver")
        with open(src, "w") as f:
            f.write(DRIVER)
        subprocess.run([cxx, "-std=c++17", "-O1", "-pthread",
                        "-I", os.path.join(ROOT, "blueberry_amd", "csrc"), src, "-o", exe],
                       check=True, timeout=180)
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().startswith("ok"), r.stdout + r.stderr
