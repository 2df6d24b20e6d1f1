"""CPU: who ends a communicator, and how (blueberry_amd/csrc/bb_comm_cache.h), compiled on its
own with the host C++ compiler and driven as a stand-alone program.  The fake communicators are
distinct heap cells that the fake destroy and abort free, so under AddressSanitizer a double end
is a report and so is a leak; counters record every call.  The rules are the library's: a
suspect communicator is evicted and aborted (leaked where there is no abort), a stale entry is
replaced and destroyed, an entry in use is never handed out or cleared.  A second build of the
same driver runs its threaded part under ThreadSanitizer."""
import os
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DRIVER = r"""
#include <stdio.h>
#include <string.h>
#include <atomic>
#include <random>
#include <thread>
#include <vector>
#include "bb_comm_cache.h"

static std::atomic<int> g_made{0}, g_destroyed{0}, g_aborted{0};
static void *make_comm() { ++g_made; return new int(0); }
static int fake_destroy(void *c) { ++g_destroyed; delete (int *)c; return 0; }
static int fake_abort(void *c) { ++g_aborted; delete (int *)c; return 5; }
static void hand_back(void *c) { delete (int *)c; }   // a leaked cell: the driver's to free

static int g_failed = 0;
#define CHECK(cond) \
    do { if (!(cond)) { printf("line %d: %s\n", __LINE__, #cond); g_failed = 1; } } while (0)

struct Id { unsigned char b[bb::kCommIdBytes]; };
static Id make_id(unsigned seed) {
    Id id;
    for (size_t i = 0; i < sizeof(id.b); ++i) id.b[i] = (unsigned char)(seed * 31u + i * 7u);
    return id;
}
static void counts(int *d, int *a) { *d = g_destroyed.load(), *a = g_aborted.load(); }
static bool peek(bb::CommCache &cc, int dev, int rank, int world, uint64_t *gen = nullptr) {
    bool avail = false;
    uint64_t g = 0;
    cc.peek(dev, rank, world, &avail, &g);
    if (gen) *gen = g;
    CHECK(avail || g == 0);
    return avail;
}

static void rules() {
    const Id id1 = make_id(1), id2 = make_id(2);
    int d0, a0, d, a;
    {   // adopt, end of lease: free, nothing destroyed; a second lease attaches to the same
        bb::CommCache cc(fake_destroy, fake_abort);
        counts(&d0, &a0);
        void *c = make_comm();
        uint64_t gen = 0;
        {
            bb::CommLease l = cc.adopt(0, 1, 2, c, &id1);
            CHECK(l && l.cached() && l.comm() == c);
            CHECK(!peek(cc, 0, 1, 2));                    // in use: not available
            CHECK(!cc.attach(0, 1, 2));                   // ... and never handed out
        }
        counts(&d, &a);
        CHECK(d == d0 && a == a0);
        CHECK(peek(cc, 0, 1, 2, &gen) && gen == bb::comm_generation_of(&id1));
        CHECK(!peek(cc, 1, 1, 2) && !cc.attach(1, 1, 2)); // another key: nothing there
        {
            bb::CommLease l2 = cc.attach(0, 1, 2);
            CHECK(l2 && l2.cached() && l2.comm() == c);
            CHECK(!peek(cc, 0, 1, 2));
        }
        uint64_t gen2 = 0;
        CHECK(peek(cc, 0, 1, 2, &gen2) && gen2 == gen);
        cc.clear();
        counts(&d, &a);
        CHECK(d == d0 + 1 && a == a0 && !peek(cc, 0, 1, 2));
    }
    {   // adopt while the key is held: a private lease, destroyed once at its end
        bb::CommCache cc(fake_destroy, fake_abort);
        void *c1 = make_comm(), *c2 = make_comm();
        bb::CommLease holder = cc.adopt(0, 0, 2, c1, &id1);
        counts(&d0, &a0);
        {
            bb::CommLease own = cc.adopt(0, 0, 2, c2, &id2);
            CHECK(own && !own.cached() && own.comm() == c2);
            CHECK(!own.detach() && own.comm() == c2);    // refused: the lease's own
        }
        counts(&d, &a);
        CHECK(d == d0 + 1 && a == a0);
        CHECK(holder.cached() && holder.comm() == c1 && !peek(cc, 0, 0, 2));
        CHECK(holder.detach() && !holder);                // a cached one: free again
        uint64_t gen = 0;
        CHECK(peek(cc, 0, 0, 2, &gen) && gen == bb::comm_generation_of(&id1));
        counts(&d, &a);
        CHECK(d == d0 + 1 && a == a0);
        cc.clear();
    }
    {   // adopt over a free entry with another communicator: the old one destroyed once
        bb::CommCache cc(fake_destroy, fake_abort);
        void *c1 = make_comm(), *c2 = make_comm();
        { bb::CommLease l = cc.adopt(0, 0, 2, c1, &id1); }
        counts(&d0, &a0);
        bb::CommLease l = cc.adopt(0, 0, 2, c2, &id2);
        counts(&d, &a);
        CHECK(d == d0 + 1 && a == a0 && l.cached() && l.comm() == c2);
        CHECK(l.end() == nullptr);
        uint64_t gen = 0;
        CHECK(peek(cc, 0, 0, 2, &gen) && gen == bb::comm_generation_of(&id2));
        cc.clear();
    }
    {   // suspect and cached: evicted, aborted once
        bb::CommCache cc(fake_destroy, fake_abort);
        bb::CommLease l = cc.adopt(0, 0, 2, make_comm(), &id1);
        counts(&d0, &a0);
        l.mark_suspect();
        CHECK(l.end() == nullptr && !l);
        counts(&d, &a);
        CHECK(d == d0 && a == a0 + 1 && !peek(cc, 0, 0, 2) && !cc.attach(0, 0, 2));
        cc.clear();
        counts(&d, &a);
        CHECK(d == d0 && a == a0 + 1);
    }
    {   // suspect, no abort: evicted, neither call made, the cell comes back
        bb::CommCache cc(fake_destroy, nullptr);
        void *c = make_comm();
        bb::CommLease l = cc.adopt(0, 0, 2, c, &id1);
        counts(&d0, &a0);
        l.mark_suspect();
        void *leaked = l.end();
        counts(&d, &a);
        CHECK(leaked == c && !l && d == d0 && a == a0 && !peek(cc, 0, 0, 2));
        hand_back(leaked);
    }
    {   // suspect while the entry meanwhile holds another communicator: that entry stays
        bb::CommCache cc(fake_destroy, fake_abort);
        void *c1 = make_comm(), *c2 = make_comm();
        bb::CommLease l1 = cc.adopt(0, 0, 2, c1, &id1);
        bb::CommLease moved = std::move(l1);              // the lease moves; the entry is c1's
        CHECK(moved.detach());
        bb::CommLease l2 = cc.adopt(0, 0, 2, c2, &id2);   // replaces (and destroys) c1 ...
        bb::CommLease stale = cc.adopt(0, 0, 2, make_comm(), &id1);   // ... held: private
        stale.mark_suspect();
        counts(&d0, &a0);
        CHECK(stale.end() == nullptr);
        counts(&d, &a);
        CHECK(d == d0 && a == a0 + 1);
        CHECK(l2.cached() && l2.comm() == c2 && !peek(cc, 0, 0, 2));
        CHECK(l2.end() == nullptr);
        uint64_t gen = 0;
        CHECK(peek(cc, 0, 0, 2, &gen) && gen == bb::comm_generation_of(&id2));
        cc.clear();
    }
    {   // after an abort the key is cached anew; a suspect lease of another key leaves it alone
        bb::CommCache cc(fake_destroy, fake_abort);
        void *c1 = make_comm(), *c2 = make_comm();
        bb::CommLease l1 = cc.adopt(0, 0, 2, c1, &id1);
        bb::CommLease keep = cc.adopt(0, 1, 2, make_comm(), &id1);
        int rc = -1;
        CHECK(l1.abort(&rc) == nullptr && rc == 5 && !l1);
        bb::CommLease l2 = cc.adopt(0, 0, 2, c2, &id2);
        keep.mark_suspect();
        CHECK(keep.end() == nullptr);
        CHECK(l2.cached() && l2.comm() == c2 && !peek(cc, 0, 1, 2));
        CHECK(l2.end() == nullptr && peek(cc, 0, 0, 2));
        cc.clear();
    }
    {   // abort, with and without an abort function
        bb::CommCache with(fake_destroy, fake_abort), without(fake_destroy, nullptr);
        bb::CommLease l = with.adopt(0, 0, 2, make_comm(), &id1);
        counts(&d0, &a0);
        int rc = -1;
        CHECK(l.abort(&rc) == nullptr && rc == 5 && !l && !l.cached());
        counts(&d, &a);
        CHECK(d == d0 && a == a0 + 1 && !peek(with, 0, 0, 2));
        CHECK(l.end() == nullptr);                        // empty: ends nothing
        void *c = make_comm();
        bb::CommLease m = without.adopt(0, 0, 2, c, &id1);
        rc = -1;
        void *leaked = m.abort(&rc);
        counts(&d, &a);
        CHECK(leaked == c && rc == -1 && !m && d == d0 && a == a0 + 1 && !peek(without, 0, 0, 2));
        hand_back(leaked);
        bb::CommLease none;                               // no communicator: nothing to abort
        CHECK(none.abort(&rc) == nullptr && rc == -1 && none.detach());
    }
    {   // clear with one entry in use and two free: two destroys, the held one survives
        bb::CommCache cc(fake_destroy, fake_abort);
        void *c0 = make_comm();
        bb::CommLease held = cc.adopt(0, 0, 3, c0, &id1);
        { bb::CommLease l = cc.adopt(0, 1, 3, make_comm(), &id1); }
        { bb::CommLease l = cc.adopt(0, 2, 3, make_comm(), &id1); }
        counts(&d0, &a0);
        cc.clear();
        counts(&d, &a);
        CHECK(d == d0 + 2 && a == a0 && !peek(cc, 0, 1, 3) && !peek(cc, 0, 2, 3));
        CHECK(held.cached() && held.comm() == c0);
        CHECK(held.end() == nullptr && peek(cc, 0, 0, 3));   // ... and still goes back afterwards
        counts(&d, &a);
        CHECK(d == d0 + 2);
        cc.clear();
        counts(&d, &a);
        CHECK(d == d0 + 3);
    }
    {   // generations: two ids differ, never 0, one id always the same
        Id zero;
        memset(zero.b, 0, sizeof(zero.b));
        CHECK(bb::comm_generation_of(&id1) != bb::comm_generation_of(&id2));
        CHECK(bb::comm_generation_of(&id1) == bb::comm_generation_of(&id1));
        for (unsigned k = 0; k < 1000; ++k) {
            const Id a1 = make_id(k), a2 = make_id(k);
            CHECK(bb::comm_generation_of(&a1) != 0);
            CHECK(bb::comm_generation_of(&a1) == bb::comm_generation_of(&a2));
        }
        CHECK(bb::comm_generation_of(&zero) != 0);
    }
    {   // a moved-from lease ends nothing
        bb::CommCache cc(fake_destroy, fake_abort);
        void *c = make_comm();
        counts(&d0, &a0);
        {
            bb::CommLease a1 = cc.adopt(0, 0, 2, c, &id1);
            bb::CommLease b1(std::move(a1));
            CHECK(!a1 && !a1.cached() && a1.end() == nullptr);
            CHECK(b1 && b1.cached() && b1.comm() == c && !peek(cc, 0, 0, 2));
            bb::CommLease c1;
            c1 = std::move(b1);
            CHECK(!b1 && c1.comm() == c);
            // a private one too: moved, it is destroyed once, by the lease that has it
            bb::CommLease p = cc.adopt(0, 0, 2, make_comm(), &id2);
            bb::CommLease q(std::move(p));
            CHECK(!p && q && !q.cached());
        }
        counts(&d, &a);
        CHECK(d == d0 + 1 && a == a0 && peek(cc, 0, 0, 2));
        cc.clear();
    }
    CHECK(g_made.load() == g_destroyed.load() + g_aborted.load() + 2);   // + the two handed back
}

// 8 threads adopt, attach, detach and clear over 3 keys.  Every cell ends exactly once: freed
// twice or never, a sanitizer says so; the counters say it too.
static void threads() {
    bb::CommCache cc(fake_destroy, fake_abort);
    const int made0 = g_made.load(), ended0 = g_destroyed.load() + g_aborted.load();
    std::vector<std::thread> th;
    for (int t = 0; t < 8; ++t)
        th.emplace_back([&cc, t] {
            std::mt19937 rng(100 + t);
            for (int round = 0; round < 2000; ++round) {
                const int key = (int)(rng() % 3);
                const Id id = make_id(rng());
                switch (rng() % 6) {
                case 0: {
                    bb::CommLease l = cc.adopt(0, key, 3, make_comm(), &id);
                    if (rng() % 8 == 0) l.mark_suspect();
                    break;
                }
                case 1: {
                    bb::CommLease l = cc.attach(0, key, 3);
                    if (l && !l.detach()) { printf("a cached lease refused detach\n"); g_failed = 1; }
                    break;
                }
                case 2: {
                    bb::CommLease l = cc.adopt(0, key, 3, make_comm(), &id);
                    bb::CommLease m = cc.attach(0, key, 3);     // held (by l or another): empty,
                    if (m && m.comm() == l.comm()) {            // or another solver's, never l's
                        printf("an entry in use was handed out\n");
                        g_failed = 1;
                    }
                    int rc = 0;
                    if (rng() % 4 == 0 && l.abort(&rc) != nullptr) g_failed = 1;
                    break;
                }
                case 3: {
                    bool avail = false;
                    uint64_t gen = 0;
                    cc.peek(0, key, 3, &avail, &gen);
                    if (avail != (gen != 0)) { printf("peek: available without generation\n"); g_failed = 1; }
                    break;
                }
                case 4: cc.clear(); break;
                default: {
                    bb::CommLease l = cc.attach(0, key, 3);
                    bb::CommLease m(std::move(l));
                    break;
                }
                }
            }
        });
    for (auto &x : th) x.join();
    cc.clear();
    const int made = g_made.load() - made0, ended = g_destroyed.load() + g_aborted.load() - ended0;
    if (made != ended) { printf("threads: %d made, %d ended\n", made, ended); g_failed = 1; }
    for (int key = 0; key < 3; ++key)
        if (peek(cc, 0, key, 3)) { printf("threads: key %d left in the cache\n", key); g_failed = 1; }
}

int main(int argc, char **argv) {
    const bool only_threads = argc > 1 && strcmp(argv[1], "threads") == 0;
    if (!only_threads) rules();
    threads();
    if (g_failed) return 1;
    printf("ok %d communicators\n", g_made.load());
    return 0;
}
"""


def _build_and_run(sanitize, args):
    cxx = shutil.which("c++") or shutil.which("g++")
    if cxx is None:
        pytest.fail("no host C++ compiler (c++ / g++) to build the communicator-cache driver")
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "driver.cpp"), os.path.join(tmp, "driver")
        with open(src, "w") as f:
            f.write(DRIVER)
        subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-pthread", "-fsanitize=" + sanitize,
                        "-fno-sanitize-recover=all",
                        "-I", os.path.join(ROOT, "blueberry_amd", "csrc"), src, "-o", exe],
                       check=True, timeout=180)
        r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().startswith("ok"), r.stdout + r.stderr
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr


def test_comm_cache_rules_under_asan_ubsan():
    _build_and_run("address,undefined", [])


def test_comm_cache_threads_under_tsan():
    _build_and_run("thread", ["threads"])
