// bb_comm_cache.h -- who ends a communicator, and how: the process-wide cache of the library's
// RCCL communicators and the lease a solver holds on one.  Plain C++17 (no HIP, no RCCL): a
// communicator is a void *, and the two calls that end one -- destroy, and abort, which may be
// missing -- are function pointers.  bb_comm.cpp passes RCCL's (bb::comm_cache());
// tests/test_comm_cache_cpu.py passes counters and drives every rule on the host.
//
// The library's communicators outlive the solvers that use them: ncclCommInitRank costs
// 0.1-1 s and every multi-rank fit() used to pay it.  One communicator per (device, rank,
// world) is kept for the life of the process; a solver borrows it (attach) and gives it back
// when its lease ends.  While one solver holds it, another one gets a communicator of its own
// (a communicator must not serve two streams at once).
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <map>
#include <mutex>
#include <tuple>
#include <utility>

namespace bb {

constexpr size_t kCommIdBytes = 128;   // NCCL_UNIQUE_ID_BYTES

// Which ncclCommInitRank made a communicator: a hash of the 128-byte unique id, the same on
// every rank of that call and on no other.  The key (device, rank, world) alone cannot tell two
// communicators of different jobs -- or of different generations of one job -- apart; the
// ranks compare this before anybody attaches (bb_comm_cached_generation, solver.comm_reuse).
inline uint64_t comm_generation_of(const void *unique_id) {
    uint64_t h = 1469598103934665603ull;             // FNV-1a over the id
    const unsigned char *b = (const unsigned char *)unique_id;
    for (size_t i = 0; i < kCommIdBytes; ++i) h = (h ^ b[i]) * 1099511628211ull;
    return h ? h : 1;                                // 0 = "none"
}

class CommLease;

class CommCache {
public:
    typedef int (*EndFn)(void *);
    typedef std::tuple<int, int, int> Key;   // (device, rank, world)
    explicit CommCache(EndFn destroy, EndFn abort = nullptr) : destroy_(destroy), abort_(abort) {}
    CommCache(const CommCache &) = delete;
    CommCache &operator=(const CommCache &) = delete;

    // After ncclCommInitRank succeeded: into the cache as in use, unless another solver holds
    // this key's entry right now -- then the lease owns the communicator privately.  A free
    // entry holding another communicator is a stale one: replaced, and the old one destroyed.
    inline CommLease adopt(int device, int rank, int world, void *comm, const void *unique_id);
    // The key's communicator, if its entry holds one and is free; else an empty lease.
    inline CommLease attach(int device, int rank, int world);
    // (available, generation) of a free entry that holds a communicator, else (false, 0).
    void peek(int device, int rank, int world, bool *available, uint64_t *generation) {
        std::lock_guard<std::mutex> lock(mu_);
        const Entry *e = free_entry(Key(device, rank, world));
        *available = e != nullptr;
        *generation = e ? e->generation : 0;
    }
    // Destroys the communicators of the free entries; the ones in use stay.
    void clear() {
        std::lock_guard<std::mutex> lock(mu_);
        for (auto it = entries_.begin(); it != entries_.end();) {
            if (it->second.in_use) { ++it; continue; }
            if (it->second.comm && destroy_) destroy_(it->second.comm);
            it = entries_.erase(it);
        }
    }

private:
    friend class CommLease;
    struct Entry {
        void *comm = nullptr;
        bool in_use = false;
        uint64_t generation = 0;
    };
    // The entry of `key` if it is there, holds a communicator and is free.  The caller holds mu_.
    Entry *free_entry(const Key &key) {
        auto it = entries_.find(key);
        return it != entries_.end() && it->second.comm && !it->second.in_use ? &it->second : nullptr;
    }
    // A lease on `comm` ends: its entry -- only while it still holds this communicator -- goes
    // (evict: a suspect or aborted communicator is not handed out again) or becomes free.
    void give_back(const Key &key, void *comm, bool evict) {
        std::lock_guard<std::mutex> lock(mu_);
        auto it = entries_.find(key);
        if (it == entries_.end() || it->second.comm != comm) return;
        if (evict) entries_.erase(it);
        else it->second.in_use = false;
    }
    const EndFn destroy_, abort_;
    std::mutex mu_;
    std::map<Key, Entry> entries_;
};

// What a solver holds in place of a communicator: the pointer, whether it is the cache's or the
// solver's own, and whether a collective on it failed to enqueue.  Move-only; the end of the
// lease (end(), the destructor) is THE place a solver's communicator ends.
class CommLease {
public:
    CommLease() = default;
    CommLease(CommLease &&o) noexcept { *this = std::move(o); }
    CommLease &operator=(CommLease &&o) noexcept {
        if (this != &o) {
            end();
            cache_ = o.cache_, key_ = o.key_, comm_ = o.comm_, cached_ = o.cached_, suspect_ = o.suspect_;
            o.comm_ = nullptr, o.cached_ = o.suspect_ = false;
        }
        return *this;
    }
    ~CommLease() { end(); }

    explicit operator bool() const { return comm_ != nullptr; }
    void *comm() const { return comm_; }
    bool cached() const { return comm_ && cached_; }
    // A collective on it failed to enqueue: its peers may now sit in a collective this rank
    // left.  Never handed out again.
    void mark_suspect() { suspect_ = true; }

    // A cached communicator back to the cache, free again.  false, and nothing done: the
    // communicator is the lease's own.  (An empty lease: true.)
    bool detach() {
        if (comm_ && !cached_) return false;
        end();
        return true;
    }
    // The end of the lease.  A suspect communicator leaves the cache and is aborted -- where
    // there is no abort it is leaked (destroy would wait for its outstanding work, perhaps for
    // ever) and returned, for whoever can still do something with it; otherwise a cached one
    // goes back free and a private one is destroyed.  Returns the leaked communicator, else null.
    void *end() {
        void *c = comm_, *leaked = nullptr;
        if (!c) return nullptr;
        if (cached_) cache_->give_back(key_, c, suspect_);
        if (suspect_) {
            if (cache_->abort_) cache_->abort_(c);
            else leaked = c;
        } else if (!cached_ && cache_->destroy_) {
            cache_->destroy_(c);
        }
        comm_ = nullptr, cached_ = suspect_ = false;
        return leaked;
    }
    // Out of the cache and aborted: *rc is what abort returned.  Without an abort the
    // communicator is leaked and returned (else null), *rc untouched.  The lease is empty after.
    void *abort(int *rc) {
        void *c = comm_, *leaked = nullptr;
        if (!c) return nullptr;
        if (cached_) cache_->give_back(key_, c, /*evict=*/true);
        comm_ = nullptr, cached_ = suspect_ = false;
        if (cache_->abort_) *rc = cache_->abort_(c);
        else leaked = c;
        return leaked;
    }

private:
    friend class CommCache;
    CommCache *cache_ = nullptr;
    CommCache::Key key_;
    void *comm_ = nullptr;
    bool cached_ = false, suspect_ = false;
};

inline CommLease CommCache::adopt(int device, int rank, int world, void *comm, const void *unique_id) {
    CommLease l;
    l.cache_ = this, l.key_ = Key(device, rank, world), l.comm_ = comm;
    std::lock_guard<std::mutex> lock(mu_);
    Entry &e = entries_[l.key_];
    if (!e.in_use) {
        if (e.comm && e.comm != comm && destroy_) destroy_(e.comm);   // a stale one: replaced
        e.comm = comm;
        e.in_use = true;
        e.generation = comm_generation_of(unique_id);
        l.cached_ = true;
    }
    return l;
}

inline CommLease CommCache::attach(int device, int rank, int world) {
    CommLease l;
    std::lock_guard<std::mutex> lock(mu_);
    if (Entry *e = free_entry(Key(device, rank, world))) {
        e->in_use = true;
        l.cache_ = this, l.key_ = Key(device, rank, world), l.comm_ = e->comm, l.cached_ = true;
    }
    return l;
}

}  // namespace bb
