// bb_common.h -- internal helpers shared by the translation units of
// libblueberry_hip.so (error state, HIP status checks, layout arithmetic).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <map>
#include <mutex>
#include <string>
#include <tuple>
#include <utility>

#include "blueberry_hip.h"

namespace bb {

// Thread-local last-error message behind bb_last_error().
void set_error(const std::string &msg);
int fail(int code, const std::string &msg);

// The status of a HIP call as the library's return code: BB_OK, or `code` with "<who>: <HIP's
// text>" as the last error.  An allocation stage passes BB_ERR_NOMEM whatever HIP said.
inline int hip_status(const char *who, hipError_t e, int code = BB_ERR_HIP) {
    return e == hipSuccess ? (int)BB_OK : fail(code, std::string(who) + ": " + hipGetErrorString(e));
}

#define BB_HIP_CHECK(expr)                                                              \
    do {                                                                                \
        hipError_t _e = (expr);                                                         \
        if (_e != hipSuccess)                                                           \
            return ::bb::fail(BB_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e)); \
    } while (0)

#define BB_TRY(expr)                  \
    do {                              \
        int _rc = (expr);             \
        if (_rc != BB_OK) return _rc; \
    } while (0)

#define BB_REQUIRE(cond, msg)                                   \
    do {                                                        \
        if (!(cond)) return ::bb::fail(BB_ERR_INVALID, (msg));  \
    } while (0)

// ---- layout constants (docs/SPEC.md 3) -----------------------------------
// A unit is always 8 KiB = 8 wave-loads of 64 lanes x 16 B.
//   fp32: 4 matrix rows x 512 columns (2 loads per row)
//   fp64: 2 rows x 512 columns (4 loads per row) above kF64WideFrom bins, where the
//         sweep is what matters; 8 rows x 128 columns (1 load per row) up to it,
//         where small column partials and many blocks matter (launch-bound regime).
// Crossover measured on MI355X: N=2,500 is 24 us per iteration narrow / 30 wide,
// N=6,000 is 64 narrow / 52 wide.
constexpr int kUnitBytes = 8192;
constexpr int64_t kF64WideFrom = 4096;
// Up to this many bins a one-rank solver iterates on the row-owner path (both
// triangles resident, one wave per bin, one launch per iteration: DESIGN.md 4.10).
constexpr int64_t kRowOwnerMaxBins = 4096;

inline int64_t elem_size(int dtype) { return dtype == BB_F64 ? 8 : 4; }
inline bool wide_layout(int dtype, int64_t n_bins) { return dtype != BB_F64 || n_bins > kF64WideFrom; }
inline int64_t tile_width(int dtype, int64_t n_bins) { return wide_layout(dtype, n_bins) ? 512 : 128; }
inline int64_t rows_per_unit(int dtype, int64_t n_bins) {
    return dtype != BB_F64 ? 4 : (wide_layout(dtype, n_bins) ? 2 : 8);
}
inline int64_t round_up(int64_t a, int64_t b) { return (a + b - 1) / b * b; }
// the next 256-byte boundary: where a part of a device buffer cut into several starts
constexpr size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

// Select the device, failing loudly when there is none.
int use_device(int device);
// Entry of every call on an existing handle: select its device.  Nothing else: the
// thread's sticky "last error" is left alone (see launch() below).
int enter_device(int device);

// Non-blocking streams are handed out from a small per-device pool: creating one costs
// 1.3-3 ms and destroying one 1.6 ms on this platform (tools/api_cost_probe.py) -- together
// two thirds of a whole chr21-sized fit.  acquire gives an idle stream of the CURRENT
// device (a pooled one, or a new one); release synchronises it and keeps up to
// kPooledStreams per device for the next handle.
hipError_t acquire_stream(int device, hipStream_t *out);
void release_stream(int device, hipStream_t stream);

// Kernel launch that hands back the launch's OWN status (hipLaunchKernel returns it).
// The library never reads hipGetLastError(): that word is per-thread, sticky, and shared
// with every other HIP user of the calling thread (torch, RCCL), so a launch check made
// through it can report somebody else's old failure -- or, if it is cleared first, hide
// one.  Every HIP call here is checked by its own return value instead; the few probes
// that are allowed to fail (an attribute an older runtime lacks, a memory flavour the
// device does not offer) consume their error on the spot with hipGetLastError().
template <typename... P, size_t... I>
inline hipError_t launch_impl(void (*kernel)(P...), dim3 grid, dim3 block, size_t lds,
                              hipStream_t stream, std::tuple<P...> &vals,
                              std::index_sequence<I...>) {
    void *ptrs[sizeof...(P) ? sizeof...(P) : 1] = {(void *)&std::get<I>(vals)...};
    return hipLaunchKernel((const void *)kernel, grid, block, ptrs, lds, stream);
}
template <typename... P, typename... A>
inline hipError_t launch(void (*kernel)(P...), dim3 grid, dim3 block, size_t lds,
                         hipStream_t stream, A &&...args) {
    static_assert(sizeof...(P) == sizeof...(A), "kernel argument count");
    std::tuple<P...> vals{static_cast<P>(std::forward<A>(args))...};
    return launch_impl(kernel, grid, block, lds, stream, vals, std::index_sequence_for<P...>{});
}

// THE owner of a device allocation: what it holds is freed when it is reset, re-allocated,
// assigned over or destroyed, and by nobody else.  A handle keeps its buffers as members of
// this type, a host-staged entry point as locals; a plain pointer into one is a view.  Movable,
// not copyable.  alloc() frees what is there and allocates anew (at least one byte); reserve()
// is the grow-only form a scratch arena uses: it keeps what is there when that is large enough
// (else the contents are lost).  A failed allocation leaves the buffer empty and consumes the
// failed hipMalloc's error on the spot (see launch() above).  adopt() takes over memory made
// elsewhere that hipFree releases (hipExtMallocWithFlags).
struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept { *this = std::move(o); }
    DevBuf &operator=(DevBuf &&o) noexcept {   // (what this held goes with o)
        std::swap(p, o.p);
        std::swap(bytes, o.bytes);
        return *this;
    }
    ~DevBuf() { reset(); }
    explicit operator bool() const { return p != nullptr; }
    template <class T>
    T *as() const { return (T *)p; }
    void reset() {
        if (p) (void)hipFree(p);
        p = nullptr, bytes = 0;
    }
    void adopt(void *mem, size_t n = 0) {
        reset();
        p = mem, bytes = n;
    }
    hipError_t alloc(size_t n) {
        reset();
        const hipError_t e = hipMalloc(&p, n ? n : 1);
        if (e == hipSuccess) {
            bytes = n;
        } else {
            p = nullptr;
            (void)hipGetLastError();
        }
        return e;
    }
    hipError_t reserve(size_t need) { return need <= bytes ? hipSuccess : alloc(need); }
};
// b.alloc(bytes) as the library's status: BB_ERR_NOMEM with "hipMalloc failed: <HIP's text>".
inline int alloc_status(DevBuf &b, size_t bytes) {
    return hip_status("hipMalloc failed", b.alloc(bytes), BB_ERR_NOMEM);
}

// The owner of a HIP event, as DevBuf is of memory: movable, not copyable, empty or valid.
struct Event {
    hipEvent_t e = nullptr;
    Event() = default;
    Event(const Event &) = delete;
    Event &operator=(const Event &) = delete;
    Event(Event &&o) noexcept { std::swap(e, o.e); }
    Event &operator=(Event &&o) noexcept {   // (what this held goes with o)
        std::swap(e, o.e);
        return *this;
    }
    ~Event() { reset(); }
    operator hipEvent_t() const { return e; }
    void reset() {
        if (e) (void)hipEventDestroy(e);
        e = nullptr;
    }
    hipError_t create(unsigned flags = hipEventDefault) {
        reset();
        return hipEventCreateWithFlags(&e, flags);   // (writes e on success only)
    }
};

// The clock of a call's stages: K events, stage k being what a stream does between mark(k) and
// mark(k + 1).  start(false) leaves it off: no event is made, a mark does nothing and every stage
// reads 0, so a call writes its marks once, timed or not.  A stage whose end was never marked -- one
// the call skipped -- reads 0 too.  It never synchronises: read after the caller's own wait.
template <int K>
struct StageClock {
    Event ev[K];
    bool marked[K] = {};
    bool on = false;
    hipError_t start(bool want = true) {
        hipError_t e = hipSuccess;
        for (int k = 0; k < K && want && e == hipSuccess; ++k) e = ev[k].create();
        on = want && e == hipSuccess;
        return e;
    }
    hipError_t mark(int k, hipStream_t stream) {
        if (!on) return hipSuccess;
        marked[k] = true;
        return hipEventRecord(ev[k], stream);
    }
    hipError_t read(int k, double *ms) const {
        float t = 0.f;
        const hipError_t e =
            on && marked[k] && marked[k + 1] ? hipEventElapsedTime(&t, ev[k], ev[k + 1]) : hipSuccess;
        *ms = t;
        return e;
    }
    hipError_t read_all(double *ms) const {   // ms[0 .. K - 2]
        hipError_t e = hipSuccess;
        for (int k = 0; k + 1 < K && e == hipSuccess; ++k) e = read(k, ms + k);
        return e;
    }
};

// Scratch kept per device between calls: a stream made on first use and ONE grow-only arena,
// guarded by a mutex -- calls that share a scratch serialise, which is what one stream would
// do anyway.  What it saves, and when the arena is given back, is told where each is used.
struct DeviceScratch {
    std::mutex mu;
    hipStream_t stream = nullptr;
    DevBuf buf;
    // the stream (created now if there is none yet) and at least `bytes` of arena
    hipError_t reserve(size_t bytes) {
        const hipError_t e = stream ? hipSuccess : hipStreamCreateWithFlags(&stream, hipStreamNonBlocking);
        return e == hipSuccess ? buf.reserve(bytes) : e;
    }
};

// The T of a device, one table per type T: never NULL, made on first use, lives for the
// process (freed by the runtime at exit).
template <typename T>
T *per_device(int device) {
    static std::mutex table_mu;
    static std::map<int, T *> table;
    std::lock_guard<std::mutex> lock(table_mu);
    T *&slot = table[device];
    if (!slot) slot = new T();
    return slot;
}

}  // namespace bb
