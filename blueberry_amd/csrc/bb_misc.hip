// bb_misc.hip -- the two remaining numeric Cython helpers of blueberry.pyx:
//   benjamini_hochberg   blueberry/blueberry.pyx:40-75   (sequential running max)
//   downsample           blueberry/blueberry.pyx:93-104  (5x5 max-pool, in place)
// Both are exact (max / min only, plus one multiply and one divide per element
// in the reference's operation order, NaN behaviour included), pinned by golden vectors.
//
// And the q-value rule of docs/SPEC.md 2.9.7 around that scan, for p-values that are NOT sorted:
//   qv_key_kernel      a 64-bit key per value whose unsigned order is numpy's sort order of
//                      float64 (NaN last, -0.0 == +0.0), and the value's place in the list
//   the sort           bb::stable_sort_pairs (bb_sort.h) of (key, place) over all 64 bits: ties
//                      keep list order, as numpy.argsort(kind="stable") keeps them
//   qv_gather_kernel   the ORIGINAL values in sorted order (the key is never inverted: a zero's
//                      sign and a NaN's payload reach the scan as they were)
//   the scan           bb::bh_scan_enqueue: the three bh_*_kernel launches, the one copy
//   qv_scatter_kernel  q[place[i]] = q_sorted[i]
// No floating-point atomics, no atomic cursor: the same bits on every run.
#include <vector>

#include "bb_common.h"
#include "bb_qvalues.h"
#include "bb_sort.h"

namespace {

// Per-device scratch kept between calls: a stream and ONE grow-only arena.  A fresh
// allocation is not what costs -- the first use of a freshly mapped block is, 0.17-0.35 s on
// this platform (tools/alloc_probe.py), and a stream costs 3-4 ms to make and destroy:
// small calls spent 3 ms around 0.1 ms of work.  Arenas above kKeepBytes are given
// back after the call.
constexpr size_t kKeepBytes = (size_t)1 << 30;
struct MiscScratch : bb::DeviceScratch {
    void trim() {
        if (buf.bytes > kKeepBytes) buf.reset();
    }
};

constexpr int kScanBlock = 256;
constexpr int kItems = 4;  // per thread -> 1024 elements per workgroup

// The reference's loop (pyx:66-71) is
//     q = p[i] * n / (i+1);  q = min(q, 1);  q = max(q, prev);  prev = q
// and Cython lowers min(q, 1) to `1 < q ? 1 : q` and max(q, prev) to `prev > q ? prev : q`.
// For ordinary numbers that is a running maximum; a NaN p-value comes out as NaN AND,
// because `NaN > q` is false, restarts the maximum at the next element (golden cases
// bh_*_4..7).  So the scan runs over pairs (v, cut): v = the running value since the last
// NaN, cut = "a NaN lies in this range, nothing from before it gets through".
struct BhRun {
    double v;
    int cut;
};
__device__ __forceinline__ double ref_max(double prev, double q) { return prev > q ? prev : q; }
// `later` follows `earlier` in the sequence
__device__ __forceinline__ BhRun bh_join(BhRun earlier, BhRun later) {
    BhRun r;
    r.v = later.cut ? later.v : ref_max(earlier.v, later.v);
    r.cut = earlier.cut | later.cut;
    return r;
}
__device__ __forceinline__ BhRun bh_identity() {
    BhRun r;
    r.v = -__builtin_huge_val();  // -inf > q is false for every q: lets q through
    r.cut = 0;
    return r;
}

// inclusive scan of one BhRun per thread over the workgroup (Hillis-Steele)
__device__ __forceinline__ BhRun bh_block_scan(BhRun mine, double *shv, int *shc, int tid) {
    shv[tid] = mine.v;
    shc[tid] = mine.cut;
    __syncthreads();
    for (int off = 1; off < kScanBlock; off <<= 1) {
        BhRun o = bh_identity();
        if (tid >= off) { o.v = shv[tid - off]; o.cut = shc[tid - off]; }
        __syncthreads();
        BhRun me;
        me.v = shv[tid];
        me.cut = shc[tid];
        me = bh_join(o, me);
        shv[tid] = me.v;
        shc[tid] = me.cut;
        __syncthreads();
    }
    BhRun r;
    r.v = shv[tid];
    r.cut = shc[tid];
    return r;
}

// phase 1: the scan inside each workgroup's 1024 elements; per workgroup its summary and
// the index of its first NaN (what came before the workgroup still reaches up to there)
__global__ __launch_bounds__(kScanBlock) void bh_local_kernel(const double *__restrict__ p,
                                                              int64_t d, double n,
                                                              double *__restrict__ q,
                                                              double *__restrict__ blockv,
                                                              int *__restrict__ blockcut,
                                                              int *__restrict__ firstcut) {
    __shared__ double shv[kScanBlock];
    __shared__ int shc[kScanBlock];
    __shared__ int first;
    const int tid = threadIdx.x;
    if (tid == 0) first = kScanBlock * kItems;
    __syncthreads();
    const int64_t base = ((int64_t)blockIdx.x * kScanBlock + tid) * kItems;
    BhRun v[kItems];
    BhRun run = bh_identity();
#pragma unroll
    for (int k = 0; k < kItems; ++k) {
        const int64_t i = base + k;
        if (i < d) {
            double t = p[i] * n / (double)(i + 1);
            t = 1.0 < t ? 1.0 : t;                   // min(q, 1) as the reference evaluates it
            BhRun e;
            e.v = t;
            e.cut = t != t;
            run = bh_join(run, e);
            if (e.cut) atomicMin(&first, tid * kItems + k);
        }
        v[k] = run;
    }
    const BhRun incl = bh_block_scan(run, shv, shc, tid);
    BhRun before = bh_identity();
    if (tid > 0) { before.v = shv[tid - 1]; before.cut = shc[tid - 1]; }
#pragma unroll
    for (int k = 0; k < kItems; ++k) {
        const int64_t i = base + k;
        if (i < d) q[i] = bh_join(before, v[k]).v;
    }
    if (tid == kScanBlock - 1) {
        blockv[blockIdx.x] = incl.v;
        blockcut[blockIdx.x] = incl.cut;
        firstcut[blockIdx.x] = first;
    }
}

// phase 2: exclusive scan of the workgroup summaries (one workgroup, sequential over
// chunks), seeded with the reference's prev_q_value = 0.0
__global__ __launch_bounds__(kScanBlock) void bh_blockscan_kernel(double *__restrict__ blockv,
                                                                  int *__restrict__ blockcut,
                                                                  int64_t nblocks) {
    __shared__ double shv[kScanBlock];
    __shared__ int shc[kScanBlock];
    __shared__ double carry_v;
    __shared__ int carry_c;
    const int tid = threadIdx.x;
    if (tid == 0) { carry_v = 0.0; carry_c = 0; }
    __syncthreads();
    for (int64_t c0 = 0; c0 < nblocks; c0 += kScanBlock) {
        const int64_t i = c0 + tid;
        BhRun mine = bh_identity();
        if (i < nblocks) { mine.v = blockv[i]; mine.cut = blockcut[i]; }
        const BhRun incl = bh_block_scan(mine, shv, shc, tid);
        BhRun c;
        c.v = carry_v;
        c.cut = carry_c;
        BhRun excl = bh_identity();
        if (tid > 0) { excl.v = shv[tid - 1]; excl.cut = shc[tid - 1]; }
        if (i < nblocks) blockv[i] = bh_join(c, excl).v;   // what reaches workgroup i from before
        __syncthreads();
        if (tid == kScanBlock - 1) {
            const BhRun nc = bh_join(c, incl);
            carry_v = nc.v;
            carry_c = nc.cut;
        }
        __syncthreads();
    }
}

// phase 3: fold what came before the workgroup into its elements up to its first NaN
__global__ __launch_bounds__(kScanBlock) void bh_apply_kernel(double *__restrict__ q, int64_t d,
                                                              const double *__restrict__ prefix,
                                                              const int *__restrict__ firstcut) {
    const double pre = prefix[blockIdx.x];
    const int first = firstcut[blockIdx.x];
    const int64_t base = ((int64_t)blockIdx.x * kScanBlock + threadIdx.x) * kItems;
#pragma unroll
    for (int k = 0; k < kItems; ++k) {
        const int64_t i = base + k;
        if (i < d && (int)threadIdx.x * kItems + k < first) q[i] = ref_max(pre, q[i]);
    }
}

// yp5i[i][j] = max(yp5i[i][j], max of the 5x5 block of yp1), i, j < n5 - 1
__global__ __launch_bounds__(256) void downsample_kernel(const float *__restrict__ yp1, int64_t n1,
                                                         float *__restrict__ yp5i, int64_t n5) {
    const int64_t j = (int64_t)blockIdx.x * 16 + (threadIdx.x & 15);
    const int64_t i = (int64_t)blockIdx.y * 16 + (threadIdx.x >> 4);
    if (i >= n5 - 1 || j >= n5 - 1) return;
    float m = yp5i[i * n5 + j];
    for (int a = 0; a < 5; ++a)
        for (int b = 0; b < 5; ++b) {
            const float v = yp1[(i * 5 + a) * n1 + (j * 5 + b)];
            m = v > m ? v : m;   // the reference's max(): NaN never replaces m
        }
    yp5i[i * n5 + j] = m;
}

// ---- the q-value rule (docs/SPEC.md 2.9.7) -------------------------------------------------------
typedef bb::sort_key u64;

// (the key: bb::order_key of bb_sort.h, numpy's order of float64)
__global__ __launch_bounds__(256) void qv_key_kernel(const double *__restrict__ p, int64_t m,
                                                     u64 *__restrict__ keys, uint32_t *__restrict__ place) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    keys[i] = bb::order_key(p[i]);
    place[i] = (uint32_t)i;
}

__global__ __launch_bounds__(256) void qv_gather_kernel(const double *__restrict__ p,
                                                        const uint32_t *__restrict__ place, int64_t m,
                                                        double *__restrict__ sorted) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < m) sorted[i] = p[place[i]];
}

__global__ __launch_bounds__(256) void qv_scatter_kernel(const double *__restrict__ sorted,
                                                         const uint32_t *__restrict__ place, int64_t m,
                                                         double *__restrict__ q) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < m) q[place[i]] = sorted[i];
}

inline int64_t bh_blocks(int64_t d) {
    const int64_t per_block = (int64_t)kScanBlock * kItems;
    return (d + per_block - 1) / per_block;
}

}  // namespace

size_t bb::bh_scan_work_bytes(int64_t d) {
    const size_t nblocks = (size_t)bh_blocks(d);
    return bb::align256(nblocks * 8) + 2 * bb::align256(nblocks * 4);
}

// work: per workgroup its summary value | its cut mark | the index of its first NaN
hipError_t bb::bh_scan_enqueue(const double *p, int64_t d, double n, double *q, void *work, hipStream_t st) {
    const int64_t nblocks = bh_blocks(d);
    char *w = (char *)work;
    double *bm = (double *)w;
    int *bc = (int *)(w + bb::align256((size_t)nblocks * 8)), *fc = bc + bb::align256((size_t)nblocks * 4) / 4;
    hipError_t e = bb::launch(bh_local_kernel, dim3((unsigned)nblocks), dim3(kScanBlock), 0, st, p, d, n, q, bm,
                              bc, fc);
    if (e == hipSuccess) e = bb::launch(bh_blockscan_kernel, dim3(1), dim3(kScanBlock), 0, st, bm, bc, nblocks);
    if (e == hipSuccess)
        e = bb::launch(bh_apply_kernel, dim3((unsigned)nblocks), dim3(kScanBlock), 0, st, q, d,
                       (const double *)bm, (const int *)fc);
    return e;
}

int bb::q_values_device(const char *who, const double *p, int64_t m, int64_t n_tests, double *q,
                        uint32_t *order, hipStream_t st, double *sort_ms, double *scan_ms) {
    if (sort_ms) *sort_ms = 0.0;
    if (scan_ms) *scan_ms = 0.0;
    BB_REQUIRE(m >= 0 && m < ((int64_t)1 << 32),
               std::string(who) + ": the number of p-values must be in [0, 2^32)");
    if (m == 0) return BB_OK;
    // keys A | keys B | places A | places B | the gathered p | the sorted q | the scan's summaries
    const size_t k8 = bb::align256((size_t)m * 8), k4 = bb::align256((size_t)m * 4);
    bb::DevBuf work;
    BB_TRY(bb::hip_status(who, work.alloc(4 * k8 + 2 * k4 + bb::bh_scan_work_bytes(m)), BB_ERR_NOMEM));
    char *base = (char *)work.p;
    u64 *ka = (u64 *)base, *kb = (u64 *)(base + k8);
    uint32_t *ia = (uint32_t *)(base + 2 * k8), *ib = (uint32_t *)(base + 2 * k8 + k4);
    double *ps = (double *)(base + 2 * k8 + 2 * k4), *qs = (double *)(base + 3 * k8 + 2 * k4);
    void *bh_work = base + 4 * k8 + 2 * k4;
    const dim3 grid((unsigned)((m + 255) / 256)), block(256);
    bb::StageClock<3> clock;                      // sort | gather, scan, scatter
    hipError_t e = clock.start(sort_ms != nullptr || scan_ms != nullptr);
    if (e == hipSuccess) e = clock.mark(0, st);
    if (e == hipSuccess) e = bb::launch(qv_key_kernel, grid, block, 0, st, p, m, ka, ia);
    if (e == hipSuccess) {
        e = bb::stable_sort_pairs<uint32_t>(ka, ia, kb, ib, m, 64, st);   // (ia: the sorted order)
        if (e == hipErrorOutOfMemory) return bb::hip_status(who, e, BB_ERR_NOMEM);
    }
    if (e == hipSuccess) e = clock.mark(1, st);
    if (e == hipSuccess) e = bb::launch(qv_gather_kernel, grid, block, 0, st, p, (const uint32_t *)ia, m, ps);
    if (e == hipSuccess) e = bb::bh_scan_enqueue(ps, m, (double)n_tests, qs, bh_work, st);
    if (e == hipSuccess)
        e = bb::launch(qv_scatter_kernel, grid, block, 0, st, (const double *)qs, (const uint32_t *)ia, m, q);
    if (e == hipSuccess) e = clock.mark(2, st);
    if (e == hipSuccess && order != nullptr)
        e = hipMemcpyAsync(order, ia, (size_t)m * 4, hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    double ms[2] = {0.0, 0.0};
    if (e == hipSuccess) e = clock.read_all(ms);
    BB_TRY(bb::hip_status(who, e));
    if (sort_ms) *sort_ms = ms[0];
    if (scan_ms) *scan_ms = ms[1];
    return BB_OK;
}

extern "C" {

int bb_benjamini_hochberg(const double *p_values, int64_t d, int64_t n, double *q_values,
                          int device) {
    BB_REQUIRE(d >= 0, "bb_benjamini_hochberg: d < 0");
    BB_REQUIRE(d == 0 || (p_values != nullptr && q_values != nullptr),
               "bb_benjamini_hochberg: NULL argument");
    int rc = bb::use_device(device);
    if (rc != BB_OK) return rc;
    if (d == 0) return BB_OK;
    MiscScratch *c = bb::per_device<MiscScratch>(device);
    std::lock_guard<std::mutex> lock(c->mu);
    const size_t o_q = bb::align256((size_t)d * 8), o_work = o_q + bb::align256((size_t)d * 8),
                 total = o_work + bb::bh_scan_work_bytes(d);
    hipError_t e = c->reserve(total);
    BB_TRY(bb::hip_status("bb_benjamini_hochberg", e, BB_ERR_NOMEM));
    hipStream_t st = c->stream;
    char *arena = (char *)c->buf.p;
    double *p = (double *)arena, *q = (double *)(arena + o_q);
    e = hipMemcpyAsync(p, p_values, (size_t)d * 8, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = bb::bh_scan_enqueue(p, d, (double)n, q, arena + o_work, st);
    if (e == hipSuccess)
        e = hipMemcpyAsync(q_values, q, (size_t)d * 8, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    c->trim();
    return bb::hip_status("bb_benjamini_hochberg", e);
}

int bb_q_values(const double *p, int64_t m, int64_t n_tests, double *q, int64_t *order, int device) {
    BB_REQUIRE(m >= 0 && m < ((int64_t)1 << 32), "bb_q_values: the number of p-values must be in [0, 2^32)");
    BB_REQUIRE(n_tests >= 0, "bb_q_values: negative n_tests");
    BB_REQUIRE(m == 0 || (p != nullptr && q != nullptr), "bb_q_values: NULL argument");
    BB_TRY(bb::use_device(device));
    if (m == 0) return BB_OK;
    MiscScratch *c = bb::per_device<MiscScratch>(device);
    std::lock_guard<std::mutex> lock(c->mu);
    // the arena stages p | q | the order; the sort's own buffers are the call's (bb::q_values_device)
    const size_t o_q = bb::align256((size_t)m * 8), o_ord = 2 * o_q,
                 total = o_ord + (order ? bb::align256((size_t)m * 4) : 0);
    BB_TRY(bb::hip_status("bb_q_values", c->reserve(total), BB_ERR_NOMEM));
    hipStream_t st = c->stream;
    char *arena = (char *)c->buf.p;
    double *dp = (double *)arena, *dq = (double *)(arena + o_q);
    uint32_t *dord = order ? (uint32_t *)(arena + o_ord) : nullptr;
    int rc = bb::hip_status("bb_q_values", hipMemcpyAsync(dp, p, (size_t)m * 8, hipMemcpyHostToDevice, st));
    if (rc == BB_OK) rc = bb::q_values_device("bb_q_values", dp, m, n_tests, dq, dord, st, nullptr, nullptr);
    if (rc == BB_OK) {
        std::vector<uint32_t> ord(order ? (size_t)m : 0);
        hipError_t e = hipMemcpyAsync(q, dq, (size_t)m * 8, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && order)
            e = hipMemcpyAsync(ord.data(), dord, (size_t)m * 4, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        rc = bb::hip_status("bb_q_values", e);
        if (rc == BB_OK)
            for (size_t i = 0; i < ord.size(); ++i) order[i] = (int64_t)ord[i];
    }
    c->trim();
    return rc;
}

int bb_downsample(const float *yp1, int64_t n1, float *yp5i, int64_t n5, int device) {
    BB_REQUIRE(yp1 != nullptr && yp5i != nullptr, "bb_downsample: NULL argument");
    BB_REQUIRE(n5 >= 1 && n1 >= 5 * (n5 - 1), "bb_downsample: yp1 smaller than 5 * (n5 - 1)");
    int rc = bb::use_device(device);
    if (rc != BB_OK) return rc;
    if (n5 < 2) return BB_OK;
    MiscScratch *c = bb::per_device<MiscScratch>(device);
    std::lock_guard<std::mutex> lock(c->mu);
    const size_t o_b = bb::align256((size_t)n1 * n1 * 4), total = o_b + bb::align256((size_t)n5 * n5 * 4);
    hipError_t e = c->reserve(total);
    BB_TRY(bb::hip_status("bb_downsample", e, BB_ERR_NOMEM));
    hipStream_t st = c->stream;
    float *a = (float *)c->buf.p, *b = (float *)((char *)c->buf.p + o_b);
    e = hipMemcpyAsync(a, yp1, (size_t)n1 * n1 * 4, hipMemcpyHostToDevice, st);
    if (e == hipSuccess)
        e = hipMemcpyAsync(b, yp5i, (size_t)n5 * n5 * 4, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) {
        const unsigned g = (unsigned)((n5 - 1 + 15) / 16);
        e = bb::launch(downsample_kernel, dim3(g, g), dim3(256), 0, st, (const float *)a, n1, b, n5);
    }
    if (e == hipSuccess)
        e = hipMemcpyAsync(yp5i, b, (size_t)n5 * n5 * 4, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    c->trim();
    return bb::hip_status("bb_downsample", e);
}

}  // extern "C"
