// bb_triples_paths.hip -- shortest paths from a few sources over the graph that resident triples
// define, never forming the dense matrix (docs/SPEC.md 2.1.2): the geodesic rows a landmark
// start needs (SPEC 2.5.4), L x N doubles where the dense completion (bb_shortest.hip) needs N x N.
//
//   the graph   nodes 0 .. n_nodes - 1; one undirected edge per stored off-diagonal cell of the
//               handle's canonical index for n_nodes (bb_triples_balance.hip: a CSR of the
//               symmetric matrix, columns ascending, the last triple of a pair the winner, cut
//               into segments of kTbSeg entries).  Its weight is the wish distance of SPEC 2.1 in
//               float64: the stored value, divided by KRnorm[i] KRnorm[j] KRexpected[j - i]
//               (i < j) and nan_to_num'ed if the vectors are given, through bb::wish_from_value
//               (bb_wish.h, the rule of every pack kernel).  0 -- anything that is not a finite
//               positive distance -- is no edge.  weights_kernel forms them once per call into
//               an array parallel to the index entries (8 B per directed entry), and counts
//               them per node for bb_triples_edge_degrees (an integer atomic per segment).
//   D           one row of `ld` doubles per node, ld = n_sources rounded up to 64: a wave reads
//               the 64 sources of a chunk of one node as 512 contiguous bytes.  +inf everywhere,
//               0 at each source's own node; the padding columns stay +inf.
//   sweep_kernel   multi-source Bellman-Ford, (min, +) where balance's segmented product has
//               (+, x): a wave takes one segment (<= kTbSeg entries of one row v) and one chunk
//               of 64 sources, lane = source.  It loads 64 (column, weight) pairs at a time,
//               coalesced, hands them round with v_readlane, and keeps acc = min(acc, D[u][lane]
//               + w).  Where acc ends below D[v][lane] it lowers that cell with an INTEGER atomic
//               min on the bit pattern (non-negative doubles order as their bits): min is exact
//               and order-free, so the segments of a long row need no second pass.  D is updated
//               IN PLACE: a cell only ever holds +inf or the float64 length of a real path and
//               only ever falls, and the fixed point of d[v] = min(d[v], fl(d[u] + w)) is unique
//               (fl(a + w) is monotone in a, w > 0) -- the bits of the result are those of
//               Dijkstra's algorithm in float64 whatever the order of relaxation.  Only the
//               NUMBER of sweeps depends on the order in which the waves of a launch run: `sweeps`
//               is not reproducible from run to run.
//   the loop    one launch per sweep, no waiting between workgroups.  A sweep that lowers a
//               cell stores 1 into its own flag (plain stores); sweep k of a batch returns at
//               once if sweep k - 1 changed nothing; the host reads a batch's flags in one copy.
//               Ends at the first sweep that changes nothing, after at most n_nodes sweeps
//               (n_nodes - 1 relax every simple path, one confirms).  Nothing is allocated per
//               sweep.
//   place_kernel   landmark placement from the resident rows: X[j][c] = -1/2 sum_a coef[a][c]
//               (D[j][a]^2 - mu[a]), a ascending, one thread per node.
// Float64, no floating-point atomics.
#include <math.h>

#include <algorithm>
#include <memory>
#include <string>
#include <vector>

#include "bb_common.h"
#include "bb_device_sums.h"
#include "bb_triples.h"
#include "bb_wish.h"

namespace {

using bb::kTbSeg;
using bb::SegmentedList;

typedef unsigned long long u64;

constexpr int64_t kMaxSources = 1024;   // (the header's BB_PATHS_MAX_SOURCES)
constexpr int kBatch = 8;               // sweeps per read of the flags

#define TP_HIP(expr)                             \
    do {                                         \
        const hipError_t _e = (expr);            \
        if (_e != hipSuccess) return _e;         \
    } while (0)

inline dim3 grid256(int64_t n) { return dim3((unsigned)((std::max<int64_t>(n, 1) + 255) / 256)); }

__device__ __forceinline__ double readlane_f64(double v, int l) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), l);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
    return __hiloint2double(hi, lo);
}

// flag[0] = 1 if a triple names a bin outside [0, n_nodes)
__global__ __launch_bounds__(256) void bins_check_kernel(const double *__restrict__ tr, int64_t n, int64_t st,
                                                         int64_t sc, double resolution, int64_t n_nodes,
                                                         int *__restrict__ flag) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    int j, k;
    if (!bb::triple_bins(bb::nan_to_num(tr[t * st]), bb::nan_to_num(tr[t * st + sc]), resolution, n_nodes,
                         j, k))
        flag[0] = 1;
}

// wt[e] = the weight of directed entry e (0: no edge), and / or deg[row] += the edges of the
// segment.  One wave per segment, 4 per workgroup.
__global__ __launch_bounds__(256) void weights_kernel(const long long *__restrict__ ptr,
                                                      const int *__restrict__ other,
                                                      const double *__restrict__ val,
                                                      const long long *__restrict__ seg_ptr,
                                                      const int *__restrict__ seg_owner, int64_t n_seg,
                                                      int kind, double neg_inv_alpha,
                                                      const double *__restrict__ kr,
                                                      const double *__restrict__ krexp,
                                                      double *__restrict__ wt, u64 *__restrict__ deg) {
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= n_seg) return;                       // (whole waves)
    const int64_t o = seg_owner[w];
    const int64_t begin = ptr[o] + (w - seg_ptr[o]) * kTbSeg;
    const int64_t end = std::min<int64_t>(ptr[o + 1], begin + kTbSeg);
    int edges = 0;
    for (int64_t e = begin + lane; e < end; e += 64) {
        const int64_t c = other[e];
        double v = val[e];                        // (nan_to_num'ed when the index was built)
        const int64_t i = std::min(o, c), j = std::max(o, c);
        if (kr != nullptr) v = bb::nan_to_num(v / (kr[i] * kr[j] * krexp[j - i]));
        const double d = c == o ? 0.0 : bb::wish_from_value<double>(v, kind, neg_inv_alpha);
        if (wt != nullptr) wt[e] = d;
        edges += d > 0.0 ? 1 : 0;
    }
    if (deg != nullptr) {
        edges = bb::wave_sum_first(edges);
        if (lane == 0 && edges > 0) atomicAdd(deg + o, (u64)edges);
    }
}

// D = +inf, then 0 at (sources[a], a)
__global__ __launch_bounds__(256) void fill_inf_kernel(double *__restrict__ D, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) D[i] = INFINITY;
}
__global__ __launch_bounds__(256) void seed_sources_kernel(double *__restrict__ D, int64_t ld,
                                                           const long long *__restrict__ sources,
                                                           int64_t n_sources) {
    const int64_t a = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (a < n_sources) D[sources[a] * ld + a] = 0.0;
}

// Sweep k of a batch: wave W = (segment W / n_chunks, chunk W % n_chunks).  flags[k] = 1 if a
// cell fell; nothing is done once the sweep before changed nothing.
__global__ __launch_bounds__(256) void sweep_kernel(const long long *__restrict__ ptr,
                                                    const int *__restrict__ other,
                                                    const double *__restrict__ wt,
                                                    const long long *__restrict__ seg_ptr,
                                                    const int *__restrict__ seg_owner, int64_t n_waves,
                                                    int64_t n_chunks, int64_t ld, double *D, int *flags,
                                                    int k) {
    if (k > 0 && flags[k - 1] == 0) return;
    const int lane = threadIdx.x & 63;
    const int64_t W = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (W >= n_waves) return;                     // (whole waves: no barrier follows)
    const int64_t seg = W / n_chunks, col = (W - seg * n_chunks) * 64 + lane;
    const int64_t v = seg_owner[seg];
    const int64_t begin = ptr[v] + (seg - seg_ptr[v]) * kTbSeg;
    const int64_t end = std::min<int64_t>(ptr[v + 1], begin + kTbSeg);
    double *mine = D + v * ld + col;
    const double *Dc = D + col;
    const double old = *mine;
    double acc = old;
    for (int64_t e0 = begin; e0 < end; e0 += 64) {
        const int64_t e = e0 + lane;
        const bool in = e < end;
        const int c = in ? other[e] : 0;
        const double w = in ? wt[e] : 0.0;        // (0: no edge, and the lanes past the end)
        const int cnt = (int)std::min<int64_t>(64, end - e0);
        for (int k0 = 0; k0 < cnt; k0 += 4) {     // (k0 + 3 <= 63: the lanes past cnt hold w = 0)
            double d[4], ww[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int u = __builtin_amdgcn_readlane(c, k0 + q);
                ww[q] = readlane_f64(w, k0 + q);
                d[q] = ww[q] > 0.0 ? Dc[(int64_t)u * ld] : INFINITY;
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) acc = fmin(acc, d[q] + ww[q]);
        }
    }
    if (acc < old) {
        atomicMin((u64 *)mine, (u64)__double_as_longlong(acc));
        flags[k] = 1;
    }
}

// count[0] += the cells (node, a < n_sources) that are still +inf
__global__ __launch_bounds__(256) void count_inf_kernel(const double *__restrict__ D, int64_t n_nodes,
                                                        int64_t ld, int64_t n_sources,
                                                        u64 *__restrict__ count) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool none = false;
    if (i < n_nodes * ld) none = (i % ld) < n_sources && D[i] == INFINITY;
    const u64 votes = __ballot(none);
    if ((threadIdx.x & 63) == 0 && votes != 0) atomicAdd(count, (u64)__popcll(votes));
}

// reached[a] += the nodes of the workgroup's slab of 256 whose D[node][a] is finite; lane = source
// of chunk blockIdx.y, the 4 waves take every fourth node
__global__ __launch_bounds__(256) void reached_kernel(const double *__restrict__ D, int64_t n_nodes,
                                                      int64_t ld, int64_t n_sources,
                                                      u64 *__restrict__ reached) {
    const int64_t a = (int64_t)blockIdx.y * 64 + (threadIdx.x & 63);
    const int64_t j0 = (int64_t)blockIdx.x * 256, j1 = std::min<int64_t>(n_nodes, j0 + 256);
    u64 n = 0;
    for (int64_t j = j0 + (threadIdx.x >> 6); j < j1; j += 4) n += D[j * ld + a] != INFINITY ? 1 : 0;
    if (a < n_sources && n > 0) atomicAdd(reached + a, n);
}

// out[(a - a0) * m + q] = D[node_q][a] for a0 <= a < a1, +inf as 0; nodes == NULL: node_q = q
__global__ __launch_bounds__(256) void gather_kernel(const double *__restrict__ D, int64_t ld,
                                                     const long long *__restrict__ nodes, int64_t m,
                                                     int64_t a0, int64_t a1, double *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (a1 - a0) * m) return;
    const int64_t a = a0 + i / m, q = i % m;
    const int64_t node = nodes != nullptr ? nodes[q] : q;
    const double d = D[node * ld + a];
    out[i] = d == INFINITY ? 0.0 : d;
}

// X[j] = -1/2 sum_a coef[a] (D[j][a]^2 - mu[a]), a ascending over the sources that take part (a
// source whose coef row and mu are all 0 does not: a dropped landmark); placed[j] = 0 and X[j]
// left alone if one of their distances is +inf
__global__ __launch_bounds__(256) void place_kernel(const double *__restrict__ D, int64_t n_nodes,
                                                    int64_t ld, int64_t n_sources,
                                                    const double *__restrict__ coef,
                                                    const double *__restrict__ mu, double *__restrict__ X,
                                                    unsigned char *__restrict__ placed) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n_nodes) return;
    const double *row = D + j * ld;
    double x = 0.0, y = 0.0, z = 0.0;
    bool ok = true;
    for (int64_t a = 0; a < n_sources; ++a) {
        const double c0 = coef[3 * a], c1 = coef[3 * a + 1], c2 = coef[3 * a + 2], m = mu[a];
        if (c0 == 0.0 && c1 == 0.0 && c2 == 0.0 && m == 0.0) continue;   // a source that takes no part
        const double d = row[a];
        ok = ok && d != INFINITY;
        const double t = d * d - m;
        x += c0 * t;
        y += c1 * t;
        z += c2 * t;
    }
    placed[j] = ok ? 1 : 0;
    if (ok) {
        X[3 * j] = -0.5 * x;
        X[3 * j + 1] = -0.5 * y;
        X[3 * j + 2] = -0.5 * z;
    }
}

// ---- host side ---------------------------------------------------------------------------------
int check_args(const char *who, const bb_triples *t, int64_t n_nodes, int kind, double alpha,
               const double *KRnorm, const double *KRexpected) {
    const std::string w(who);
    BB_REQUIRE(t != nullptr, w + ": triples is NULL");
    BB_REQUIRE(n_nodes >= 1 && n_nodes < 2147483647, w + ": n_nodes is out of range");
    BB_REQUIRE(kind == BB_KIND_WISH || kind == BB_KIND_COUNTS, w + ": bad kind");
    BB_REQUIRE(alpha > 0.0, w + ": alpha must be > 0");
    BB_REQUIRE((KRnorm == nullptr) == (KRexpected == nullptr), w + ": KRnorm and KRexpected go together");
    return BB_OK;
}

// The index of the graph: every bin inside it (as bb_solver_set_wish_triples refuses a bin
// outside its map), then the handle's canonical index for n_nodes.
int graph_index(bb_triples *t, int64_t n_nodes, const char *who) {
    BB_TRY(bb::enter_device(t->device));
    bb::DevBuf flag;
    BB_TRY(bb::hip_status(who, flag.alloc(sizeof(int)), BB_ERR_NOMEM));
    int bad = 0;
    hipError_t e = hipMemsetAsync(flag.p, 0, sizeof(int), nullptr);
    if (e == hipSuccess && t->n > 0)
        e = bb::launch(bins_check_kernel, grid256(t->n), dim3(256), 0, (hipStream_t) nullptr, t->from(0), t->n,
                       t->st, t->sc, t->resolution, n_nodes, flag.as<int>());
    if (e == hipSuccess) e = hipMemcpy(&bad, flag.p, sizeof(int), hipMemcpyDeviceToHost);
    BB_TRY(bb::hip_status(who, e));
    if (bad) return bb::fail(BB_ERR_INVALID, std::string(who) + ": an index is outside [0, n_nodes)");
    return bb::triples_ensure_index(t, n_nodes, who);
}

// The KR vectors (n_nodes doubles each) on the device, or two NULL views.
hipError_t upload_kr(const double *KRnorm, const double *KRexpected, int64_t n_nodes, bb::DevBuf &buf,
                     const double **kr, const double **ke) {
    *kr = *ke = nullptr;
    if (KRnorm == nullptr) return hipSuccess;
    TP_HIP(buf.alloc((size_t)n_nodes * 16));
    TP_HIP(hipMemcpy(buf.p, KRnorm, (size_t)n_nodes * 8, hipMemcpyHostToDevice));
    TP_HIP(hipMemcpy(buf.as<double>() + n_nodes, KRexpected, (size_t)n_nodes * 8, hipMemcpyHostToDevice));
    *kr = buf.as<double>();
    *ke = buf.as<double>() + n_nodes;
    return hipSuccess;
}

hipError_t weights_enqueue(const SegmentedList &rows, int kind, double alpha, const double *kr,
                           const double *ke, double *wt, u64 *deg) {
    if (rows.n_seg == 0) return hipSuccess;
    return bb::launch(weights_kernel, dim3((unsigned)((rows.n_seg + 3) / 4)), dim3(256), 0,
                      (hipStream_t) nullptr, (const long long *)rows.ptr.p, (const int *)rows.other.p,
                      (const double *)rows.val.p, (const long long *)rows.seg_ptr.p,
                      (const int *)rows.seg_owner.p, rows.n_seg, kind, -1.0 / alpha, kr, ke, wt, deg);
}

// The sweeps to the fixed point.  *sweeps: the launches that ran, the confirming one included.
hipError_t run_sweeps(const SegmentedList &rows, const double *wt, bb_paths *p, int *flags,
                      int64_t *sweeps, bool *converged) {
    hipStream_t st = nullptr;
    const int64_t n_chunks = p->ld / 64, n_waves = rows.n_seg * n_chunks;
    *sweeps = 0;
    *converged = true;
    if (n_waves == 0) return hipSuccess;          // no stored cell: nothing to relax
    *converged = false;
    int host_flags[kBatch];
    while (*sweeps < p->n_nodes) {
        const int batch = (int)std::min<int64_t>(kBatch, p->n_nodes - *sweeps);
        TP_HIP(hipMemsetAsync(flags, 0, sizeof(int) * kBatch, st));
        for (int k = 0; k < batch; ++k)
            TP_HIP(bb::launch(sweep_kernel, dim3((unsigned)((n_waves + 3) / 4)), dim3(256), 0, st,
                              (const long long *)rows.ptr.p, (const int *)rows.other.p, wt,
                              (const long long *)rows.seg_ptr.p, (const int *)rows.seg_owner.p, n_waves,
                              n_chunks, p->ld, p->D.as<double>(), flags, k));
        TP_HIP(hipMemcpy(host_flags, flags, sizeof(int) * kBatch, hipMemcpyDeviceToHost));
        for (int k = 0; k < batch; ++k) {
            ++*sweeps;
            if (host_flags[k] == 0) {
                *converged = true;
                return hipSuccess;
            }
        }
    }
    return hipSuccess;
}

}  // namespace

extern "C" {

int bb_triples_edge_degrees(bb_triples *t, int64_t n_nodes, int kind, double alpha, const double *KRnorm,
                            const double *KRexpected, int64_t *deg) {
    const char *who = "bb_triples_edge_degrees";
    BB_TRY(check_args(who, t, n_nodes, kind, alpha, KRnorm, KRexpected));
    BB_REQUIRE(deg != nullptr, "bb_triples_edge_degrees: NULL argument");
    BB_TRY(graph_index(t, n_nodes, who));
    bb::DevBuf kr_buf, bdeg;
    const double *kr, *ke;
    hipError_t e = bdeg.alloc((size_t)n_nodes * 8);
    if (e == hipSuccess) e = upload_kr(KRnorm, KRexpected, n_nodes, kr_buf, &kr, &ke);
    if (e == hipErrorOutOfMemory) return bb::hip_status(who, e, BB_ERR_NOMEM);
    if (e == hipSuccess) e = hipMemsetAsync(bdeg.p, 0, (size_t)n_nodes * 8, nullptr);
    if (e == hipSuccess) e = weights_enqueue(t->index.rows, kind, alpha, kr, ke, nullptr, bdeg.as<u64>());
    if (e == hipSuccess) e = hipMemcpy(deg, bdeg.p, (size_t)n_nodes * 8, hipMemcpyDeviceToHost);
    return bb::hip_status(who, e);
}

int bb_triples_paths(bb_triples *t, int64_t n_nodes, int kind, double alpha, const double *KRnorm,
                     const double *KRexpected, const int64_t *sources, int64_t n_sources, bb_paths **out) {
    const char *who = "bb_triples_paths";
    BB_REQUIRE(out != nullptr, "bb_triples_paths: out is NULL");
    *out = nullptr;
    BB_TRY(check_args(who, t, n_nodes, kind, alpha, KRnorm, KRexpected));
    BB_REQUIRE(sources != nullptr, "bb_triples_paths: sources is NULL");
    BB_REQUIRE(n_sources >= 1 && n_sources <= kMaxSources,
               "bb_triples_paths: n_sources must be in [1, " + std::to_string(kMaxSources) + "]");
    for (int64_t a = 0; a < n_sources; ++a)
        BB_REQUIRE(sources[a] >= 0 && sources[a] < n_nodes,
                   "bb_triples_paths: source " + std::to_string(a) + " is outside [0, n_nodes)");
    BB_TRY(graph_index(t, n_nodes, who));
    const SegmentedList &rows = t->index.rows;

    // the size, up front: D, the weights, and what is asked of the device
    const int64_t ld = bb::round_up(n_sources, 64);
    const size_t d_bytes = (size_t)n_nodes * (size_t)ld * 8, w_bytes = (size_t)rows.n_entries * 8;
    size_t free_b = 0, total_b = 0;
    BB_TRY(bb::hip_status(who, hipMemGetInfo(&free_b, &total_b)));
    const std::string sizes = "the distances of " + std::to_string(n_sources) + " sources to " +
                              std::to_string(n_nodes) + " nodes need " + std::to_string(d_bytes) +
                              " B and the edge weights " + std::to_string(w_bytes) + " B; " +
                              std::to_string(free_b) + " B are free";
    if (d_bytes + w_bytes > free_b) return bb::fail(BB_ERR_NOMEM, std::string(who) + ": " + sizes);

    std::unique_ptr<bb_paths> p(new (std::nothrow) bb_paths());
    if (!p) return bb::fail(BB_ERR_NOMEM, "bb_triples_paths: out of host memory");
    p->device = t->device;
    p->n_sources = n_sources;
    p->sources.assign(sources, sources + n_sources);
    p->n_nodes = n_nodes;
    p->ld = ld;
    bb::DevBuf wt, kr_buf, small;                 // small: sources | flags | the count
    bb::StageClock<3> clock;                      // the weights | the sweeps
    const double *kr = nullptr, *ke = nullptr;
    const size_t src_bytes = bb::align256((size_t)n_sources * 8);
    hipError_t e = p->D.alloc(d_bytes);
    if (e == hipSuccess) e = wt.alloc(w_bytes);
    if (e == hipSuccess) e = small.alloc(src_bytes + 512);
    if (e == hipSuccess) e = upload_kr(KRnorm, KRexpected, n_nodes, kr_buf, &kr, &ke);
    if (e == hipErrorOutOfMemory)
        return bb::fail(BB_ERR_NOMEM, std::string(who) + ": hipMalloc failed: " + sizes);
    hipStream_t st = nullptr;
    long long *d_sources = small.as<long long>();
    int *flags = (int *)((char *)small.p + src_bytes);
    u64 *count = (u64 *)((char *)small.p + src_bytes + 256);
    bool converged = false;
    if (e == hipSuccess) e = clock.start();
    if (e == hipSuccess) e = hipMemcpy(d_sources, sources, (size_t)n_sources * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemsetAsync(count, 0, 8, st);
    if (e == hipSuccess) e = clock.mark(0, st);
    if (e == hipSuccess) e = weights_enqueue(rows, kind, alpha, kr, ke, wt.as<double>(), nullptr);
    if (e == hipSuccess) e = clock.mark(1, st);
    if (e == hipSuccess)
        e = bb::launch(fill_inf_kernel, grid256(n_nodes * ld), dim3(256), 0, st, p->D.as<double>(), n_nodes * ld);
    if (e == hipSuccess)
        e = bb::launch(seed_sources_kernel, grid256(n_sources), dim3(256), 0, st, p->D.as<double>(), ld,
                       (const long long *)d_sources, n_sources);
    if (e == hipSuccess) e = run_sweeps(rows, wt.as<double>(), p.get(), flags, &p->sweeps, &converged);
    if (e == hipSuccess) e = clock.mark(2, st);
    if (e == hipSuccess)
        e = bb::launch(count_inf_kernel, grid256(n_nodes * ld), dim3(256), 0, st, (const double *)p->D.p,
                       n_nodes, ld, n_sources, count);
    u64 none = 0;
    if (e == hipSuccess) e = hipMemcpy(&none, count, 8, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = clock.read(0, &p->weights_ms);
    if (e == hipSuccess) e = clock.read(1, &p->sweeps_ms);
    BB_TRY(bb::hip_status(who, e));
    if (!converged) return bb::fail(BB_ERR_STATE, "bb_triples_paths: no fixed point after n_nodes sweeps");
    p->unreachable = (int64_t)none;
    *out = p.release();
    return BB_OK;
}

int bb_paths_info(const bb_paths *p, int64_t *n_sources, int64_t *n_nodes, int64_t *sweeps,
                  int64_t *unreachable) {
    BB_REQUIRE(p != nullptr, "bb_paths_info: paths are NULL");
    if (n_sources) *n_sources = p->n_sources;
    if (n_nodes) *n_nodes = p->n_nodes;
    if (sweeps) *sweeps = p->sweeps;
    if (unreachable) *unreachable = p->unreachable;
    return BB_OK;
}

int bb_paths_timing(const bb_paths *p, double *weights_ms, double *sweeps_ms) {
    BB_REQUIRE(p != nullptr, "bb_paths_timing: paths are NULL");
    if (weights_ms) *weights_ms = p->weights_ms;
    if (sweeps_ms) *sweeps_ms = p->sweeps_ms;
    return BB_OK;
}

int bb_paths_reached(const bb_paths *p, int64_t *reached) {
    const char *who = "bb_paths_reached";
    BB_REQUIRE(p != nullptr && reached != nullptr, "bb_paths_reached: NULL argument");
    BB_TRY(bb::enter_device(p->device));
    bb::DevBuf br;
    BB_TRY(bb::hip_status(who, br.alloc((size_t)p->n_sources * 8), BB_ERR_NOMEM));
    hipError_t e = hipMemsetAsync(br.p, 0, (size_t)p->n_sources * 8, nullptr);
    if (e == hipSuccess)
        e = bb::launch(reached_kernel, dim3((unsigned)((p->n_nodes + 255) / 256), (unsigned)(p->ld / 64)),
                       dim3(256), 0, (hipStream_t) nullptr, (const double *)p->D.p, p->n_nodes, p->ld,
                       p->n_sources, br.as<u64>());
    if (e == hipSuccess) e = hipMemcpy(reached, br.p, (size_t)p->n_sources * 8, hipMemcpyDeviceToHost);
    return bb::hip_status(who, e);
}

int bb_paths_read_columns(const bb_paths *p, const int64_t *nodes, int64_t m, double *out) {
    const char *who = "bb_paths_read_columns";
    BB_REQUIRE(p != nullptr, "bb_paths_read_columns: paths are NULL");
    BB_REQUIRE(m >= 0 && (m == 0 || (nodes != nullptr && out != nullptr)),
               "bb_paths_read_columns: NULL argument");
    for (int64_t q = 0; q < m; ++q)
        BB_REQUIRE(nodes[q] >= 0 && nodes[q] < p->n_nodes,
                   "bb_paths_read_columns: node " + std::to_string(q) + " is outside [0, n_nodes)");
    if (m == 0) return BB_OK;
    BB_TRY(bb::enter_device(p->device));
    bb::DevBuf bn, bo;
    const int64_t rows_at_once = std::min<int64_t>(p->n_sources, 64);
    hipError_t e = bn.alloc((size_t)m * 8);
    if (e == hipSuccess) e = bo.alloc((size_t)(rows_at_once * m) * 8);
    BB_TRY(bb::hip_status(who, e, BB_ERR_NOMEM));
    e = hipMemcpy(bn.p, nodes, (size_t)m * 8, hipMemcpyHostToDevice);
    for (int64_t a0 = 0; a0 < p->n_sources && e == hipSuccess; a0 += rows_at_once) {
        const int64_t a1 = std::min(p->n_sources, a0 + rows_at_once);
        e = bb::launch(gather_kernel, grid256((a1 - a0) * m), dim3(256), 0, (hipStream_t) nullptr,
                       (const double *)p->D.p, p->ld, (const long long *)bn.p, m, a0, a1, bo.as<double>());
        if (e == hipSuccess) e = hipMemcpy(out + a0 * m, bo.p, (size_t)((a1 - a0) * m) * 8, hipMemcpyDeviceToHost);
    }
    return bb::hip_status(who, e);
}

int bb_paths_read(const bb_paths *p, double *dist) {
    const char *who = "bb_paths_read";
    BB_REQUIRE(p != nullptr && dist != nullptr, "bb_paths_read: NULL argument");
    BB_TRY(bb::enter_device(p->device));
    // 64 sources at a time through one staging buffer
    const int64_t m = p->n_nodes, rows_at_once = std::min<int64_t>(p->n_sources, 64);
    bb::DevBuf bo;
    BB_TRY(bb::hip_status(who, bo.alloc((size_t)(rows_at_once * m) * 8), BB_ERR_NOMEM));
    hipError_t e = hipSuccess;
    for (int64_t a0 = 0; a0 < p->n_sources && e == hipSuccess; a0 += rows_at_once) {
        const int64_t a1 = std::min(p->n_sources, a0 + rows_at_once);
        e = bb::launch(gather_kernel, grid256((a1 - a0) * m), dim3(256), 0, (hipStream_t) nullptr,
                       (const double *)p->D.p, p->ld, (const long long *)nullptr, m, a0, a1, bo.as<double>());
        if (e == hipSuccess) e = hipMemcpy(dist + a0 * m, bo.p, (size_t)((a1 - a0) * m) * 8, hipMemcpyDeviceToHost);
    }
    return bb::hip_status(who, e);
}

int bb_paths_place(const bb_paths *p, const double *coef, const double *mu, double *xyz, uint8_t *placed) {
    const char *who = "bb_paths_place";
    BB_REQUIRE(p != nullptr && coef != nullptr && mu != nullptr && xyz != nullptr && placed != nullptr,
               "bb_paths_place: NULL argument");
    BB_TRY(bb::enter_device(p->device));
    const int64_t n = p->n_nodes, L = p->n_sources;
    bb::DevBuf bc, bx, bp;                        // coef | mu, X, placed
    hipError_t e = bc.alloc((size_t)L * 32);
    if (e == hipSuccess) e = bx.alloc((size_t)n * 24);
    if (e == hipSuccess) e = bp.alloc((size_t)n);
    BB_TRY(bb::hip_status(who, e, BB_ERR_NOMEM));
    std::vector<double> x((size_t)n * 3);
    e = hipMemcpy(bc.p, coef, (size_t)L * 24, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(bc.as<double>() + 3 * L, mu, (size_t)L * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess)
        e = bb::launch(place_kernel, grid256(n), dim3(256), 0, (hipStream_t) nullptr, (const double *)p->D.p, n,
                       p->ld, L, (const double *)bc.p, (const double *)(bc.as<double>() + 3 * L),
                       bx.as<double>(), bp.as<unsigned char>());
    if (e == hipSuccess) e = hipMemcpy(placed, bp.p, (size_t)n, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(x.data(), bx.p, (size_t)n * 24, hipMemcpyDeviceToHost);
    BB_TRY(bb::hip_status(who, e));
    for (int64_t j = 0; j < n; ++j)               // (a row that is not placed stays as it was)
        if (placed[j])
            for (int c = 0; c < 3; ++c) xyz[3 * j + c] = x[(size_t)(3 * j + c)];
    return BB_OK;
}

int bb_paths_destroy(bb_paths *p) {
    if (!p) return BB_OK;
    (void)bb::enter_device(p->device);
    delete p;
    return BB_OK;
}

}  // extern "C"
