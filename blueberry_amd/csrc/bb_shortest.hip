// bb_shortest.hip -- completion of a resident ContactMap matrix by graph shortest paths
// (docs/SPEC.md 2.1.1): all-pairs shortest paths over the graph whose edges are the map's
// wish distances, by blocked Floyd-Warshall on a padded float64 work matrix in HBM.
//
// The graph is undirected, so the work matrix W (P x P, P = d rounded up to the tile edge 64) is
// symmetric and only its UPPER tiles (I <= J; diagonal tiles whole) are kept up to date: half
// the relaxations and half the traffic of the full matrix, and G_ij == G_ji bit for bit because
// the lower triangle of the result IS the upper one.
//
//   fw_load_kernel     resident (d, d) matrix -> upper tiles of W: counts -> wish by the rule of
//                      the solver's packers (bb_solver_kernels.h: finite and positive, then
//                      pow(v, -1/alpha) in double), +inf = no edge, padding +inf, diagonal 0.
//                      Only the upper triangle of the input is read, as the packers read it.
//   per round K (one 64-block of intermediate bins), three launches on one stream:
//     fw_diag_kernel   tile (K, K) closed in LDS by one workgroup (64 sequential steps)
//     fw_panel_kernel  row panel K, every J != K: R_J = min(R_J, (K, K) (x) R_J), where R_J is
//                      tile (K, J) for J > K and the transpose of tile (J, K) for J < K; the
//                      result goes back into that tile and, row-major, into the panel buffer
//     fw_tiles_kernel  every upper tile (I, J), I != K != J: C = min(C, R_I^T (x) R_J), both
//                      operands from the panel buffer (12.8 MB at d = 24,926: it stays in cache)
//   fw_store_kernel    W -> destination matrix, both triangles from the upper tiles, +inf -> 0
//                      ("no constraint"), counting the unreachable pairs i < j per row (summed on
//                      the host: no atomics).
//
// (x) is the min-plus product: v_add_f64 + v_min_f64 on the vector ALU; there is no matrix-core
// form of it.  Because the diagonal tile is closed before the panel uses it, a panel update is
// one min-plus product against the panel's OLD values -- no sequential dependence inside the
// tile, the same inner loop as the third phase.  A diagonal tile (I, I) of the third phase takes
// R_I for both operands: its cells (i, j) and (j, i) are the same sums in the same order (float
// addition commutes), so it stays symmetric.  Sizes and the traffic / ALU arithmetic:
// DESIGN.md 4.14.
#include <math.h>

#include <algorithm>
#include <string>
#include <vector>

#include "bb_cm_internal.h"
#include "bb_common.h"

namespace {

constexpr int kFT = 64;                    // tile edge = k-depth of a round
constexpr double kInf = __builtin_inf();
typedef double f64x2 __attribute__((ext_vector_type(2)));

__global__ __launch_bounds__(256) void fw_load_kernel(const double *__restrict__ m, int64_t d,
                                                      double *__restrict__ w, int64_t ld, int kind,
                                                      double neg_inv_alpha) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= ld) return;
    for (int64_t i = blockIdx.y; i < ld; i += gridDim.y) {
        if (i / kFT > j / kFT) continue;               // a lower tile: never read
        double v = kInf;
        if (i == j) {
            v = 0.0;
        } else if (i < d && j < d) {
            const double c = i < j ? m[i * d + j] : m[j * d + i];
            if ((c > 0.0) && (c <= 1.7976931348623157e308)) {      // finite, positive
                const double e = kind == BB_KIND_COUNTS ? pow(c, neg_inv_alpha) : c;
                if ((e > 0.0) && (e <= 1.7976931348623157e308)) v = e;
            }
        }
        w[i * ld + j] = v;
    }
}

// Tile (K, K): the classic in-place recurrence, one barrier per step.  Step k leaves row k and
// column k as they are (D[k][k] = 0 and no entry is negative), so nobody reads a cell another
// thread writes in the same step; D symmetric before a step is symmetric after it.
__global__ __launch_bounds__(256) void fw_diag_kernel(double *__restrict__ w, int64_t ld, int K) {
    __shared__ double D[kFT * kFT];
    double *t = w + ((int64_t)K * kFT) * ld + (int64_t)K * kFT;
    const int col = threadIdx.x & 63, r0 = threadIdx.x >> 6;
#pragma unroll
    for (int q = 0; q < 16; ++q) D[(r0 + 4 * q) * kFT + col] = t[(int64_t)(r0 + 4 * q) * ld + col];
    __syncthreads();
    for (int k = 0; k < kFT; ++k) {
        const double dk = D[k * kFT + col];
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int row = r0 + 4 * q;
            D[row * kFT + col] = __builtin_fmin(D[row * kFT + col], D[row * kFT + k] + dk);
        }
        __syncthreads();
    }
#pragma unroll
    for (int q = 0; q < 16; ++q) t[(int64_t)(r0 + 4 * q) * ld + col] = D[(r0 + 4 * q) * kFT + col];
}

// The inner loop of phases 2 and 3: c = min(c, A^T (x) B) for one 64 x 64 tile per workgroup of
// 256 threads over KS values of k.  Ra[k][i] and Rb[k][j] are staged in LDS and a thread keeps a 4 x 4 block of C in registers: rows {2 ty, 2 ty + 1, 32 + 2 ty, 33 + 2 ty},
// columns the same of tx.  Per k a thread reads its four A and four B values as four 16-byte LDS
// reads, for 16 adds and 16 mins.  The 16 tx of a lane group read 16 consecutive 16-byte slots
// (all 64 banks once), lanes of equal tx or ty the same address (broadcast): no bank conflict.
template <int KS = kFT>
__device__ __forceinline__ void minplus_tile(double (&c)[4][4], const double *Ra, const double *Rb,
                                             int tx, int ty) {
#pragma unroll 8
    for (int k = 0; k < KS; ++k) {
        const f64x2 a01 = *reinterpret_cast<const f64x2 *>(&Ra[k * kFT + 2 * ty]);
        const f64x2 a23 = *reinterpret_cast<const f64x2 *>(&Ra[k * kFT + 32 + 2 * ty]);
        const f64x2 b01 = *reinterpret_cast<const f64x2 *>(&Rb[k * kFT + 2 * tx]);
        const f64x2 b23 = *reinterpret_cast<const f64x2 *>(&Rb[k * kFT + 32 + 2 * tx]);
        const double a[4] = {a01.x, a01.y, a23.x, a23.y}, b[4] = {b01.x, b01.y, b23.x, b23.y};
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int s = 0; s < 4; ++s) c[r][s] = __builtin_fmin(c[r][s], a[r] + b[s]);
    }
}

// a thread's 4 x 4 block <-> a row-major tile with leading dimension ld (global or LDS)
__device__ __forceinline__ void block_load(double (&c)[4][4], const double *t, int64_t ld, int tx, int ty) {
    const int ri[4] = {2 * ty, 2 * ty + 1, 32 + 2 * ty, 33 + 2 * ty};
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const f64x2 lo = *reinterpret_cast<const f64x2 *>(t + ri[r] * ld + 2 * tx);
        const f64x2 hi = *reinterpret_cast<const f64x2 *>(t + ri[r] * ld + 32 + 2 * tx);
        c[r][0] = lo.x; c[r][1] = lo.y; c[r][2] = hi.x; c[r][3] = hi.y;
    }
}
__device__ __forceinline__ void block_store(const double (&c)[4][4], double *t, int64_t ld, int tx, int ty) {
    const int ri[4] = {2 * ty, 2 * ty + 1, 32 + 2 * ty, 33 + 2 * ty};
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        *reinterpret_cast<f64x2 *>(t + ri[r] * ld + 2 * tx) = f64x2{c[r][0], c[r][1]};
        *reinterpret_cast<f64x2 *>(t + ri[r] * ld + 32 + 2 * tx) = f64x2{c[r][2], c[r][3]};
    }
}

// Phase 2, one workgroup per tile J != K of row panel K.  A = the closed diagonal tile
// (symmetric: D^T = D).  B = C's start = the panel tile's old values: tile (K, J) as it is for
// J > K, tile (J, K) transposed on its way into LDS for J < K (the lower tiles are not kept).
// The result goes to panel[J] (64 x 64, row-major, contiguous) for the third phase and back
// into the matrix: rows of (K, J), or, transposed through LDS, rows of (J, K).
__global__ __launch_bounds__(256, 2) void fw_panel_kernel(double *__restrict__ w, int64_t ld, int K,
                                                          double *__restrict__ panel) {
    const int J = blockIdx.x;
    if (J == K) return;
    __shared__ __attribute__((aligned(16))) double Ra[kFT * kFT];
    __shared__ __attribute__((aligned(16))) double Rb[kFT * kFT];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const bool upper = J > K;
    const double *pd = w + ((int64_t)K * kFT) * ld + (int64_t)K * kFT;
    double *pt = upper ? w + ((int64_t)K * kFT) * ld + (int64_t)J * kFT
                       : w + ((int64_t)J * kFT) * ld + (int64_t)K * kFT;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int e = q * 256 + tid, row = e >> 5, c2 = (e & 31) * 2;
        *reinterpret_cast<f64x2 *>(&Ra[row * kFT + c2]) =
            *reinterpret_cast<const f64x2 *>(pd + (int64_t)row * ld + c2);
        const f64x2 v = *reinterpret_cast<const f64x2 *>(pt + (int64_t)row * ld + c2);
        if (upper) {
            *reinterpret_cast<f64x2 *>(&Rb[row * kFT + c2]) = v;
        } else {
            Rb[c2 * kFT + row] = v.x;
            Rb[(c2 + 1) * kFT + row] = v.y;
        }
    }
    __syncthreads();
    double c[4][4];
    block_load(c, Rb, kFT, tx, ty);
    minplus_tile(c, Ra, Rb, tx, ty);
    block_store(c, panel + (int64_t)J * (kFT * kFT), kFT, tx, ty);
    if (upper) {
        block_store(c, pt, ld, tx, ty);
        return;
    }
    // Rb <- C^T, then row-contiguous stores into tile (J, K)
    __syncthreads();                       // everybody is done reading Ra / Rb
    const int ri[2] = {2 * ty, 32 + 2 * ty}, cj[4] = {2 * tx, 2 * tx + 1, 32 + 2 * tx, 33 + 2 * tx};
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        *reinterpret_cast<f64x2 *>(&Rb[cj[s] * kFT + ri[0]]) = f64x2{c[0][s], c[1][s]};
        *reinterpret_cast<f64x2 *>(&Rb[cj[s] * kFT + ri[1]]) = f64x2{c[2][s], c[3][s]};
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int e = q * 256 + tid, row = e >> 5, c2 = (e & 31) * 2;
        *reinterpret_cast<f64x2 *>(pt + (int64_t)row * ld + c2) =
            *reinterpret_cast<const f64x2 *>(&Rb[row * kFT + c2]);
    }
}

// Phase 3, one workgroup per upper tile (I, J), I <= J: blockIdx.x = J (J + 1) / 2 + I, so that
// consecutive workgroups share their B operand.  Tiles of row or column block K are phase 2's.
__global__ __launch_bounds__(256, 4) void fw_tiles_kernel(double *__restrict__ w, int64_t ld, int K,
                                                          const double *__restrict__ panel) {
    const unsigned b = blockIdx.x;
    int J = (int)((__builtin_sqrt(8.0 * (double)b + 1.0) - 1.0) * 0.5);
    while ((unsigned)J * (unsigned)(J + 1) / 2 > b) --J;
    while ((unsigned)(J + 1) * (unsigned)(J + 2) / 2 <= b) ++J;
    const int I = (int)(b - (unsigned)J * (unsigned)(J + 1) / 2);
    if (I == K || J == K) return;
    // the operands go through LDS in two halves of 32 k (2 x 16 KiB per workgroup): four
    // workgroups per CU = four waves per SIMD instead of two
    constexpr int KS = kFT / 2;
    __shared__ __attribute__((aligned(16))) double Ra[KS * kFT];
    __shared__ __attribute__((aligned(16))) double Rb[KS * kFT];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    double *pc = w + ((int64_t)I * kFT) * ld + (int64_t)J * kFT;
    double c[4][4];
    block_load(c, pc, ld, tx, ty);
    const double *pa = panel + (int64_t)I * (kFT * kFT), *pb = panel + (int64_t)J * (kFT * kFT);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        if (h) __syncthreads();                // everybody is done with the first half
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int e = (q * 256 + tid) * 2;
            *reinterpret_cast<f64x2 *>(&Ra[e]) = *reinterpret_cast<const f64x2 *>(pa + h * (KS * kFT) + e);
            *reinterpret_cast<f64x2 *>(&Rb[e]) = *reinterpret_cast<const f64x2 *>(pb + h * (KS * kFT) + e);
        }
        __syncthreads();
        minplus_tile<KS>(c, Ra, Rb, tx, ty);
    }
    block_store(c, pc, ld, tx, ty);
}

// Row i of the result -> row i of the (d, d) destination, the cells left of i's diagonal tile
// from the transposed upper tile; counts[i] = unreachable pairs (i, j), j > i.
__global__ __launch_bounds__(256) void fw_store_kernel(const double *__restrict__ w, int64_t ld,
                                                       double *__restrict__ out, int64_t d,
                                                       int64_t *__restrict__ counts) {
    __shared__ int part[256];
    const int64_t i = blockIdx.x, j0 = i / kFT * kFT;
    int n = 0;
    for (int64_t j = threadIdx.x; j < d; j += 256) {
        const double v = j >= j0 ? w[i * ld + j] : w[j * ld + i];
        const bool none = !(v <= 1.7976931348623157e308);
        out[i * d + j] = none ? 0.0 : v;
        n += (none && j > i) ? 1 : 0;
    }
    n = bb::block_sum<256>(n, part);
    if (threadIdx.x == 0) counts[i] = n;
}

}  // namespace

extern "C" int bb_cm_shortest_paths(const bb_cm *src, bb_cm *dst, int kind, double alpha,
                                    int64_t *unreachable_pairs) {
    BB_REQUIRE(src != nullptr && dst != nullptr, "bb_cm_shortest_paths: contact map is NULL");
    BB_REQUIRE(kind == BB_KIND_WISH || kind == BB_KIND_COUNTS,
               "bb_cm_shortest_paths: kind must be BB_KIND_WISH or BB_KIND_COUNTS");
    BB_REQUIRE(alpha > 0.0, "bb_cm_shortest_paths: alpha must be positive");
    BB_REQUIRE(src->d == dst->d, "bb_cm_shortest_paths: src and dst differ in their edge");
    BB_REQUIRE(src->device == dst->device, "bb_cm_shortest_paths: src and dst live on different devices");
    BB_REQUIRE(src->d >= 1, "bb_cm_shortest_paths: the contact map is empty");
    BB_TRY(bb::enter_device(src->device));
    const int64_t d = src->d, ld = bb::round_up(d, kFT);
    const int nt = (int)(ld / kFT);
    BB_REQUIRE(nt <= 65535, "bb_cm_shortest_paths: matrix too large for one launch grid");
    // work matrix | row panel of the round (nt tiles of 64 x 64) | per-row counts
    const size_t w_bytes = (size_t)ld * (size_t)ld * 8, panel_bytes = (size_t)ld * kFT * 8;
    const size_t need = w_bytes + panel_bytes + (size_t)d * 8;
    bb::CmScratch *scr = bb::per_device<bb::CmScratch>(src->device);
    std::lock_guard<std::mutex> scratch_lock(scr->mu);
    hipError_t e = scr->buf.reserve(need);
    if (e != hipSuccess)
        return bb::fail(BB_ERR_NOMEM,
                        "bb_cm_shortest_paths: cannot allocate the work matrix: " +
                            std::to_string(need) + " bytes (edge " + std::to_string(d) +
                            " padded to " + std::to_string(ld) + ") beside the resident matrix of " +
                            std::to_string((size_t)d * (size_t)d * 8) + " bytes: " +
                            hipGetErrorString(e));
    double *w = (double *)scr->buf.p, *panel = w + ld * ld;
    int64_t *counts = (int64_t *)(panel + ld * kFT);
    hipStream_t st = src->stream;
    e = bb::launch(fw_load_kernel, dim3((unsigned)((ld + 255) / 256), (unsigned)std::min<int64_t>(ld, 65535)), dim3(256),
                   0, st, (const double *)src->m, d, w, ld, kind, -1.0 / alpha);
    for (int K = 0; K < nt && e == hipSuccess; ++K) {
        e = bb::launch(fw_diag_kernel, dim3(1), dim3(256), 0, st, w, ld, K);
        if (nt == 1) break;
        if (e == hipSuccess)
            e = bb::launch(fw_panel_kernel, dim3((unsigned)nt), dim3(256), 0, st, w, ld, K, panel);
        if (e == hipSuccess)
            e = bb::launch(fw_tiles_kernel, dim3((unsigned)nt * (unsigned)(nt + 1) / 2), dim3(256), 0, st,
                           w, ld, K, (const double *)panel);
    }
    if (e == hipSuccess)
        e = bb::launch(fw_store_kernel, dim3((unsigned)d), dim3(256), 0, st, (const double *)w, ld,
                       dst->m, d, counts);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    std::vector<int64_t> host;
    if (e == hipSuccess && unreachable_pairs) {
        host.resize((size_t)d);
        e = hipMemcpy(host.data(), counts, (size_t)d * 8, hipMemcpyDeviceToHost);
    }
    BB_TRY(bb::hip_status("bb_cm_shortest_paths", e));
    if (unreachable_pairs) {
        int64_t total = 0;
        for (int64_t v : host) total += v;
        *unreachable_pairs = total;
    }
    return BB_OK;
}
