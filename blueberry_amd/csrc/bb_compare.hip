// bb_compare.hip -- comparing two structures (docs/SPEC.md 2.10): the moments
// a superposition needs, and -- for a transform the host made from them -- the aligned copy, its
// per-bin deviation, seven float64 sums per separation k = j - i and two per bin over the pairs of
// used bins, and on request the sums of products of the centred average ranks of the two lists of
// pair distances (Spearman).  Handle-less: host arrays in, host arrays out.  gfx950 only.
//
// All arithmetic is float64, no floating-point atomics, every sum in an order fixed by n and the
// used vector alone:
//   cmp_sum_kernel / cmp_centred_kernel   per workgroup of 1,024 bins the 7 sums (count, A, B), then
//                         the 11 centred sums (EA, EB, H); cmp_reduce_kernel adds the workgroups'
//                         partials, a thread every 256th, then the wave butterfly and the 4 waves
//   cmp_transform_kernel  aligned = s R B + t and |A - aligned|^2 per bin (NaN at unused bins)
//   cmp_pairs_kernel      one workgroup per CHUNK: consecutive tiles (I, I + D) of ONE tile
//                         difference D, kT = 256 bins a side; both structures' row and column
//                         strips sit in LDS, a thread owns the tile-relative diagonals t and t + 256
//                         and keeps their seven sums in registers over the whole chunk
//   cmp_fold_kernel       profile[k][col] = the chunks' sums of diagonal k, in chunk order
//   cmp_bins_kernel       a wave owns 4 bins, a workgroup 16; the other bins pass through LDS 256
//                         at a time (the pair math a second time: it is cheap, the slots are not)
//   cmp_key_kernel, bb::stable_sort_pairs, cmp_rank_kernel, cmp_rank_sum_kernel
//                         the distances of one structure as sort keys in canonical pair order, the
//                         library's stable radix sort with the pair's place as payload, the run of
//                         equal keys around every sorted slot by two bounded binary searches (at
//                         most 32 probes each, whatever the run's length), the centred average rank
//                         scattered back to pair order; then the other structure through the same
//                         buffers, and the three sums over pair order
//
// Slot memory of a call: a chunk holds at most ceil(nb / 16) tiles, nb = ceil(n / 256), so there
// are at most 9 nb + 8 chunks of (2 kT - 1) * 7 * 8 = 28,616 B: under 1,007 B per bin + 0.5 MB
// (293 MB at n = 309,568; a slot per tile would be 21 GB there).  Beside it 153 B per bin of
// inputs and results.  Ranks: 40 B per pair (two key and two place buffers of the sort, 8 + 8 + 4
// + 4, and the two lists of centred ranks, 8 + 8), 172 GB at the 2^32 - 1 pairs the places' 32
// bits allow.  Everything is allocated for the call and released with it.
#include <cmath>
#include <vector>

#include "bb_common.h"
#include "bb_device_sums.h"
#include "bb_sort.h"

namespace {

constexpr int kT = 256, kNO = 2 * kT - 1;        // tile edge of the pair pass, diagonals of a tile
constexpr int kProfileCols = 7, kBinCols = 2;
constexpr int kChunkSplit = 16;                  // a tile difference's tiles go to about this many chunks
constexpr int kBinsPerWave = 4, kBinsPerBlock = 4 * kBinsPerWave;
constexpr int kMomentBins = 1024;                // bins per workgroup of the moment kernels
constexpr int64_t kRankBlocks = 2048;            // most workgroups of cmp_rank_sum_kernel

// |x_i - x_j| in float64, the rule of bb_score.hip: products and sums rounded one by one,
// ((dx^2 + dy^2) + dz^2), and a correctly rounded root.
__device__ __forceinline__ double pair_distance(double xi, double yi, double zi, double xj, double yj,
                                                double zj) {
#pragma clang fp contract(off)
    const double dx = xi - xj, dy = yi - yj, dz = zi - zj;
    return sqrt((dx * dx + dy * dy) + dz * dz);
}

__device__ __forceinline__ void add_pair(double (&a)[kProfileCols], double da, double db) {
#pragma clang fp contract(off)
    const double res = da - db;
    a[0] += 1.0;
    a[1] += da;
    a[2] += db;
    a[3] += da * da;
    a[4] += db * db;
    a[5] += da * db;
    a[6] += res * res;
}

// partials[g][q] = over the used bins of workgroup g's 1,024: the count, sum A (3), sum B (3)
__global__ __launch_bounds__(256) void cmp_sum_kernel(const double *__restrict__ a,
                                                      const double *__restrict__ b,
                                                      const uint8_t *__restrict__ use, int64_t n,
                                                      double *__restrict__ partials) {
    __shared__ double sh[7][4];
    double v[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int r = 0; r < kMomentBins / 256; ++r) {
        const int64_t i = (int64_t)blockIdx.x * kMomentBins + r * 256 + threadIdx.x;
        if (i < n && use[i]) {
            v[0] += 1.0;
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                v[1 + q] += a[3 * i + q];
                v[4 + q] += b[3 * i + q];
            }
        }
    }
    bb::block_sums_all(v, sh);
    if (threadIdx.x < 7) partials[(int64_t)blockIdx.x * 7 + threadIdx.x] = v[threadIdx.x];
}

// partials[g][q] = over the same bins: EA, EB and H row-major, H[p][q] = sum (B - cB)_p (A - cA)_q;
// mean: the count, cA, cB (cmp_reduce_kernel's output of the first pass)
__global__ __launch_bounds__(256) void cmp_centred_kernel(const double *__restrict__ a,
                                                          const double *__restrict__ b,
                                                          const uint8_t *__restrict__ use, int64_t n,
                                                          const double *__restrict__ mean,
                                                          double *__restrict__ partials) {
#pragma clang fp contract(off)
    __shared__ double sh[11][4];
    double v[11];
#pragma unroll
    for (int q = 0; q < 11; ++q) v[q] = 0.0;
    for (int r = 0; r < kMomentBins / 256; ++r) {
        const int64_t i = (int64_t)blockIdx.x * kMomentBins + r * 256 + threadIdx.x;
        if (i < n && use[i]) {
            double da[3], db[3];
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                da[q] = a[3 * i + q] - mean[1 + q];
                db[q] = b[3 * i + q] - mean[4 + q];
            }
            v[0] += (da[0] * da[0] + da[1] * da[1]) + da[2] * da[2];
            v[1] += (db[0] * db[0] + db[1] * db[1]) + db[2] * db[2];
#pragma unroll
            for (int p = 0; p < 3; ++p)
#pragma unroll
                for (int q = 0; q < 3; ++q) v[2 + 3 * p + q] += db[p] * da[q];
        }
    }
    bb::block_sums_all(v, sh);
    if (threadIdx.x < 11) partials[(int64_t)blockIdx.x * 11 + threadIdx.x] = v[threadIdx.x];
}

// out[q] = the sum of partials[g][q] over g: thread t adds g = t, t + 256, ..., then the
// workgroup's fixed sum.  One workgroup.  as_mean: out[q] = sum_q / sum_0 for q > 0.
template <int Q>
__global__ __launch_bounds__(256) void cmp_reduce_kernel(const double *__restrict__ partials, int64_t n_parts,
                                                         int as_mean, double *__restrict__ out) {
    __shared__ double sh[Q][4];
    double v[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) v[q] = 0.0;
    for (int64_t g = threadIdx.x; g < n_parts; g += 256)
#pragma unroll
        for (int q = 0; q < Q; ++q) v[q] += partials[g * Q + q];
    bb::block_sums_all(v, sh);
    if (threadIdx.x == 0)
#pragma unroll
        for (int q = 0; q < Q; ++q) out[q] = (as_mean && q > 0) ? v[q] / v[0] : v[q];
}

// aligned_i = ((R[p][0] x + R[p][1] y) + R[p][2] z) s + t[p], each step rounded; dev2[i] =
// ((ex^2 + ey^2) + ez^2) of e = A_i - aligned_i.  Unused bins: NaN in both.  tr: R, t, s.
__global__ __launch_bounds__(256) void cmp_transform_kernel(const double *__restrict__ a,
                                                            const double *__restrict__ b,
                                                            const uint8_t *__restrict__ use, int64_t n,
                                                            const double *__restrict__ tr,
                                                            double *__restrict__ aligned,
                                                            double *__restrict__ dev2) {
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    if (!use[i]) {
        aligned[3 * i] = aligned[3 * i + 1] = aligned[3 * i + 2] = dev2[i] = nan;
        return;
    }
    const double x = b[3 * i], y = b[3 * i + 1], z = b[3 * i + 2], s = tr[12];
    double e[3];
#pragma unroll
    for (int p = 0; p < 3; ++p) {
        const double w = ((tr[3 * p] * x + tr[3 * p + 1] * y) + tr[3 * p + 2] * z) * s + tr[9 + p];
        aligned[3 * i + p] = w;
        e[p] = a[3 * i + p] - w;
    }
    dev2[i] = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2];
}

// Row r of a tile for thread t: its one column c = (t + r + 1) mod kT, added to the sums of
// diagonal t + 256 (SIDE 1), of diagonal t (SIDE 0), or of whichever holds it (SIDE -1).
template <int SIDE>
__device__ __forceinline__ void pair_row(double (&acc)[2][kProfileCols], const double (&rows)[6][kT],
                                         const double (&cols)[6][kT], const uint8_t (&row_use)[kT],
                                         const uint8_t (&col_use)[kT], int t, int r, int ahead) {
    if (!row_use[r]) return;                         // (the same for every thread)
    const int c = (t + r + 1) & (kT - 1);
    if (!col_use[c] || ahead + c <= r) return;
    const double da = pair_distance(rows[0][r], rows[1][r], rows[2][r], cols[0][c], cols[1][c], cols[2][c]);
    const double db = pair_distance(rows[3][r], rows[4][r], rows[5][r], cols[3][c], cols[4][c], cols[5][c]);
    if (SIDE >= 0) {
        add_pair(acc[SIDE < 0 ? 0 : SIDE], da, db);
    } else {                                         // (x + 0.0 = x: no sum here is negative)
        double term[kProfileCols] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        add_pair(term, da, db);
        const bool upper = t + r + 1 < kT;
#pragma unroll
        for (int q = 0; q < kProfileCols; ++q) {
            acc[1][q] += upper ? term[q] : 0.0;
            acc[0][q] += upper ? 0.0 : term[q];
        }
    }
}

// chunks[c] = {D, I_begin, I_end, 0}: the tiles (I, I + D), I_begin <= I < I_end.  In a tile the
// row strip is the bins I kT + r and the column strip (I + D) kT + c; thread t owns the diagonals
// o = t + 256 m, o = c - r + kT - 1 in [0, 2 kT - 2], so in row r consecutive threads take
// consecutive columns and every pair of the tile has exactly one owner.  A strip holds zeros and
// use = 0 for bins that are unused or past n.  slots: (7, 2 kT - 1) doubles per chunk.
__global__ __launch_bounds__(256) void cmp_pairs_kernel(const double *__restrict__ a,
                                                        const double *__restrict__ al,
                                                        const uint8_t *__restrict__ use, int64_t n,
                                                        const int4 *__restrict__ chunks,
                                                        double *__restrict__ slots) {
    constexpr int OPT = 2;
    static_assert(kT == 256, "a thread per column, two diagonals per thread");
    __shared__ double rows[6][kT], cols[6][kT];      // x, y, z of A, then of the aligned B
    __shared__ uint8_t row_use[kT], col_use[kT];
    const int4 ch = chunks[blockIdx.x];
    const int t = threadIdx.x;
    double acc[OPT][kProfileCols];
#pragma unroll
    for (int m = 0; m < OPT; ++m)
#pragma unroll
        for (int q = 0; q < kProfileCols; ++q) acc[m][q] = 0.0;

    for (int I = ch.y; I < ch.z; ++I) {
        const int64_t i0 = (int64_t)I * kT, j0 = (int64_t)(I + ch.x) * kT;
        __syncthreads();                             // (the tile before has been read)
        {
            const int64_t i = i0 + t, j = j0 + t;
            const bool ui = i < n && use[i], uj = j < n && use[j];
            row_use[t] = ui, col_use[t] = uj;
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                rows[q][t] = ui ? a[3 * i + q] : 0.0;
                rows[3 + q][t] = ui ? al[3 * i + q] : 0.0;
                cols[q][t] = uj ? a[3 * j + q] : 0.0;
                cols[3 + q][t] = uj ? al[3 * j + q] : 0.0;
            }
        }
        __syncthreads();
        // In row r a thread's two diagonals hold ONE column between them: c = (t + r + 1) mod kT,
        // on diagonal t + 256 while t + r + 1 < kT and on diagonal t from there on.  For the 64
        // threads of a wave the change falls within 64 rows; in the other 192 the whole wave is
        // on one side.  Either set of sums gets its rows in ascending order, whatever the split.
        const int ahead = ch.x * kT;                 // j0 - i0
        const int mixed = kT - 64 * ((t >> 6) + 1);  // the wave's first row with threads on both sides
        int r = 0;
        for (; r < mixed; ++r) pair_row<1>(acc, rows, cols, row_use, col_use, t, r, ahead);
        for (; r < mixed + 64; ++r) pair_row<-1>(acc, rows, cols, row_use, col_use, t, r, ahead);
        for (; r < kT; ++r) pair_row<0>(acc, rows, cols, row_use, col_use, t, r, ahead);
    }
    double *slot = slots + (int64_t)blockIdx.x * (kProfileCols * kNO);
#pragma unroll
    for (int m = 0; m < OPT; ++m) {
        const int o = t + 256 * m;
        if (o < kNO)
#pragma unroll
            for (int q = 0; q < kProfileCols; ++q) slot[q * kNO + o] = acc[m][q];
    }
}

// profile[k][col] = the sum over the chunks that hold diagonal k, in chunk order.  A chunk of tile
// difference D holds k at o = k - D kT + kT - 1, so only D in {k / kT, k / kT + 1} can:
// chunk_ptr[D] .. chunk_ptr[D + 1] are the chunks of D (they are listed by D).
__global__ __launch_bounds__(256) void cmp_fold_kernel(const double *__restrict__ slots,
                                                       const int *__restrict__ chunk_ptr, int n_blocks,
                                                       int64_t n, double *__restrict__ profile) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int col = blockIdx.y;
    if (k >= n) return;
    double s = 0.0;
    if (k > 0) {
        const int q = (int)(k / kT);
        for (int D = q; D <= q + 1 && D < n_blocks; ++D) {
            const int o = (int)(k - (int64_t)D * kT) + kT - 1;
            if (o < 0) continue;
            for (int p = chunk_ptr[D]; p < chunk_ptr[D + 1]; ++p)
                s += slots[(int64_t)p * (kProfileCols * kNO) + col * kNO + o];
        }
    }
    profile[k * kProfileCols + col] = s;
}

// Per bin i: its pairs and sum (dA - dB)^2 over the other used bins.  A wave owns the bins
// 16 blockIdx + 4 wave + {0..3}; the bins j pass through LDS 256 at a time, lane l taking
// j = 64 q + l of each batch for its wave's four bins; then the wave butterfly.
__global__ __launch_bounds__(256) void cmp_bins_kernel(const double *__restrict__ a,
                                                       const double *__restrict__ al,
                                                       const uint8_t *__restrict__ use, int64_t n,
                                                       double *__restrict__ bins) {
#pragma clang fp contract(off)
    __shared__ double cols[6][256];
    __shared__ uint8_t col_use[256];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int64_t first = (int64_t)blockIdx.x * kBinsPerBlock + wave * kBinsPerWave;
    double xa[kBinsPerWave][3], xb[kBinsPerWave][3], cnt[kBinsPerWave], sq[kBinsPerWave];
    bool on[kBinsPerWave];
#pragma unroll
    for (int w = 0; w < kBinsPerWave; ++w) {
        const int64_t i = first + w;
        on[w] = i < n && use[i];
        cnt[w] = sq[w] = 0.0;
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            xa[w][q] = on[w] ? a[3 * i + q] : 0.0;
            xb[w][q] = on[w] ? al[3 * i + q] : 0.0;
        }
    }
    for (int64_t j0 = 0; j0 < n; j0 += 256) {
        __syncthreads();
        {
            const int64_t j = j0 + t;
            const bool uj = j < n && use[j];
            col_use[t] = uj;
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                cols[q][t] = uj ? a[3 * j + q] : 0.0;
                cols[3 + q][t] = uj ? al[3 * j + q] : 0.0;
            }
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int c = 64 * q + lane;
            if (!col_use[c]) continue;
            const double ax = cols[0][c], ay = cols[1][c], az = cols[2][c];
            const double bx = cols[3][c], by = cols[4][c], bz = cols[5][c];
#pragma unroll
            for (int w = 0; w < kBinsPerWave; ++w)
                if (on[w] && j0 + c != first + w) {
                    const double res = pair_distance(xa[w][0], xa[w][1], xa[w][2], ax, ay, az) -
                                       pair_distance(xb[w][0], xb[w][1], xb[w][2], bx, by, bz);
                    cnt[w] += 1.0;
                    sq[w] += res * res;
                }
        }
    }
#pragma unroll
    for (int w = 0; w < kBinsPerWave; ++w) {
        const double c = bb::wave_sum_all(cnt[w]), s = bb::wave_sum_all(sq[w]);
        if (lane == 0 && first + w < n) {
            bins[(first + w) * kBinCols] = c;
            bins[(first + w) * kBinCols + 1] = s;
        }
    }
}

// Canonical pair order over the used bins idx[0] < idx[1] < ...: pair (u, v), u < v, has place
// u (2 nu - u - 1) / 2 + (v - u - 1).  One workgroup per u.  keys: the distance in structure xyz
// as the sort's order-preserving key; place: the pair's place.
__global__ __launch_bounds__(256) void cmp_key_kernel(const double *__restrict__ xyz,
                                                      const uint32_t *__restrict__ idx, int64_t nu,
                                                      bb::sort_key *__restrict__ keys,
                                                      uint32_t *__restrict__ place) {
    const int64_t u = blockIdx.x;
    const int64_t base = u * (2 * nu - u - 1) / 2 - u - 1;      // + v = the place
    const int64_t i = idx[u];
    const double xi = xyz[3 * i], yi = xyz[3 * i + 1], zi = xyz[3 * i + 2];
    for (int64_t v = u + 1 + threadIdx.x; v < nu; v += 256) {
        const int64_t j = idx[v];
        keys[base + v] = bb::order_key(pair_distance(xi, yi, zi, xyz[3 * j], xyz[3 * j + 1], xyz[3 * j + 2]));
        place[base + v] = (uint32_t)(base + v);
    }
}

// keys sorted: slot s lies in the run [lo, hi) of its key, whose average rank (1-based) is
// (lo + hi + 1) / 2; centred by (m + 1) / 2 that is (lo + hi - m) / 2, an exact half-integer.
// The run's ends are looked at next door first and else found by binary search: at most 32
// probes each.
__global__ __launch_bounds__(256) void cmp_rank_kernel(const bb::sort_key *__restrict__ keys,
                                                       const uint32_t *__restrict__ place, int64_t m,
                                                       double *__restrict__ rank) {
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= m) return;
    const bb::sort_key k = keys[s];
    int64_t lo = s, hi = s + 1;
    if (s > 0 && keys[s - 1] == k) {                 // the first slot of [0, s - 1] that holds k
        int64_t l = 0, h = s - 1;
        while (l < h) {
            const int64_t mid = (l + h) >> 1;
            if (keys[mid] < k) l = mid + 1;
            else h = mid;
        }
        lo = l;
    }
    if (s + 1 < m && keys[s + 1] == k) {             // the first slot of [s + 2, m] above k
        int64_t l = s + 2, h = m;
        while (l < h) {
            const int64_t mid = (l + h) >> 1;
            if (keys[mid] > k) h = mid;
            else l = mid + 1;
        }
        hi = l;
    }
    rank[place[s]] = 0.5 * (double)(lo + hi - m);
}

// partials[g] = sum rA^2, sum rB^2, sum rA rB over the places [g per, (g + 1) per), per a multiple
// of 256: thread t takes every 256th place from t.
__global__ __launch_bounds__(256) void cmp_rank_sum_kernel(const double *__restrict__ ra,
                                                           const double *__restrict__ rb, int64_t m,
                                                           int64_t per, double *__restrict__ partials) {
#pragma clang fp contract(off)
    __shared__ double sh[3][4];
    double v[3] = {0.0, 0.0, 0.0};
    const int64_t begin = (int64_t)blockIdx.x * per, end = begin + per < m ? begin + per : m;
    for (int64_t p = begin + threadIdx.x; p < end; p += 256) {
        const double x = ra[p], y = rb[p];
        v[0] += x * x;
        v[1] += y * y;
        v[2] += x * y;
    }
    bb::block_sums_all(v, sh);
    if (threadIdx.x < 3) partials[(int64_t)blockIdx.x * 3 + threadIdx.x] = v[threadIdx.x];
}

// use_eff[i] = (use == NULL or use[i]) and the six coordinates of bin i are finite; returns how many
int64_t used_bins(const double *a, const double *b, const uint8_t *use, int64_t n, std::vector<uint8_t> &eff) {
    eff.assign((size_t)n, 0);
    int64_t nu = 0;
    for (int64_t i = 0; i < n; ++i) {
        bool ok = use == nullptr || use[i] != 0;
        for (int q = 0; q < 3 && ok; ++q) ok = std::isfinite(a[3 * i + q]) && std::isfinite(b[3 * i + q]);
        eff[(size_t)i] = ok;
        nu += ok;
    }
    return nu;
}

int alloc_named(const char *who, bb::DevBuf &buf, size_t bytes) {
    const hipError_t e = buf.alloc(bytes);
    if (e == hipSuccess) return BB_OK;
    return bb::fail(BB_ERR_NOMEM, std::string(who) + ": hipMalloc of " + std::to_string(bytes) +
                                      " bytes failed: " + hipGetErrorString(e));
}

// A stream of the device's pool for the length of a call.
struct CallStream {
    int device;
    hipStream_t st = nullptr;
    explicit CallStream(int d) : device(d) {}
    ~CallStream() {
        if (st) bb::release_stream(device, st);
    }
};

// The ranks of the distances in structure xyz, centred, in pair order (into rank).
int rank_pass(const char *who, const double *xyz, const uint32_t *idx, int64_t nu, int64_t m,
              bb::sort_key *ka, bb::sort_key *kb, uint32_t *pa, uint32_t *pb, double *rank, hipStream_t st) {
    BB_HIP_CHECK(bb::launch(cmp_key_kernel, dim3((unsigned)(nu - 1)), dim3(256), 0, st, xyz, idx, nu, ka, pa));
    const hipError_t e = bb::stable_sort_pairs<uint32_t>(ka, pa, kb, pb, m, 64, st);
    if (e != hipSuccess) return bb::hip_status(who, e, e == hipErrorOutOfMemory ? BB_ERR_NOMEM : BB_ERR_HIP);
    BB_HIP_CHECK(bb::launch(cmp_rank_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st,
                            (const bb::sort_key *)ka, (const uint32_t *)pa, m, rank));
    return BB_OK;
}

}  // namespace

extern "C" {

int bb_structures_moments(const double *a, const double *b, const uint8_t *use, int64_t n, int device,
                          double *out18) {
    const char *who = "bb_structures_moments";
    BB_REQUIRE(a != nullptr && b != nullptr && out18 != nullptr, "bb_structures_moments: NULL argument");
    BB_REQUIRE(n >= 2 && n < ((int64_t)1 << 31), "bb_structures_moments: n must be in [2, 2^31)");
    std::vector<uint8_t> eff;
    used_bins(a, b, use, n, eff);
    BB_TRY(bb::use_device(device));
    CallStream cs(device);
    BB_TRY(bb::hip_status(who, bb::acquire_stream(device, &cs.st)));
    hipStream_t st = cs.st;

    const int64_t groups = (n + kMomentBins - 1) / kMomentBins;
    const size_t xyz_bytes = bb::align256((size_t)n * 24), use_bytes = bb::align256((size_t)n);
    const size_t part_bytes = bb::align256((size_t)groups * 11 * 8);
    bb::DevBuf buf;
    BB_TRY(alloc_named(who, buf, 2 * xyz_bytes + use_bytes + part_bytes + 256));
    char *p = buf.as<char>();
    double *d_a = (double *)p, *d_b = (double *)(p += xyz_bytes);
    uint8_t *d_use = (uint8_t *)(p += xyz_bytes);
    double *d_part = (double *)(p += use_bytes);
    double *d_out = (double *)(p += part_bytes);     // the count, cA, cB | EA, EB, H
    BB_HIP_CHECK(hipMemcpyAsync(d_a, a, (size_t)n * 24, hipMemcpyHostToDevice, st));
    BB_HIP_CHECK(hipMemcpyAsync(d_b, b, (size_t)n * 24, hipMemcpyHostToDevice, st));
    BB_HIP_CHECK(hipMemcpyAsync(d_use, eff.data(), (size_t)n, hipMemcpyHostToDevice, st));
    BB_HIP_CHECK(bb::launch(cmp_sum_kernel, dim3((unsigned)groups), dim3(256), 0, st, (const double *)d_a,
                            (const double *)d_b, (const uint8_t *)d_use, n, d_part));
    BB_HIP_CHECK(bb::launch(cmp_reduce_kernel<7>, dim3(1), dim3(256), 0, st, (const double *)d_part, groups, 1,
                            d_out));
    BB_HIP_CHECK(bb::launch(cmp_centred_kernel, dim3((unsigned)groups), dim3(256), 0, st, (const double *)d_a,
                            (const double *)d_b, (const uint8_t *)d_use, n, (const double *)d_out, d_part));
    BB_HIP_CHECK(bb::launch(cmp_reduce_kernel<11>, dim3(1), dim3(256), 0, st, (const double *)d_part, groups, 0,
                            d_out + 7));
    BB_HIP_CHECK(hipMemcpyAsync(out18, d_out, 18 * 8, hipMemcpyDeviceToHost, st));
    BB_HIP_CHECK(hipStreamSynchronize(st));
    return BB_OK;
}

int bb_structures_compare(const double *a, const double *b, const uint8_t *use, int64_t n,
                          const double *transform13, int flags, int device, double *aligned, double *bin_dev,
                          double *profile, double *bins, double *rank_sums, double *ms) {
    const char *who = "bb_structures_compare";
    BB_REQUIRE(a != nullptr && b != nullptr && transform13 != nullptr && bin_dev != nullptr &&
                   profile != nullptr && bins != nullptr,
               "bb_structures_compare: NULL argument");
    BB_REQUIRE(n >= 2 && n < ((int64_t)1 << 31), "bb_structures_compare: n must be in [2, 2^31)");
    BB_REQUIRE((flags & ~BB_CMP_SPEARMAN) == 0, "bb_structures_compare: unknown flag");
    const bool ranks = (flags & BB_CMP_SPEARMAN) != 0;
    BB_REQUIRE(!ranks || rank_sums != nullptr, "bb_structures_compare: BB_CMP_SPEARMAN needs rank_sums");
    std::vector<uint8_t> eff;
    const int64_t nu = used_bins(a, b, use, n, eff);
    const int64_t m = nu * (nu - 1) / 2;
    BB_REQUIRE(!ranks || m < ((int64_t)1 << 32),
               "bb_structures_compare: BB_CMP_SPEARMAN needs fewer than 2^32 pairs of used bins");
    if (ms)
        for (int q = 0; q < 5; ++q) ms[q] = 0.0;
    if (rank_sums) rank_sums[0] = rank_sums[1] = rank_sums[2] = rank_sums[3] = 0.0;
    BB_TRY(bb::use_device(device));
    CallStream cs(device);
    BB_TRY(bb::hip_status(who, bb::acquire_stream(device, &cs.st)));
    hipStream_t st = cs.st;

    // the chunks: per tile difference D its nb - D tiles in runs of at most per_chunk
    const int64_t nb = (n + kT - 1) / kT, per_chunk = (nb + kChunkSplit - 1) / kChunkSplit;
    std::vector<int4> chunks;
    std::vector<int> chunk_ptr((size_t)nb + 1, 0);
    for (int64_t D = 0; D < nb; ++D) {
        for (int64_t I = 0; I < nb - D; I += per_chunk)
            chunks.push_back(make_int4((int)D, (int)I, (int)(I + per_chunk < nb - D ? I + per_chunk : nb - D), 0));
        chunk_ptr[(size_t)D + 1] = (int)chunks.size();
    }
    const int64_t n_chunks = (int64_t)chunks.size();

    const size_t xyz_bytes = bb::align256((size_t)n * 24), use_bytes = bb::align256((size_t)n);
    const size_t slot_bytes = bb::align256((size_t)n_chunks * kNO * kProfileCols * 8);
    const size_t prof_bytes = bb::align256((size_t)n * kProfileCols * 8);
    const size_t bins_bytes = bb::align256((size_t)n * kBinCols * 8), dev_bytes = bb::align256((size_t)n * 8);
    const size_t chunk_bytes = bb::align256((size_t)n_chunks * sizeof(int4));
    const size_t ptr_bytes = bb::align256(chunk_ptr.size() * sizeof(int));
    bb::DevBuf buf;                                  // released when the call returns
    BB_TRY(alloc_named(who, buf, 3 * xyz_bytes + use_bytes + slot_bytes + prof_bytes + bins_bytes + dev_bytes +
                                     chunk_bytes + ptr_bytes + 256));
    char *p = buf.as<char>();
    double *d_a = (double *)p, *d_b = (double *)(p += xyz_bytes), *d_al = (double *)(p += xyz_bytes);
    uint8_t *d_use = (uint8_t *)(p += xyz_bytes);
    double *d_slots = (double *)(p += use_bytes);
    double *d_profile = (double *)(p += slot_bytes);
    double *d_bins = (double *)(p += prof_bytes);
    double *d_dev = (double *)(p += bins_bytes);
    int4 *d_chunks = (int4 *)(p += dev_bytes);
    int *d_chunk_ptr = (int *)(p += chunk_bytes);
    double *d_tr = (double *)(p += ptr_bytes);

    BB_HIP_CHECK(hipMemcpyAsync(d_a, a, (size_t)n * 24, hipMemcpyHostToDevice, st));
    BB_HIP_CHECK(hipMemcpyAsync(d_b, b, (size_t)n * 24, hipMemcpyHostToDevice, st));
    BB_HIP_CHECK(hipMemcpyAsync(d_use, eff.data(), (size_t)n, hipMemcpyHostToDevice, st));
    BB_HIP_CHECK(hipMemcpyAsync(d_chunks, chunks.data(), (size_t)n_chunks * sizeof(int4), hipMemcpyHostToDevice, st));
    BB_HIP_CHECK(hipMemcpyAsync(d_chunk_ptr, chunk_ptr.data(), chunk_ptr.size() * sizeof(int),
                                hipMemcpyHostToDevice, st));
    BB_HIP_CHECK(hipMemcpyAsync(d_tr, transform13, 13 * 8, hipMemcpyHostToDevice, st));
    bb::StageClock<6> clock;                         // transform | pairs | fold | bins | ranks
    BB_HIP_CHECK(clock.start(ms != nullptr));
    BB_HIP_CHECK(clock.mark(0, st));
    BB_HIP_CHECK(bb::launch(cmp_transform_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st,
                            (const double *)d_a, (const double *)d_b, (const uint8_t *)d_use, n,
                            (const double *)d_tr, d_al, d_dev));
    BB_HIP_CHECK(clock.mark(1, st));
    BB_HIP_CHECK(bb::launch(cmp_pairs_kernel, dim3((unsigned)n_chunks), dim3(256), 0, st, (const double *)d_a,
                            (const double *)d_al, (const uint8_t *)d_use, n, (const int4 *)d_chunks, d_slots));
    BB_HIP_CHECK(clock.mark(2, st));
    BB_HIP_CHECK(bb::launch(cmp_fold_kernel, dim3((unsigned)((n + 255) / 256), kProfileCols), dim3(256), 0, st,
                            (const double *)d_slots, (const int *)d_chunk_ptr, (int)nb, n, d_profile));
    BB_HIP_CHECK(clock.mark(3, st));
    BB_HIP_CHECK(bb::launch(cmp_bins_kernel, dim3((unsigned)((n + kBinsPerBlock - 1) / kBinsPerBlock)), dim3(256),
                            0, st, (const double *)d_a, (const double *)d_al, (const uint8_t *)d_use, n, d_bins));
    BB_HIP_CHECK(clock.mark(4, st));
    if (aligned) BB_HIP_CHECK(hipMemcpyAsync(aligned, d_al, (size_t)n * 24, hipMemcpyDeviceToHost, st));
    BB_HIP_CHECK(hipMemcpyAsync(bin_dev, d_dev, (size_t)n * 8, hipMemcpyDeviceToHost, st));
    BB_HIP_CHECK(hipMemcpyAsync(profile, d_profile, (size_t)n * kProfileCols * 8, hipMemcpyDeviceToHost, st));
    BB_HIP_CHECK(hipMemcpyAsync(bins, d_bins, (size_t)n * kBinCols * 8, hipMemcpyDeviceToHost, st));

    if (ranks) rank_sums[0] = (double)m;
    if (ranks && m > 0) {
        std::vector<uint32_t> idx;
        idx.reserve((size_t)nu);
        for (int64_t i = 0; i < n; ++i)
            if (eff[(size_t)i]) idx.push_back((uint32_t)i);
        const int64_t groups = (m + 255) / 256 < kRankBlocks ? (m + 255) / 256 : kRankBlocks;
        const int64_t per = bb::round_up((m + groups - 1) / groups, 256);
        const size_t k8 = bb::align256((size_t)m * 8), k4 = bb::align256((size_t)m * 4);
        const size_t idx_bytes = bb::align256((size_t)nu * 4), part_bytes = bb::align256((size_t)groups * 3 * 8);
        bb::DevBuf work;                             // keys A | keys B | places A | places B | rA | rB | ...
        BB_TRY(alloc_named(who, work, 4 * k8 + 2 * k4 + idx_bytes + part_bytes + 256));
        char *w = work.as<char>();
        bb::sort_key *ka = (bb::sort_key *)w, *kb = (bb::sort_key *)(w += k8);
        uint32_t *pa = (uint32_t *)(w += k8), *pb = (uint32_t *)(w += k4);
        double *ra = (double *)(w += k4), *rb = (double *)(w += k8);
        uint32_t *d_idx = (uint32_t *)(w += k8);
        double *d_part = (double *)(w += idx_bytes), *d_sums = (double *)(w += part_bytes);
        BB_HIP_CHECK(hipMemcpyAsync(d_idx, idx.data(), (size_t)nu * 4, hipMemcpyHostToDevice, st));
        BB_TRY(rank_pass(who, d_a, d_idx, nu, m, ka, kb, pa, pb, ra, st));
        BB_TRY(rank_pass(who, d_al, d_idx, nu, m, ka, kb, pa, pb, rb, st));
        BB_HIP_CHECK(bb::launch(cmp_rank_sum_kernel, dim3((unsigned)groups), dim3(256), 0, st, (const double *)ra,
                                (const double *)rb, m, per, d_part));
        BB_HIP_CHECK(bb::launch(cmp_reduce_kernel<3>, dim3(1), dim3(256), 0, st, (const double *)d_part, groups, 0,
                                d_sums));
        BB_HIP_CHECK(clock.mark(5, st));
        BB_HIP_CHECK(hipMemcpyAsync(rank_sums + 1, d_sums, 3 * 8, hipMemcpyDeviceToHost, st));
        BB_HIP_CHECK(hipStreamSynchronize(st));      // (work is still alive)
    }
    BB_HIP_CHECK(hipStreamSynchronize(st));
    if (ms) BB_HIP_CHECK(clock.read_all(ms));        // (no ranks: that entry is 0)
    return BB_OK;
}

}  // extern "C"
