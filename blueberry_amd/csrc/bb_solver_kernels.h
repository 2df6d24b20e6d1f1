// bb_solver_kernels.h -- device code of the core of the 3D-structure solver (gfx950 only): the
// pair math, the stress + gradient sweep, the deterministic partial reduce (+ update / exchange
// / peer push, and the one-launch peer exchange over the helpers of bb_peer_kernels.h), the
// apply kernel, the row-owner kernel, the 24-bit stream's pack kernels and the f64 <-> T
// conversions.  Included by bb_solver.hip and by nothing else in the library (the tests' probe
// of the refined fp64 routines includes it too): everything here lives in the including
// translation unit's anonymous namespace.  The kernels of the input routes:
// bb_input_kernels.h; of the queries: bb_query_kernels.h.  Shapes, wave helpers, the streaming
// loads and shared constants: bb_solver_device.h.
//
// Specification: docs/SPEC.md (build-authored; the reference has no solver,
// SURVEY.md section 0).  Data layout and kernel design: DESIGN.md 3-4.
#pragma once

#include "bb_solver_device.h"
#include "bb_peer_kernels.h"

namespace {

// --------------------------------------------------------------------------
// stress + gradient kernel
// --------------------------------------------------------------------------
// 1/sqrt(d2) and sqrt(d2) in fp64 from the v_rsq_f64 seed (relative error <= 2^-23) by ONE
// third-order step: with e = 1 - d2 r0^2, r = r0 (1 - e)^(-1/2) = r0 (1 + e/2 + 3 e^2/8 + ...);
// the term dropped is 5 e^3 / 16 < 1e-20, so both results are good to the last bit or two.
// 6 instructions behind the seed (two Newton steps on r plus one on the root took 10).
__device__ __forceinline__ void rsqrt_sqrt_f64(double d2, double &rinv, double &dist) {
    const double r0 = __builtin_amdgcn_rsq(d2);
    const double t = d2 * r0;                    // ~ sqrt(d2)
    const double e = fma(-t, r0, 1.0);
    const double q = e * fma(e, 0.375, 0.5);
    rinv = fma(r0, q, r0);
    dist = fma(t, q, t);
}
// 1.0 where delta > 0, else 0.0, in one instruction (see wish_floor): the compiler folds
// min(max(x, 0), 1) into the clamp output modifier (v_ldexp_f64 ... clamp).  Not inline asm:
// asm statements are convergent in HIP device code, and a loop that holds one is not
// unrolled at run time (row_owner_kernel).
__device__ __forceinline__ double weight01_f64(double delta) {
    return __builtin_fmin(__builtin_fmax(delta * 0x1p1000, 0.0), 1.0);
}

// 1/x in fp64 from the v_rcp_f64 seed (relative error ~2^-26) by one third-order step:
// with e = 1 - x r0, 1/x = r0 (1 + e + e^2 + ...); the term dropped is e^3 < 2^-78.
__device__ __forceinline__ double rcp_f64(double x) {
    const double r0 = __builtin_amdgcn_rcp(x);
    const double e = fma(-x, r0, 1.0);
    return fma(r0, fma(e, e, e), r0);
}

// Pair math of one fp64 pair: column C (0, 1) of a 16-byte load (fp32 has pair_step2).
template <int C, int OP>
__device__ __forceinline__ void pair_step(const double2 &drow, double xi, double yi, double zi,
                                          const double (&xj)[2][3], double (&gc)[2][3], double &gx,
                                          double &gy, double &gz, double &s) {
    using T = double;
    const T delta = C == 0 ? drow.x : drow.y;
    if constexpr (OP == kOpMatvec2) {
        const T a = delta * delta;
        gx += a * xj[C][0]; gy += a * xj[C][1]; gz += a * xj[C][2];
        gc[C][0] += a * xi; gc[C][1] += a * yi; gc[C][2] += a * zi;
        return;
    }
    const T dx = xi - xj[C][0], dy = yi - xj[C][1], dz = zi - xj[C][2];
    const T d2 = fma(dx, dx, fma(dy, dy, fma(dz, dz, Traits<T>::eps2())));  // SPEC 2.2
    // fp64 has no packed forms and its pair math alone is worth the HBM time of a
    // unit, so every instruction counts: 25 + v_rsq per pair
    T rinv, dist;
    rsqrt_sqrt_f64(d2, rinv, dist);
    if constexpr (is_weighted_op<OP>()) {
        // SPEC 2.3.1.  m = 1 (delta > 0) or 0; r = 1/delta, or 1/1 where delta = 0 so that
        // nothing is inf (inf * 0 = NaN): res = 0 there and so is everything below
        const T m = weight01_f64(delta);
        const T res = fma(dist, m, -delta);
        const T r = rcp_f64(delta + (1.0 - m));
        const T u = res * r;                     // (d - delta) / delta
        T coef;
        if constexpr (OP == kOpStressW1) {
            s = fma(res, u, s);                  // (d - delta)^2 / delta
            coef = u * rinv;
        } else {
            s = fma(u, u, s);                    // ((d - delta) / delta)^2
            coef = (u * r) * rinv;
        }
        gx = fma(coef, dx, gx); gy = fma(coef, dy, gy); gz = fma(coef, dz, gz);
        gc[C][0] = fma(-coef, dx, gc[C][0]);
        gc[C][1] = fma(-coef, dy, gc[C][1]);
        gc[C][2] = fma(-coef, dz, gc[C][2]);
        return;
    }
    // (dist - delta) or 0 in ONE instruction: w is 1, or 0 exactly where delta is 0, so
    // dist * w - delta is dist - delta (the product is exact) or 0 - 0
    const T res = fma(dist, weight01_f64(delta), -delta);
    s = fma(res, res, s);
    const T coef = res * rinv;  // (d - delta) / d ; the factor 2 is applied in the reduce
    gx = fma(coef, dx, gx); gy = fma(coef, dy, gy); gz = fma(coef, dz, gz);
    gc[C][0] = fma(-coef, dx, gc[C][0]);
    gc[C][1] = fma(-coef, dy, gc[C][1]);
    gc[C][2] = fma(-coef, dz, gc[C][2]);
}

// Where a wave's rolling window is refilled from: the k-th wave-load (1 KiB) of the NEXT
// unit, through plain pointers.  (Buffer loads through a descriptor of the wave's chunk, so
// that the refills of its last unit fall out of range, measured 1.5-2.5 us slower per launch:
// profiles/r03_window_ab.txt.  The pointer form gets the same saving by pointing all lanes of
// those last refills at one line: see window_of in the kernel.)  The fp64 units keep a pointer per
// lane; the fp32 unit gives the same addresses as a scalar base + a lane offset (WinBase32).
template <typename Vec>
struct WinPtr {
    const Vec *p;
    template <bool NT>
    __device__ __forceinline__ Vec load(int k) const { return stream_load<NT>(p + k * 64); }
};

// The three unit forms (fp64 narrow, fp64 wide, fp32) share one shape: load k of row r of
// the CURRENT unit is consumed from d[r*LPR + k], which is then refilled at once with the same
// load of the NEXT unit, so 8 KiB per wave stay in flight with a single register window.
// xrow.get(q): the unit's q-th row coordinate, wave-uniform.
//
// ---- fp64, 8 x 128 units: one wave-load per matrix row, row sums by the DPP tree ----
template <bool NT, int OP, typename XR, typename WIN>
__device__ __forceinline__ void process_unit_f64n(double2 (&d)[8], const XR &xrow, const WIN &next,
                                                  const double (&xj)[1][2][3], double (&gc)[1][2][3],
                                                  double &stress, __amdgpu_buffer_rsrc_t row_rsrc,
                                                  unsigned row_voff) {
    double s = 0.0;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const double xi = xrow.get(3 * r), yi = xrow.get(3 * r + 1), zi = xrow.get(3 * r + 2);
        double gx = 0.0, gy = 0.0, gz = 0.0;
        pair_step<0, OP>(d[r], xi, yi, zi, xj[0], gc[0], gx, gy, gz, s);
        pair_step<1, OP>(d[r], xi, yi, zi, xj[0], gc[0], gx, gy, gz, s);
        d[r] = next.template load<NT>(r);
        wave_sum_hi3(gx, gy, gz);
        // one 3-element store per matrix row, from the lane holding the sums
        store_row3(row_rsrc, row_voff + r * 24u, gx, gy, gz);
        // keep the rows in program order: otherwise the scheduler interleaves the
        // rows for ILP and spills
        __builtin_amdgcn_sched_barrier(0);
    }
    stress += s;
}

// ---- fp64, 2 x 512 units: the row sums go through the matrix pipe ---------------
// In fp64 the pair math alone (~35 ops per pair, no packed forms) is worth the whole HBM
// time of a unit, so everything else the VALU does is paid in full.  The largest such
// item was the cross-lane reduction of the 6 row sums of a unit: v_add_f64 has no DPP
// form, so each of the 6 tree steps of each sum is 2 v_mov_dpp + 1 add -- 108
// instructions per unit, a sixth of the unit.  v_mfma_f64_16x16x4_f64 adds across lanes
// for free: with A = one partial sum per lane (A[i][k] = lane i + 16 k) and B = a 0/1
// selector with ones in column v, D[i][v] += sum_k A[i][k], and six of them accumulate the
// unit's six sums side by side in the columns 0..5 of ONE 16 x 16 accumulator.  What is
// left for the VALU: 3 adds over the lane's 4 accumulator rows and 2 lane-preserving
// shuffles over the 4 lane groups.  The matrix pipe is idle otherwise and runs beside the
// partner wave's VALU work; the order of the additions is fixed (bitwise reproducible).
typedef double f64x4 __attribute__((ext_vector_type(4)));

// t + (t of the lane 16 / 32 further on or back): x = {r0, r0, r2, r2}, y = {r1, r1, r3, r3}
__device__ __forceinline__ double swap_sum16(double t) {
    const unsigned lo = (unsigned)__double2loint(t), hi = (unsigned)__double2hiint(t);
    const auto a = __builtin_amdgcn_permlane16_swap(lo, lo, false, false);
    const auto b = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
    return __hiloint2double((int)b[0], (int)a[0]) + __hiloint2double((int)b[1], (int)a[1]);
}
__device__ __forceinline__ double swap_sum32(double t) {
    const unsigned lo = (unsigned)__double2loint(t), hi = (unsigned)__double2hiint(t);
    const auto a = __builtin_amdgcn_permlane32_swap(lo, lo, false, false);
    const auto b = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
    return __hiloint2double((int)b[0], (int)a[0]) + __hiloint2double((int)b[1], (int)a[1]);
}

// The 12 row sums of an fp32 unit (4 matrix rows x 3 components) over the 64 lanes, as ONE
// transposed reduction: 12 registers of per-lane partials in, one register out that holds
// every total.  gfx950's lane swaps exchange half of one register with the other half of a
// second one, so ONE swap + ONE add both adds across the halves and sorts two sums apart --
// registers and lane span halve together:
//   v_permlane32_swap + add   12 -> 6 registers: lanes 0..31 hold the first sum of a pair,
//                             lanes 32..63 the second
//   v_permlane16_swap + add    6 -> 3 registers: the even 16-lane rows hold the first register's
//                             two sums, the odd rows the second's
//   row16_sum3                 3 -> 1: the totals of the 16-lane rows of three registers
// 6 + 3 swaps, 9 adds and 7 DPP adds per unit, against 4 x (3 swaps + 3 adds + 4 DPP adds + one
// select) for a tree per matrix row.  Fixed tree: bitwise reproducible.
__device__ __forceinline__ float swap_add32(float a, float b) {
    const auto s = __builtin_amdgcn_permlane32_swap(__float_as_uint(a), __float_as_uint(b), false, false);
    return __uint_as_float(s[0]) + __uint_as_float(s[1]);
}
__device__ __forceinline__ float swap_add16(float a, float b) {
    const auto s = __builtin_amdgcn_permlane16_swap(__float_as_uint(a), __float_as_uint(b), false, false);
    return __uint_as_float(s[0]) + __uint_as_float(s[1]);
}
// Sums over each 16-lane row of a, b and c.  The write mask of a DPP instruction has a bit per
// bank of 4 lanes, which lets the DPP steps halve the registers too: after row_mirror a row's
// lanes 0..7 hold all there is of it, so lanes 8..15 of the same register take c's; after
// row_half_mirror lanes 0..3 do, and lanes 4..7 take b's.  Result: in every 16-lane row, a's
// total in lanes 0..3, b's in 4..7, c's in 8..11 (12..15: c's again).  One asm block for the
// same reason as wave_sum_hi3: a DPP read needs 2 wait states after the VALU write of its
// source, and the block places its own (the inputs were just written by VALU code).
__device__ __forceinline__ float row16_sum3(float a, float b, float c) {
    float t, u, w;
    asm("s_nop 1\n\t"
        "v_add_f32_dpp %0, %3, %3 row_mirror row_mask:0xf bank_mask:0xf\n\t"
        "v_add_f32_dpp %0, %5, %5 row_mirror row_mask:0xf bank_mask:0xc\n\t"
        "v_add_f32_dpp %1, %4, %4 row_mirror row_mask:0xf bank_mask:0xf\n\t"
        "s_nop 0\n\t"
        "v_add_f32_dpp %2, %0, %0 row_half_mirror row_mask:0xf bank_mask:0xf\n\t"
        "v_add_f32_dpp %2, %1, %1 row_half_mirror row_mask:0xf bank_mask:0x2\n\t"
        "s_nop 1\n\t"
        "v_add_f32_dpp %2, %2, %2 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
        "s_nop 1\n\t"
        "v_add_f32_dpp %2, %2, %2 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf"
        : "=&v"(t), "=v"(u), "=v"(w)   // u and w are written when a, b and c have been read
        : "v"(a), "v"(b), "v"(c));
    return w;
}
// The tree above the 16-lane rows.  g[3 * r + c]: this lane's partial of component c of matrix
// row r = the unit's row sum number 3 r + c.  Pairs (2i, 2i + 1) meet in the 32-lane step (h),
// registers (2m, 2m + 1) in the 16-lane step (m), so register m of the last step holds the sums
// 4m, 4m + 2, 4m + 1, 4m + 3 in its rows 0..3 (swap_rowsum_slot is the inverse of this).
// row_sums_step<R> does every step whose inputs are there after matrix row R -- the tree is the
// same wherever its steps are issued, and at most three registers of it live across a row's
// pair math instead of nine.
template <int R>
__device__ __forceinline__ void row_sums_step(const float (&g)[12], float (&h)[6], float (&m)[3]) {
    if constexpr (R == 0) h[0] = swap_add32(g[0], g[1]);
    if constexpr (R == 1) {
        h[1] = swap_add32(g[2], g[3]); h[2] = swap_add32(g[4], g[5]);
        m[0] = swap_add16(h[0], h[1]);
    }
    if constexpr (R == 2) { h[3] = swap_add32(g[6], g[7]); m[1] = swap_add16(h[2], h[3]); }
    if constexpr (R == 3) {
        h[4] = swap_add32(g[8], g[9]); h[5] = swap_add32(g[10], g[11]);
        m[2] = swap_add16(h[4], h[5]);
    }
}
// which of a unit's 12 row sums a lane holds after row_sums_step + row16_sum3.  EVERY lane holds
// one: the four lanes of a bank carry the same bits (the last two steps add the same four
// values, and a + b = b + a bit for bit), and so do banks 2 and 3 (what lanes 12..15 add up is
// what lanes 11..8 do, operands swapped).
__device__ __forceinline__ int swap_rowsum_slot(int lane) {
    const int row = lane >> 4, bank = (lane >> 2) & 3;
    return 4 * (bank < 3 ? bank : 2) + ((row & 1) << 1) + (row >> 1);
}
// the lane that stores the sum: the first of the banks 0..2 of every 16-lane row
__device__ __forceinline__ bool swap_rowsum_stores(int lane) { return (lane & 3) == 0 && (lane & 12) != 12; }

template <bool NT, int OP, typename XR, typename WIN>
__device__ __forceinline__ void process_unit_f64w(double2 (&d)[8], const XR &xrow,
                                                  const WIN &next,
                                                  const double (&xj)[4][2][3], double (&gc)[4][2][3],
                                                  const double (&sel)[6], double &stress,
                                                  __amdgpu_buffer_rsrc_t row_rsrc, unsigned row_voff,
                                                  int stage_idx) {
    extern __shared__ __attribute__((aligned(16))) float row_lds[];
    double s = 0.0;
    f64x4 acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const double xi = xrow.get(3 * r), yi = xrow.get(3 * r + 1), zi = xrow.get(3 * r + 2);
        double gx = 0.0, gy = 0.0, gz = 0.0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            pair_step<0, OP>(d[r * 4 + k], xi, yi, zi, xj[k], gc[k], gx, gy, gz, s);
            pair_step<1, OP>(d[r * 4 + k], xi, yi, zi, xj[k], gc[k], gx, gy, gz, s);
            d[r * 4 + k] = next.template load<NT>(r * 4 + k);
        }
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(gx, sel[3 * r + 0], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(gy, sel[3 * r + 1], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(gz, sel[3 * r + 2], acc, 0, 0, 0);
    }
    // lane (g = lane / 16, j = lane % 16) holds four of the 16 rows of column j: add them,
    // then the 4 lane groups with the gfx950 lane swaps (VALU, no LDS round trip):
    // permlane16_swap exchanges the odd 16-lane rows of one register with the even rows
    // of the other, permlane32_swap the upper half with the lower half
    double t = (acc.x + acc.y) + (acc.z + acc.w);
    t = swap_sum16(t);
    t = swap_sum32(t);                   // every lane with lane % 16 == v: the unit's sum v
    // lanes 48..53 keep one sum each; parked in LDS or stored, exactly one of the two lands
    *reinterpret_cast<double *>(row_lds + stage_idx) = t;
    const u32x2 bits = {(unsigned)__double2loint(t), (unsigned)__double2hiint(t)};
    __builtin_amdgcn_raw_buffer_store_b64(bits, row_rsrc, row_voff, 0, 0);
    stress += s;
}

// ---- fp32: the same unit with explicit 2-wide packed math (v_pk_*_f32) -------
// A lane owns 8 columns of the 512-wide strip: load k (k = 0,1) brings columns
// k*256 + 4*lane .. +3, and within a load the pairs {0,1} and {2,3} share every
// instruction that has a packed form.  Column-side state is [load][half]
// [component] so that the two pairs of a half sit in adjacent registers.
typedef float f32x2 __attribute__((ext_vector_type(2)));

struct StripF32 {
    f32x2 x[2][2][3];  // coordinates of this lane's columns
    f32x2 g[2][2][3];  // column-side gradient accumulators, same shape
};

// w = 1 where delta > 0, else 0, for both halves in ONE instruction:
// clamp(delta * 2^100) saturates any delta >= 2^-100 to 1 and leaves 0 at 0
// (delta is never negative or NaN: the pack kernels store 0 for "no
// constraint" and flush anything below 1e-30).  Replaces 2 v_cmp + 2 v_cndmask.
__device__ __forceinline__ f32x2 weight01(f32x2 delta) {
    f32x2 w;
    const f32x2 big = {0x1p100f, 0x1p100f};
    asm("v_pk_mul_f32 %0, %1, %2 clamp" : "=v"(w) : "v"(delta), "v"(big));
    return w;
}

// The row coordinates of an fp32 unit: x0 y0 | z0 x1 | y1 z1 | x2 y2 | z2 x3 | y3 z3, twelve
// consecutive floats of X fetched through the scalar cache as six 64-bit scalars, so that every
// pair sits in an aligned pair of scalar registers.  Coordinate q is half q & 1 of pair q >> 1.
struct XRowS32 {
    f32x2 p[6];
};
// {s, s} - xj for the scalar s = half HALF of `pair`, read where it is: a VOP3P source may be an
// aligned scalar pair, and op_sel / op_sel_hi pick the same half of it for both results.  The
// instruction hipcc forms for f32x2{s, s} - xj once s is in a vector register, without the copy
// that puts it there (12 v_mov_b32 per unit).  One scalar source: within the constant-bus limit.
template <int HALF>
__device__ __forceinline__ f32x2 row_minus(f32x2 pair, f32x2 xj) {
    f32x2 d;
    if constexpr (HALF == 0)
        asm("v_pk_add_f32 %0, %1, %2 op_sel_hi:[0,1] neg_lo:[0,1] neg_hi:[0,1]"
            : "=v"(d) : "s"(pair), "v"(xj));
    else
        asm("v_pk_add_f32 %0, %1, %2 op_sel:[1,0] op_sel_hi:[1,1] neg_lo:[0,1] neg_hi:[0,1]"
            : "=v"(d) : "s"(pair), "v"(xj));
    return d;
}
// acc += a * {s, s}, the matvec's column side, from the pair in the same way (the fused multiply-add
// hipcc contracts `acc += a * xi` to: the same bits)
template <int HALF>
__device__ __forceinline__ void row_fma(f32x2 &acc, f32x2 a, f32x2 pair) {
    if constexpr (HALF == 0)
        asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel_hi:[1,0,1]" : "+v"(acc) : "v"(a), "s"(pair));
    else
        asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel:[0,1,0] op_sel_hi:[1,1,1]"
            : "+v"(acc) : "v"(a), "s"(pair));
}

// MASK = false (kOpStress only): the caller knows that no delta of the unit is 0 -- a packed unit
// of the 24-bit stream with base != 0, see process_unit_f32 -- so the weight is exactly 1.0f and
// res * 1.0f is res, bit for bit: neither is formed.
// R: the matrix row of the unit; its coordinates are read from the scalar pairs of `xr`.
template <int K, int H, bool FIRST, int OP, int R, bool MASK = true>
__device__ __forceinline__ void pair_step2(f32x2 delta, const XRowS32 &xr, StripF32 &st,
                                           f32x2 &rx, f32x2 &ry, f32x2 &rz, f32x2 &s2) {
    static_assert(MASK || OP == kOpStress, "only the plain stress sweep has a mask-free form");
    constexpr int QX = 3 * R, QY = 3 * R + 1, QZ = 3 * R + 2;
    if constexpr (OP == kOpMatvec2) {
        const f32x2 a = delta * delta;
        if constexpr (FIRST) {
            rx = a * st.x[K][H][0]; ry = a * st.x[K][H][1]; rz = a * st.x[K][H][2];
        } else {
            rx += a * st.x[K][H][0]; ry += a * st.x[K][H][1]; rz += a * st.x[K][H][2];
        }
        row_fma<QX & 1>(st.g[K][H][0], a, xr.p[QX >> 1]);
        row_fma<QY & 1>(st.g[K][H][1], a, xr.p[QY >> 1]);
        row_fma<QZ & 1>(st.g[K][H][2], a, xr.p[QZ >> 1]);
        return;
    }
    const f32x2 eps2 = {1e-30f, 1e-30f};
    const f32x2 dx = row_minus<QX & 1>(xr.p[QX >> 1], st.x[K][H][0]),
                dy = row_minus<QY & 1>(xr.p[QY >> 1], st.x[K][H][1]),
                dz = row_minus<QZ & 1>(xr.p[QZ >> 1], st.x[K][H][2]);
    const f32x2 d2 = dx * dx + (dy * dy + (dz * dz + eps2));  // SPEC 2.2: |d|^2 + eps^2
    f32x2 rinv;
    rinv.x = __builtin_amdgcn_rsqf(d2.x);
    rinv.y = __builtin_amdgcn_rsqf(d2.y);
    if constexpr (is_weighted_op<OP>()) {
        // SPEC 2.3.1: the weight w = 1/delta resp. 1/delta^2 by one v_rcp_f32 per pair (the
        // square first: as many live values as q = 1, where w (r) then r (rinv) would spill
        // the 4-wave form), of max(., 2^-126) so that delta = 0 gives a finite w -- res is 0
        // there and so is everything below (never inf * 0).  t = w (d - delta)
        const f32x2 res = (d2 * rinv - delta) * weight01(delta);
        f32x2 a = delta;
        if constexpr (OP == kOpStressW2) a = delta * delta;
        f32x2 w;
        w.x = __builtin_amdgcn_rcpf(__builtin_fmaxf(a.x, 0x1p-126f));
        w.y = __builtin_amdgcn_rcpf(__builtin_fmaxf(a.y, 0x1p-126f));
        const f32x2 t = res * w;
        s2 += res * t;
        const f32x2 coef = t * rinv;
        if constexpr (FIRST) {
            rx = coef * dx; ry = coef * dy; rz = coef * dz;
        } else {
            rx += coef * dx; ry += coef * dy; rz += coef * dz;
        }
        st.g[K][H][0] -= coef * dx;
        st.g[K][H][1] -= coef * dy;
        st.g[K][H][2] -= coef * dz;
        return;
    }
    f32x2 res = d2 * rinv - delta;
    if constexpr (MASK) res *= weight01(delta);  // (dist - delta) or 0
    s2 += res * res;
    const f32x2 coef = res * rinv;
    if constexpr (FIRST) {
        rx = coef * dx; ry = coef * dy; rz = coef * dz;
    } else {
        rx += coef * dx; ry += coef * dy; rz += coef * dz;
    }
    st.g[K][H][0] -= coef * dx;
    st.g[K][H][1] -= coef * dy;
    st.g[K][H][2] -= coef * dz;
}

// d[] holds the unit's 8 wave-loads in row order: d[2*r + k] = row r, load k.
// Row side: both loads of a matrix row run into ONE chain of packed accumulators (load 1
// continues load 0's), whose halves are added once per row; the 12 per-lane partials of the
// unit then go through one transposed reduction (row_sums_step, row16_sum3: 25 cross-lane and add
// instructions per unit where a tree per matrix row took 56, and no select).  Through the
// matrix pipe, as the fp64 unit does, the row sums measured 2.7-6 % slower at every size (164
// VGPRs, the wait for the accumulator at the end of every unit:
// profiles/r03_mfma_rowsum_ab.txt).  At two waves per SIMD the chip runs this kernel at
// 1.75-1.83 GHz (power) and the SIMD's VALU is then busy most of a unit's time, so an
// instruction less per unit is time (docs/MEASUREMENTS.md, machine code against the parent).
//
// PK: the unit is a PACKED unit of the 24-bit stream (SPEC 3.7), 6 wave-loads.  Dword c of
// load L = 2r + k (rows 0..2) carries the code of the pair (r, k, c) in its low 24 bits and one
// byte of a row-3 code on top: the codes of row 3, load 0 lie on loads 0, 1, 2 (bytes 0, 1, 2),
// those of row 3, load 1 on loads 4, 5, 3.  So the two loads of row 0 give up their top bytes
// together and are refilled as in a raw unit, as are those of row 2; only load 3 waits one row
// for its refill.  Decode: one v_mad_u32_u24 per pair of rows 0..2 (mask to 24 bits, add the
// unit's base from a scalar register), two v_perm_b32 and one add per pair of row 3 -- 48 per
// unit (row 1 decodes load 3, which keeps its top bytes for row 2, out of place into the
// registers of load 2: no move).
// This body runs the packed units whose base is not 0, and those hold NO empty pair: every
// stored wish distance is 0 or at least 1e-30 (bb_wish.h), whose bit pattern lies above 2^24,
// and a unit packs only when its words span less than 2^24 from the base, its smallest word --
// so a zero in the unit means base = 0 and nothing but zeros (such a unit goes through the raw
// body: bb_sweep_body.inc).  1e-30 is above 2^-100, where weight01 saturates: every weight here
// is exactly 1.0f, and the body forms neither the weight nor res * weight (MASK = false, 32
// packed instructions per unit).  The pair math, its order and every sum are otherwise those
// of the raw unit: the bits are the same.
template <bool ROW3>
__device__ __forceinline__ void pk24_decode(float &word, unsigned base) {
    // volatile: memory operations keep their side of such a statement, so the refills stay in
    // the row that issues them.  Their only reader is the NEXT trip of the loop, and left alone
    // hipcc decodes the whole unit up front (waiting for all six loads at once) and sinks all
    // six refills to the end of the body: the window then stands empty for most of a unit.
    // That hipcc keeps plain loads on their side of these statements is what it does, not what
    // the language promises, and no test fails if it stops: after a compiler update rerun
    // `tools/vmcnt_pattern.sh stream24_grad_kernelIfLb1ELb1ELi0ELi8` and look for the packed
    // body's waits 5 6 5 4 (docs/MEASUREMENTS.md, "the 24-bit stream").
    if constexpr (ROW3) {   // the collected code of a row-3 pair: its top byte is 0
        asm volatile("v_add_u32 %0, %0, %1" : "+v"(word) : "s"(base));
    } else {
        asm volatile("v_mad_u32_u24 %0, %0, 1, %1" : "+v"(word) : "s"(base));
    }
}
template <bool ROW3>
__device__ __forceinline__ void pk24_decode(float4 &w, unsigned base) {
    pk24_decode<ROW3>(w.x, base); pk24_decode<ROW3>(w.y, base);
    pk24_decode<ROW3>(w.z, base); pk24_decode<ROW3>(w.w, base);
}
// out of place: the codes of `src`, whose top bytes are still wanted, as distances in `dst`
__device__ __forceinline__ void pk24_decode_to(float &dst, float src, unsigned base) {
    asm volatile("v_mad_u32_u24 %0, %1, 1, %2" : "=v"(dst) : "v"(src), "s"(base));
}
__device__ __forceinline__ void pk24_decode_to(float4 &dst, const float4 &src, unsigned base) {
    pk24_decode_to(dst.x, src.x, base); pk24_decode_to(dst.y, src.y, base);
    pk24_decode_to(dst.z, src.z, base); pk24_decode_to(dst.w, src.w, base);
}
constexpr unsigned kPk24SelPair = 0x0c0c0703u;   // {0, 0, top of S0, top of S1}
constexpr unsigned kPk24SelThird = 0x0c070100u;  // {0, top of S0, byte 1 of S1, byte 0 of S1}
__device__ __forceinline__ float pk24_tops(float hi, float lo, unsigned sel) {
    float v;   // (volatile for the reason given at pk24_decode: it needs its row's loads, no others)
    asm volatile("v_perm_b32 %0, %1, %2, %3" : "=v"(v) : "v"(hi), "v"(lo), "s"(sel));
    return v;
}
__device__ __forceinline__ float4 pk24_tops(float4 hi, float4 lo, unsigned sel) {
    return make_float4(pk24_tops(hi.x, lo.x, sel), pk24_tops(hi.y, lo.y, sel),
                       pk24_tops(hi.z, lo.z, sel), pk24_tops(hi.w, lo.w, sel));
}

// The row coordinates of the NEXT unit, into the registers of the current one as matrix row R lets
// go of them: a second set of twelve does not fit the scalar file beside the rest of the sweep,
// and a refresh in place needs none.  Rows 0 and 1 share the pair z0 x1, rows 2 and 3 z2 x3, so
// x y of an even row go when that row is done and the other four floats after the odd row: each
// scalar load is at least a quarter of a unit ahead of its first reader.
// xnext: where the next unit's rows begin in X, in bytes.  `after` is a value of row R that
// exists only when the row's subtracts are done (one of its sums); the empty asm statement makes
// the load's address depend on it.  X is read-only here, so nothing else orders these loads, and
// left alone hipcc issues all of them early in the raw body, into twelve more registers that it
// copies over at the end: a double buffer again, and scalars spilled around the loops.
template <int R>
__device__ __forceinline__ void xrow_refresh(XRowS32 &xr, const float *__restrict__ X, unsigned xnext,
                                             float after) {
    asm("" : "+s"(xnext) : "v"(after));
    const f32x2 *__restrict__ px =
        reinterpret_cast<const f32x2 *>(reinterpret_cast<const char *>(X) + xnext);
    constexpr int P = 3 * (R >> 1);
    if constexpr (R & 1) {
        xr.p[P + 1] = px[P + 1];
        xr.p[P + 2] = px[P + 2];
    } else {
        xr.p[P] = px[P];
    }
}

// The fp32 window: the k-th wave-load of a unit from a wave-uniform base, kept in scalar
// registers, and a 32-bit per-lane byte offset that is a loop constant (lane * 16; 0 where all
// lanes ask for the same 16 bytes: window_of) -- global_load_dwordx4 v, v_off, s[base:base+1].
// The base points at the unit's byte 4,096, so that the instruction's signed 13-bit offset
// reaches all eight KiB.  The addresses are those of WinPtr.
struct WinBase32 {
    const char *mid;
    unsigned voff;
    // (the distance through an empty asm statement: hipcc otherwise folds the 4,096 back into
    // the offsets, reaches four loads from the scalar base and builds 64-bit vector addresses
    // for the rest; the distance and not the pointer, which stays a pointer to global memory)
    __device__ __forceinline__ WinBase32(const void *units, int64_t unit_byte, unsigned lane_off)
        : voff(lane_off) {
        int64_t to_mid = unit_byte + 4096;
        asm("" : "+s"(to_mid));
        mid = static_cast<const char *>(units) + to_mid;
    }
    template <bool NT>
    __device__ __forceinline__ float4 load(int k) const {
        return stream_load<NT>(reinterpret_cast<const float4 *>(mid + voff + (k * 1024 - 4096)));
    }
};

template <bool NT, int OP, bool PK = false, typename WIN>
__device__ __forceinline__ void process_unit_f32(float4 (&d)[8], XRowS32 &xrow, const float *X,
                                                 unsigned xnext, const WIN &next, StripF32 &st,
                                                 double &stress, __amdgpu_buffer_rsrc_t row_rsrc,
                                                 unsigned row_voff, int stage_idx,
                                                 unsigned base = 0u) {
    extern __shared__ __attribute__((aligned(16))) float row_lds[];
    f32x2 s2 = {0.f, 0.f};
    float g[12], h[6], m[3];  // the unit's 12 row sums on their way through the tree
    auto row = [&](auto rc) __attribute__((always_inline)) {
        constexpr int r = decltype(rc)::value;
        f32x2 rx, ry, rz;  // row-side sums of the row's 8 pairs
        if constexpr (PK) {
            // The codes become distances IN the window's registers, and d[6], d[7] -- which a
            // packed unit has no loads for -- collect the codes of row 3: the body holds what
            // the raw one holds (alone in the kernel it takes 124 VGPRs).  Row 1 decodes its
            // second load INTO the registers of its first (done with by then), because load 3
            // keeps its top bytes for row 2.  No pair of this body has a zero distance: no mask.
            constexpr int A = r < 3 ? 2 * r : 6, B = r == 0 ? 1 : (r == 1 ? 2 : (r == 2 ? 5 : 7));
            if constexpr (r == 0) d[6] = pk24_tops(d[1], d[0], kPk24SelPair);
            if constexpr (r == 1) d[6] = pk24_tops(d[2], d[6], kPk24SelThird);
            if constexpr (r == 2) {
                d[7] = pk24_tops(d[3], pk24_tops(d[5], d[4], kPk24SelPair), kPk24SelThird);
                d[3] = next.template load<NT>(3);
            }
            pk24_decode<r == 3>(d[A], base);
            pair_step2<0, 0, true, OP, r, false>(f32x2{d[A].x, d[A].y}, xrow, st, rx, ry, rz, s2);
            pair_step2<0, 1, false, OP, r, false>(f32x2{d[A].z, d[A].w}, xrow, st, rx, ry, rz, s2);
            if constexpr (r == 0) d[0] = next.template load<NT>(0);
            if constexpr (r == 2) d[4] = next.template load<NT>(4);
            if constexpr (r == 1) pk24_decode_to(d[2], d[3], base);
            else pk24_decode<r == 3>(d[B], base);
            pair_step2<1, 0, false, OP, r, false>(f32x2{d[B].x, d[B].y}, xrow, st, rx, ry, rz, s2);
            pair_step2<1, 1, false, OP, r, false>(f32x2{d[B].z, d[B].w}, xrow, st, rx, ry, rz, s2);
            if constexpr (r == 0) d[1] = next.template load<NT>(1);
            if constexpr (r == 1) d[2] = next.template load<NT>(2);
            if constexpr (r == 2) d[5] = next.template load<NT>(5);
            g[3 * r] = rx.x + rx.y; g[3 * r + 1] = ry.x + ry.y; g[3 * r + 2] = rz.x + rz.y;
            row_sums_step<r>(g, h, m);
            xrow_refresh<r>(xrow, X, xnext, g[3 * r + 2]);
            return;
        }
        pair_step2<0, 0, true, OP, r>(f32x2{d[2 * r].x, d[2 * r].y}, xrow, st, rx, ry, rz, s2);
        pair_step2<0, 1, false, OP, r>(f32x2{d[2 * r].z, d[2 * r].w}, xrow, st, rx, ry, rz, s2);
        d[2 * r] = next.template load<NT>(2 * r);
        // (no sched_barrier here: letting the scheduler mix the rows of a unit measured
        // 1 % faster at N=50k and 6 % faster at 1/8 size; it stays within 125 VGPRs)
        pair_step2<1, 0, false, OP, r>(f32x2{d[2 * r + 1].x, d[2 * r + 1].y}, xrow, st, rx, ry, rz, s2);
        pair_step2<1, 1, false, OP, r>(f32x2{d[2 * r + 1].z, d[2 * r + 1].w}, xrow, st, rx, ry, rz, s2);
        d[2 * r + 1] = next.template load<NT>(2 * r + 1);
        g[3 * r] = rx.x + rx.y; g[3 * r + 1] = ry.x + ry.y; g[3 * r + 2] = rz.x + rz.y;
        row_sums_step<r>(g, h, m);
        xrow_refresh<r>(xrow, X, xnext, g[3 * r + 2]);
    };
    row(std::integral_constant<int, 0>{});
    row(std::integral_constant<int, 1>{});
    row(std::integral_constant<int, 2>{});
    row(std::integral_constant<int, 3>{});
    const float keep = row16_sum3(m[0], m[1], m[2]);   // every sum in its lane (swap_rowsum_slot)
    // both are issued for every unit and exactly one of them counts -- while the unit is
    // stored directly the LDS write goes to the wave's parking slot 0, which the first parked
    // unit overwrites; the store's lanes are all out of range (free) while the unit is
    // parked (see the kernel's DEFER)
    row_lds[stage_idx] = keep;
    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(keep), row_rsrc, row_voff, 0, 0);
    stress += (double)(s2.x + s2.y);
}

// load_strip(st, X, j0, lane): the strip's coordinates, accumulators zeroed; store_strip(st,
// slot, lane): its column partial in the layout of a slot -- one overload per strip state
__device__ __forceinline__ void load_strip(StripF32 &st, const float *__restrict__ X, int j0,
                                           int lane) {
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const float4 *p = reinterpret_cast<const float4 *>(
            X + ((int64_t)j0 + k * 256 + (int64_t)lane * 4) * 3);
        const float4 a = p[0], b = p[1], c = p[2];  // x0 y0 z0 x1 | y1 z1 x2 y2 | z2 x3 y3 z3
        st.x[k][0][0] = f32x2{a.x, a.w}; st.x[k][0][1] = f32x2{a.y, b.x};
        st.x[k][0][2] = f32x2{a.z, b.y};
        st.x[k][1][0] = f32x2{b.z, c.y}; st.x[k][1][1] = f32x2{b.w, c.z};
        st.x[k][1][2] = f32x2{c.x, c.w};
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int c3 = 0; c3 < 3; ++c3) st.g[k][h][c3] = f32x2{0.f, 0.f};
    }
}

__device__ __forceinline__ void store_strip(const StripF32 &st, float *__restrict__ slot,
                                            int lane) {
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        float4 *p = reinterpret_cast<float4 *>(slot + (k * 256 + (int64_t)lane * 4) * 3);
        const auto &g = st.g[k];
        p[0] = make_float4(g[0][0].x, g[0][1].x, g[0][2].x, g[0][0].y);
        p[1] = make_float4(g[0][1].y, g[0][2].y, g[1][0].x, g[1][1].x);
        p[2] = make_float4(g[1][2].x, g[1][0].y, g[1][1].y, g[1][2].y);
    }
}

template <typename T>
__device__ __forceinline__ const typename Traits<T>::Vec *unit_ptr(const T *__restrict__ units,
                                                                   int64_t ul, int lane) {
    using Vec = typename Traits<T>::Vec;
    return reinterpret_cast<const Vec *>(units) + ul * 512 + lane;  // 8 KiB = 512 x 16 B
}

// coordinates of a unit's rows: 3*RPU consecutive elements, one per lane
template <typename T, bool W>
__device__ __forceinline__ T load_xrow(const T *__restrict__ X, int i0, int lane) {
    return X[(int64_t)i0 * 3 + (lane < 3 * Lay<T, W>::RPU ? lane : 0)];
}

// fp64 column-strip state: load k of a row brings columns k*128 + lane*2, +1, so lane l owns
// 6 consecutive coordinates per k.
template <int LPR>
struct StripF64 {
    double xj[LPR][2][3], gc[LPR][2][3];
};
template <int LPR>
__device__ __forceinline__ void load_strip(StripF64<LPR> &st, const double *__restrict__ X, int j0,
                                           int lane) {
#pragma unroll
    for (int k = 0; k < LPR; ++k) {
        const double2 *p =
            reinterpret_cast<const double2 *>(X + ((int64_t)j0 + k * 128 + (int64_t)lane * 2) * 3);
        const double2 a = p[0], b = p[1], c = p[2];
        st.xj[k][0][0] = a.x; st.xj[k][0][1] = a.y; st.xj[k][0][2] = b.x;
        st.xj[k][1][0] = b.y; st.xj[k][1][1] = c.x; st.xj[k][1][2] = c.y;
    }
#pragma unroll
    for (int k = 0; k < LPR; ++k)
#pragma unroll
        for (int c = 0; c < 2; ++c) st.gc[k][c][0] = st.gc[k][c][1] = st.gc[k][c][2] = 0.0;
}
template <int LPR>
__device__ __forceinline__ void store_strip(const StripF64<LPR> &st, double *__restrict__ slot,
                                            int lane) {
#pragma unroll
    for (int k = 0; k < LPR; ++k) {
        double2 *p = reinterpret_cast<double2 *>(slot + ((int64_t)k * 128 + (int64_t)lane * 2) * 3);
        const auto &g = st.gc[k];
        p[0] = make_double2(g[0][0], g[0][1]);
        p[1] = make_double2(g[0][2], g[1][0]);
        p[2] = make_double2(g[1][1], g[1][2]);
    }
}
// An entry of the 24-bit stream's table (stress_grad_kernel, PK): where the unit begins in the
// stream, in 16-byte words, and its base; nothing for a plain descriptor.
__device__ __forceinline__ int64_t pk24_word_offset(const int4 &e) { return (int64_t)(e.z & 0x7fffffff) * 64; }
__device__ __forceinline__ int64_t pk24_word_offset(const int2 &) { return 0; }
__device__ __forceinline__ bool pk24_packed(const int4 &e) { return e.z < 0; }
__device__ __forceinline__ bool pk24_packed(const int2 &) { return false; }
__device__ __forceinline__ unsigned pk24_base(const int4 &e) { return (unsigned)e.w; }
__device__ __forceinline__ unsigned pk24_base(const int2 &) { return 0u; }
// the packed BODY runs a packed unit whose base is not 0 (no zero in it: process_unit_f32); a
// packed unit with base 0 is 6 KiB of zero dwords and goes through the raw body
__device__ __forceinline__ bool pk24_packed_body(const int4 &e) { return e.z < 0 && e.w != 0; }
__device__ __forceinline__ bool pk24_packed_body(const int2 &) { return false; }

// One wave = one contiguous chunk of units; 4 independent waves per workgroup.
// No LDS, no barriers, no atomics: results are bitwise reproducible.
//
// Arguments are separate __restrict__ pointers (not a struct) so that the
// read-only index arrays are provably unclobbered and load through the scalar
// cache.  Unit indices are 32-bit (a rank holds < 2^31 units = 16 TiB).
//   units      this rank's units, 8 KiB (RPU rows x VW columns) each
//   X          (n_pad, 3) coordinates
//   udesc      per local unit {i0, j0}
//   chunk_q/_r units per wave: n_local = n_waves * q + r, the first r waves take q + 1
//   wave_slots per wave {first private column-partial slot, the workgroup's shared slot of
//              the strip the wave ENDS in (-1: the wave has no units)}; see the epilogue
//   rowpart    3*RPU elements per unit, base shifted to the rank's first tile
//   colpart    3*VW elements per slot
//   stresspart one double per wave: the stress of the strip the wave ENDS in
//   stress_slot one double per private column slot: the stress of a strip the wave left
//
// DEFER (fp32 and fp64 wide): the row sums do not leave the wave unit by unit.  Writing 48
// bytes to a fresh line per 8 KiB read costs 7.5 % of the kernel at N=50k, and not in
// issue: a store whose lanes are all out of range is free, so is one that keeps
// hitting the same line, and grouping 16 units into 768-byte bursts changes nothing
// -- the write-back cache decides when dirty lines go to HBM, and it sends them into
// a saturated read stream.  The column partials of the same size cost almost nothing
// because they are written when a wave is done.  So, when a wave's whole chunk of
// row sums fits in LDS (cap_units * 48 B per wave: N=50k on one GPU, every multi-GPU
// share), they are parked there and written out as one contiguous burst when the
// wave has finished reading: -5.8 % kernel time at N=50k.  A longer chunk parks its
// LAST cap_units units and stores the ones before them directly.  A property of the
// layout, not a launch choice: a rank without units (cap_units = 0) parks nothing.
//
// WPB = waves per workgroup.  4: one wave per SIMD and workgroup.  8 (used when a CU
// holds 8 waves): the two waves that share a SIMD -- wave k and k + 4 -- sit in ONE
// workgroup and keep each other's pace.  Left alone, the SIMD's issue arbitration favours
// the older of two co-resident waves on every conflict, and with static, equal chunks
// that adds up: per-wave time stamps have the favoured partner
// finish its chunk 15-25 % before the other, which then runs the tail alone with half the
// bytes in flight.  Each wave posts the number of units it has done in LDS and reads its
// partner's; whoever is behind raises its priority (s_setprio) for the next unit.  The
// results do not depend on any of it: chunks, slots and summation order stay static.
//
// PK (fp32 only): `units` is the rank's 24-bit STREAM (SPEC 3.7) -- the same units in the same
// order, each packed (6 KiB) or raw (8 KiB) -- and `udesc` its int4 table {i0, j0, offset of
// the unit in the stream in KiB | packed << 31, base}, fetched one unit ahead like the
// descriptor it contains.  The inner loop then exists twice, one copy per format, and the
// outer loop makes one trip per (strip, format) run: see the loops below.  Chunks, slots,
// parking and every sum are the same, so are the results, bit for bit.
// With two unit bodies hipcc does not keep the kernel within 128 VGPRs (either body alone
// fits; side by side, in any arrangement of the loops, it spills 400-800 bytes), so PK is
// built for two waves per SIMD (<= 256 VGPRs: stream24_grad_kernel).  The sweep never runs more (waves_per_cu: 4 or 8
// waves per CU), so that costs no occupancy.
// The sweep's body is bb_sweep_body.inc, compiled under two kernels with their own names and
// register budgets: stress_grad_kernel (PK = false: what it always was, instruction for
// instruction) and stream24_grad_kernel (PK = true), below it.
template <typename T, bool W, bool NT, int OP, int WPB>
__global__ __launch_bounds__(64 * WPB, (Lay<T, W>::MIN_WG)) void stress_grad_kernel(
    const T *__restrict__ units, const T *__restrict__ X, const int2 *__restrict__ udesc,
    int chunk_q, int chunk_r, const int2 *__restrict__ wave_slots, T *__restrict__ rowpart,
    T *__restrict__ colpart, double *__restrict__ stresspart, int cap_units, int lds_wave_floats,
    int dense_u0, double *__restrict__ stress_slot) {
    constexpr bool PK = sizeof(T) == 0;   // false, and dependent: what is for PK is not instantiated
#include "bb_sweep_body.inc"
}

// The fp32 sweep over the 24-bit stream: `units` is the stream, `udesc` its int4 table.  Built
// for the waves per SIMD the sweep runs with (waves_per_cu): two in workgroups of 8 waves, one
// in workgroups of 4 -- hipcc takes 256 registers for the two bodies in the first form and 257
// in the second, no scratch (with a bound of two there as well: 256 and one spilled).
// Ranks that share a GPU do not use it (ensure_pk24): their kernels share the wave slots.
// (T = float, W = true only; parameters so that the body's choices by type stay dependent)
template <typename T, bool W, bool NT, int OP, int WPB>
__global__ __launch_bounds__(64 * WPB, (WPB == 8 ? 2 : 1)) void stream24_grad_kernel(
    const T *__restrict__ units, const T *__restrict__ X, const int2 *__restrict__ udesc,
    int chunk_q, int chunk_r, const int2 *__restrict__ wave_slots, T *__restrict__ rowpart,
    T *__restrict__ colpart, double *__restrict__ stresspart, int cap_units, int lds_wave_floats,
    int dense_u0, double *__restrict__ stress_slot) {
    static_assert(sizeof(T) == 4 && W, "the 24-bit stream is fp32 only");
    constexpr bool PK = sizeof(T) == 4;
#include "bb_sweep_body.inc"
}

// --------------------------------------------------------------------------
// reduce (+ update) kernel: one workgroup per vw-bin block
// --------------------------------------------------------------------------
template <typename T>
struct ReduceParams {
    const T *__restrict__ part;              // rowpart | colpart | a chunk of zeros
    const double *__restrict__ stresspart;
    T *__restrict__ X;                       // apply mode
    T *__restrict__ V;                       // apply mode: velocity (heavy-ball momentum)
    T mu;                                    // momentum coefficient, 0 = plain gradient step
    T scale;                                 // 2 for the gradient (SPEC 2.3), 1 for a matvec
    T *__restrict__ exch;                    // exchange mode: [3*n_pad | hi | lo]
    const PeerTable<T> *__restrict__ peer;   // peer mode: destinations, in device memory
    unsigned *__restrict__ peer_counter;     // peer mode: workgroups done (last one raises flags)
    const PeerState *peer_state;             // peer mode: a failed rank pushes nothing
    unsigned long long seq;                  // peer mode: value the flags take
    int n_peers;
    double *__restrict__ stress_out;         // apply / stress-only: where the stress goes
    int64_t n_pad;
    int n_waves;
    int mode;
    T lr;
    const double *__restrict__ stress_slot;  // per private column slot (see the sweep)
    int n_slots;
    // a step per bin (bb_solver_set_bin_steps / _block_steps; bb_solver_set_maps: the map's):
    // the gradient of bin i leaves the reduce as bin_scale[i] * g_i -- into the update, the
    // exchange buffer or the peers' arenas alike, so every rank and every later kernel steps
    // with the one uniform lr (nullptr for a plain sum: the matvec).  Several maps
    // (world = 1): the stress is folded per map -- map m's partials are
    // map_idx[map_ptr[m] .. map_ptr[m + 1]) (index < n_waves: stresspart, else stress_slot) --
    // into stress_out[m].  n_maps <= 1: one map, every partial, stress_out[0].
    const T *__restrict__ bin_scale;        // n_pad factors (element o of X belongs to bin o / 3)
    // peer exchange: which ranks hold units that touch block b (bit r of peer_mask[b]; the same
    // table on every rank, from the tile list and the partition).  A rank outside a block's
    // mask has nothing but zeros for it: it does not push them, and nobody waits for or adds
    // its slot.  nullptr: every rank, every block (BB_PEER_MASK=0).
    const unsigned *__restrict__ peer_mask;
    int rank;
    const int *__restrict__ map_ptr;
    const int *__restrict__ map_idx;
    int n_maps;
};

// this thread's share of map `m`'s stress partials (stride = threads of the workgroup)
template <typename T>
__device__ __forceinline__ double stress_share(const ReduceParams<T> &p, int m, int tid, int stride) {
    double s = 0.0;
    if (p.n_maps <= 1) {
        for (int i = tid; i < p.n_waves; i += stride) s += p.stresspart[i];
        for (int i = tid; i < p.n_slots; i += stride) s += p.stress_slot[i];
    } else {
        for (int i = p.map_ptr[m] + tid; i < p.map_ptr[m + 1]; i += stride) {
            const int idx = p.map_idx[i];
            s += idx < p.n_waves ? p.stresspart[idx] : p.stress_slot[idx - p.n_waves];
        }
    }
    return s;
}

constexpr int kRedWG = 128;  // elements a reduce workgroup sums

// ---- the reduce in ONE launch of one memory round trip (round 3) ------------------
// Round 2's reduce walked a block's list with one thread per element: a list of L chunks was
// ceil(L / 16) dependent round trips behind three more (kernel arguments -> list pointer ->
// list), and lists beyond 128 chunks took a second launch.  The kernel trace had that
// chain at 6.2-7.4 us per iteration from N=8,000 to 17,700 and 11-13 us at N=24,926 -- 6 % of
// a 1/8 share of N=50k.  Here a workgroup is 128 elements x S slices of the list (S = 4 or
// 8): every thread has its whole slice -- 16 chunks per trip -- in flight at once, the
// slices meet in LDS and are added in slice order (fixed: bitwise reproducible), and the
// lists come as ONE table of fixed stride (`list_stride` entries per block, padded with the
// offset of a chunk of zeros), so the table's address does not wait for a list pointer and no
// load is predicated.  A wave is one slice of 64 elements: its table entries are
// wave-uniform and travel through the scalar cache.
// slice sl of block b's list, summed for element e in list order, 16 chunks per trip in flight
template <int S, typename T>
__device__ __forceinline__ T list_slice_sum(const T *__restrict__ part, const int64_t *__restrict__ lists,
                                            int list_stride, int b, int sl, int e) {
    const int lps = list_stride / S;                              // a multiple of 16
    const int64_t *list = lists + (int64_t)b * list_stride + (int64_t)sl * lps;
    T acc = T(0);
    for (int k = 0; k < lps; k += 16) {
        T v[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) v[q] = part[list[k + q] + e];
#pragma unroll
        for (int q = 0; q < 16; ++q) acc += v[q];
    }
    return acc;
}
// the S slices of element el, where they met in LDS, added in slice order
template <int S, typename T>
__device__ __forceinline__ T slices_total(const T (&meet)[S][kRedWG], int el) {
    T tot = meet[0][el];
#pragma unroll
    for (int q = 1; q < S; ++q) tot += meet[q][el];
    return tot;
}
// the gradient element o from the total of its partials: times scale (2, SPEC 2.3; 1 for a
// matvec) and the bin's step factor (ReduceParams::bin_scale)
template <typename T>
__device__ __forceinline__ T gradient_element(const ReduceParams<T> &p, int64_t o, T tot) {
    return p.bin_scale ? p.bin_scale[o / 3] * (p.scale * tot) : p.scale * tot;
}

template <typename T, bool W, int S>
__global__ __launch_bounds__(128 * S) void reduce_sliced_kernel(ReduceParams<T> p,
                                                                const int64_t *__restrict__ lists,
                                                                int list_stride) {
    constexpr int CH = 3 * Lay<T, W>::VW;
    static_assert(CH % kRedWG == 0, "3*vw is a multiple of 128");
    const int tid = threadIdx.x;
    const int el = tid & (kRedWG - 1);
    const int sl = __builtin_amdgcn_readfirstlane(tid >> 7);      // slice: uniform per wave
    const int b = blockIdx.x;
    const int e = (int)blockIdx.y * kRedWG + el;                  // element of the block, < CH
    __shared__ __attribute__((aligned(16))) T meet[S][kRedWG];
    const bool peer_live =
        p.mode != kReducePeer ||
        __hip_atomic_load(&p.peer_state->status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0;
    if (p.mode != kReduceStressOnly) {
        const int64_t o = (int64_t)b * CH + e;
        T xo = T(0), vo = T(0);
        if (p.mode == kReduceApply && sl == 0) { xo = p.X[o]; vo = p.V[o]; }   // early: independent
        meet[sl][el] = list_slice_sum<S>(p.part, lists, list_stride, b, sl, e);
        __syncthreads();
        if (sl == 0) {
            const T g = gradient_element(p, o, slices_total(meet, el));
            if (p.mode == kReduceApply) {
                momentum_step(p.X, p.V, o, xo, vo, p.mu, p.lr, g);
            } else if (p.mode == kReducePeer) {
                meet[0][el] = g;
            } else {
                p.exch[o] = g;
            }
        }
        if (p.mode == kReducePeer && peer_live) {
            typedef T vec_t __attribute__((ext_vector_type(16 / sizeof(T))));
            constexpr int NV = kRedWG * (int)sizeof(T) / 16;
            __syncthreads();
            if (tid < NV && (p.peer_mask == nullptr || (p.peer_mask[b] >> p.rank & 1u))) {
                const vec_t val = ((const vec_t *)meet[0])[tid];
                for (int q = 0; q < p.n_peers; ++q)
                    ((vec_t *)(p.peer->dst[q] + (int64_t)b * CH + (int64_t)blockIdx.y * kRedWG))[tid] = val;
            }
        }
    }
    if (b < (p.n_maps > 1 ? p.n_maps : 1) && blockIdx.y == 0) {
        // the stress: per-wave and per-slot partials of the sweep, fixed tree
        __shared__ double sh[128 * S];
        sh[tid] = stress_share(p, b, tid, 128 * S);
        __syncthreads();
        lds_tree_fold(sh, tid, 128 * S);
        if (tid == 0) {
            const double Sx = sh[0];
            T hi, lo;
            split_hi_lo(Sx, hi, lo);
            if (p.mode == kReduceExchange) {
                p.exch[3 * p.n_pad] = hi;
                p.exch[3 * p.n_pad + 1] = lo;
            } else if (p.mode == kReducePeer) {
                for (int q = 0; q < (peer_live ? p.n_peers : 0); ++q) {
                    p.peer->dst[q][3 * p.n_pad] = hi;
                    p.peer->dst[q][3 * p.n_pad + 1] = lo;
                }
            } else {
                p.stress_out[b] = Sx;
            }
        }
    }
    if (p.mode == kReducePeer && peer_live) {
        // Every workgroup makes its stores visible system-wide and checks in; the last one
        // raises this rank's flag on every peer (release).  ONE lane fences for the
        // workgroup, behind a barrier that every storing wave reaches with its stores
        // acknowledged (__syncthreads() waits vmcnt(0)): a release is a write-back of the
        // XCD's L2, and with all 16 waves of the workgroup issuing one the push cost 33 us
        // instead of 12 (tools/exchange_timing.py).
        // The wait is spelled out in EVERY storing wave: that __syncthreads() emits one is a
        // code-generation detail (the memory model lets a workgroup-scope release omit it), and
        // a flag that overtakes the data would make a peer sum stale partials silently.  It
        // costs nothing: no cache write-back, and the barrier waits for the slowest wave anyway.
        __shared__ int last;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (tid == 0) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");   // system scope
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // (the compiler may drop its own)
            // two levels: the gridDim.y workgroups of a block check in on the block's own
            // counter (its own 128-byte line), the last of them on the top counter -- 12 + 35
            // adds in a row instead of 420 on one word (11-13 ns each) at a 1/8 share of N=50k
            unsigned *mine = p.peer_counter + 32 * (b + 1);
            last = 0;
            if (atomicAdd(mine, 1u) == gridDim.y - 1) {
                atomicExch(mine, 0u);
                last = atomicAdd(p.peer_counter, 1u) == gridDim.x - 1;
            }
        }
        __syncthreads();
        if (last) {
            if (tid == 0) atomicExch(p.peer_counter, 0u);
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            if (tid < p.n_peers)
                __hip_atomic_store(p.peer->flag[tid], p.seq, __ATOMIC_RELEASE,
                                   __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}

// ---- the peer exchange in ONE launch: reduce, push, wait, sum, update (round 3) --------
// reduce_sliced_kernel in peer mode + peer_receive_kernel are two launches with a check-in of
// every workgroup in between (release fence, two atomic counters, the last arriver raises
// the rank's flag), and the receiving launch has one wave wait for the flags of all ranks
// before any of its workgroups may move: 10 + 6.6 us at a 1/8 share of N=50,000 against
// 5.1 us for the reduce that applies its own sum (kernel trace of tools/exchange_timing.py).
// Here the unit of exchange is what a workgroup reduces anyway -- 128 gradient elements of
// one block -- and the two waves that hold those sums see them through: each thread stores
// its element into its rank's slot on every peer, then reads the same element of every
// rank's slot in its own arena until all of them have ARRIVED, adds them in rank order,
// updates its coordinate and marks the words it consumed as empty again.
//   No flags, no fences: a word says by itself whether it has arrived.  An empty slot word
// holds kPeerEmpty -- all bits set, a NaN no arithmetic produces (the sender turns a sum that
// should ever carry those bits into the canonical NaN) -- and a 4- or 8-byte store is seen
// whole or not at all; nothing else is published with it, so nothing has to be ordered
// against it: relaxed system-scope stores and loads on uncached memory, one round trip from
// "the peer's store has landed" to "the sum is known".  The slots start out empty
// (bb_solver_peer_export), a consumer empties what it has read, and with two parities a
// word is written again only two exchanges later, by a sender that has seen this rank's NEXT
// push -- issued a whole launch after the emptying store.
//   Nobody waits for anybody's slowest workgroup but the owners of the same 64 elements.
// Progress: workgroups are dispatched in index order and each pushes BEFORE it waits, so the
// lowest unfinished index is resident (or next in line) on every rank and has pushed
// wherever it is resident: it completes everywhere, frees its slot, and so on.  That needs
// each rank's GPU to itself (the product's model: one process per GPU); ranks SHARING one
// device can fill its wave slots and LDS with waiting workgroups while the rank they wait for
// still sweeps -- bb_solver_peer_connect keeps the two-launch form then (BB_PEER_FUSED).
//   Failure: a wait that runs into the time limit, a peer's poison word, or this rank's own
// sticky status end the wave without an update; it sets the status, leaves the poison word
// on every peer, and every wave still waiting -- here and there -- leaves within a poll.
// Unlike the two-launch form this one can fail PARTIALLY (some 64-element pieces of the
// step applied, others not): the status is sticky, bb_solver_peer_status reports it, and the
// coordinates of a failed solver are not a result.
// (What a slot word says -- peer_word_empty, peer_sendable -- and a wave's bounded wait for the
// words of every rank, peer_wait_sum: bb_peer_kernels.h.)
template <typename T, bool W, int S>
__global__ __launch_bounds__(128 * S) void reduce_exchange_kernel(
    ReduceParams<T> p, const int64_t *__restrict__ lists, int list_stride,
    const PeerTableX<T> *__restrict__ xt, const T *arena, const unsigned long long *my_poison,
    int64_t slot_elems, PeerState *state, long long limit) {
    constexpr int CH = 3 * Lay<T, W>::VW;
    const int tid = threadIdx.x;
    const int el = tid & (kRedWG - 1);
    const int sl = __builtin_amdgcn_readfirstlane(tid >> 7);      // slice: uniform per wave
    const int b = blockIdx.x;
    const int e = (int)blockIdx.y * kRedWG + el;                  // element of the block, < CH
    const int R = p.n_peers;
    __shared__ __attribute__((aligned(16))) T meet[S][kRedWG];
    __shared__ double sh[128 * S];
    // a failed rank pushes nothing and leaves X alone (its peers have its poison word);
    // ONE thread asks, the first barrier below tells the others: the word can change under us
    const int dead_here =
        tid == 0 ? __hip_atomic_load(&state->status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;

    const int64_t o = (int64_t)b * CH + e;
    T xo = T(0), vo = T(0);
    if (sl == 0) { xo = p.X[o]; vo = p.V[o]; }                    // early: independent
    meet[sl][el] = list_slice_sum<S>(p.part, lists, list_stride, b, sl, e);
    const bool first = b == 0 && blockIdx.y == 0;
    if (first)                                // the stress: the sweep's partials, fixed tree
        sh[tid] = stress_share(p, 0, tid, 128 * S);
    if (__syncthreads_or(dead_here) != 0) return;
    if (first) lds_tree_fold(sh, tid, 128 * S);
    if (sl == 0) {
        // the two waves that own the workgroup's 128 elements: push, wait, sum, update
        const T mine = peer_sendable(gradient_element(p, o, slices_total(meet, el)));
        const unsigned mask = p.peer_mask ? p.peer_mask[b] : ~0u;
        if (mask >> p.rank & 1u)
            for (int q = 0; q < R; ++q)
                __hip_atomic_store(xt->dst[q] + o, mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        T g;
        double unused;
        if (peer_wait_sum<T, 1>(arena + o, true, R, slot_elems, xt, my_poison, state, limit, g, unused, mask)) {
            // g = the sum over ranks in rank order
            momentum_step(p.X, p.V, o, xo, vo, p.mu, p.lr, g);
        }
    } else if (first && tid >= 128 && tid < 192) {
        // the stress travels the same way, as a pair (hi, lo) behind the 3 * n_pad elements:
        // one lane of a wave that has nothing else to do
        const bool lane0 = tid == 128;
        const int64_t n3 = 3 * p.n_pad;
        if (lane0) {
            T hi, lo;
            split_hi_lo(sh[0], hi, lo);
            for (int q = 0; q < R; ++q) {
                __hip_atomic_store(xt->dst[q] + n3, peer_sendable(hi), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                __hip_atomic_store(xt->dst[q] + n3 + 1, peer_sendable(lo), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            }
        }
        T unused;
        double Sx;
        if (peer_wait_sum<T, 2>(arena + n3, lane0, R, slot_elems, xt, my_poison, state, limit, unused, Sx) && lane0) {
            *p.stress_out = Sx;
            __hip_atomic_store(&state->verdict, p.seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

template <typename T>
__global__ __launch_bounds__(256) void apply_kernel(T *__restrict__ X, T *__restrict__ V,
                                                    const T *__restrict__ exch, int64_t n3, T lr,
                                                    T mu, double *stress_out) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e < n3) momentum_step(X, V, e, mu, lr, exch[e]);
    if (e == 0 && stress_out) *stress_out = (double)exch[n3] + (double)exch[n3 + 1];
}

// --------------------------------------------------------------------------
// row-owner path: small maps, one launch per iteration
// --------------------------------------------------------------------------
// For a map whose whole symmetric matrix stays in the caches (N up to a few thousand
// bins: chr21 at 50 kb is 963) the unit sweep above is launch-bound -- three dependent
// launches per iteration, two of them only to add up partial sums.  Here BOTH
// triangles are stored (`full`, n rows of `ld` elements, ld a multiple of 128, zero
// = no constraint, zero diagonal) and one wave owns one bin i: it reads row i and the
// coordinates X_k of every bin, so g_i is complete inside the wave -- no partial sums,
// no reduce launch, no atomics, and a fixed summation order.  X_{k+1} goes to a second
// buffer (the other waves are still reading X_k), so one launch is one iteration.
// Every pair is evaluated twice (once from each end), which at these sizes is cheaper
// than the two extra launches it saves.
//
// Stress: S(X_k) = 1/2 sum_i sum_j res_ij^2.  Each workgroup leaves the sum over its
// four rows in part_out[block]; the fold is done by ONE extra workgroup of the NEXT
// launch (blockIdx = gridDim - 1; it runs beside that launch's row workgroups) and by a
// fold-only launch after the last iteration of a bb_solver_iterate call.
// Q = weight power of SPEC 2.3.1 (0: unweighted)
template <typename T, int Q>
__device__ __forceinline__ void pair_row(T delta, T xi, T yi, T zi, T xj, T yj, T zj, T &gx,
                                         T &gy, T &gz, T &s) {
    const T dx = xi - xj, dy = yi - yj, dz = zi - zj;
    const T d2 = fma(dx, dx, fma(dy, dy, fma(dz, dz, Traits<T>::eps2())));  // SPEC 2.2
    T rinv, dist;
    if constexpr (sizeof(T) == 4) {
        rinv = __builtin_amdgcn_rsqf(d2);
        dist = d2 * rinv;
    } else {
        rsqrt_sqrt_f64(d2, rinv, dist);      // as pair_step<double>
    }
    T res;
    if constexpr (sizeof(T) == 4)
        res = delta > T(0) ? dist - delta : T(0);
    else
        res = fma(dist, weight01_f64(delta), -delta);        // as pair_step<double>
    if constexpr (Q > 0) {
        // SPEC 2.3.1: r = 1/delta, 0 where delta = 0 (res is 0 there too)
        T r;
        if constexpr (sizeof(T) == 4)
            r = delta > T(0) ? __builtin_amdgcn_rcpf(delta) : T(0);
        else
            r = rcp_f64(delta + (1.0 - weight01_f64(delta))) * weight01_f64(delta);
        const T u = res * r;
        T coef;
        if constexpr (Q == 1) {
            s = fma(res, u, s);
            coef = u * rinv;
        } else {
            s = fma(u, u, s);
            coef = (u * r) * rinv;
        }
        gx = fma(coef, dx, gx);
        gy = fma(coef, dy, gy);
        gz = fma(coef, dz, gz);
        return;
    }
    s = fma(res, res, s);
    const T coef = res * rinv;
    gx = fma(coef, dx, gx);
    gy = fma(coef, dy, gy);
    gz = fma(coef, dz, gz);
}

// columns per loop trip of a wave: one 16-byte load per lane = 4 (fp32) / 2 (fp64) columns.
// Round 4: per pair the kernel issued one 4-byte (8-byte) load of the matrix and three scalar
// loads of the partner's coordinates.  A lane now takes 4 (2) CONSECUTIVE columns: one 16-byte
// load of the row and three 16-byte loads of the 12 (6) contiguous coordinates of those
// columns -- one load per pair (two in fp64) instead of four: fp64 -9 % at N=963, -12 % at
// 2,500, -19 % at 4,096 (28.4 -> 23.0 us); fp32 -4 % at 2,500, -8 % at 4,096
// (profiles/r04_row_owner_ab.txt, measured against the old trip).
// Packed fp32 pair math on top of it (v_pk_* straight on the AoS register pairs) changed
// nothing: from N ~ 4,000 the kernel moves both triangles at ~5 TB/s and that is its bound.
template <typename T> struct RowTrip { static constexpr int COLS = 64 * (16 / (int)sizeof(T)); };

// WPR waves share one row (1, 2 or 4: the host picks it so that a small map still
// puts >= 16 waves on every CU): wave part p takes the 128-column trips p, p + WPR, ...;
// the parts meet in LDS and are added in part order by the row's first wave.
template <typename T, int WPR, int Q>
__global__ __launch_bounds__(256) void row_owner_kernel(
    const T *__restrict__ full, int64_t ld, int n, const T *__restrict__ Xin,
    T *__restrict__ Xout, T *__restrict__ V, T lr, T mu, const double *__restrict__ part_prev,
    int n_prev, double *__restrict__ hist_prev, double *__restrict__ part_out,
    const T *__restrict__ bin_scale) {
    constexpr int ROWS = 4 / WPR;                 // rows per workgroup
    __shared__ double sh[256];
    __shared__ T red[4][4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (blockIdx.x == gridDim.x - 1) {
        // the fold workgroup: stress of the PREVIOUS launch, fixed order
        if (hist_prev == nullptr) return;
        double a = 0.0;
        for (int q = tid; q < n_prev; q += 256) a += part_prev[q];
        sh[tid] = a;
        __syncthreads();
        lds_tree_fold(sh, tid, 256);
        if (tid == 0) *hist_prev = 0.5 * sh[0];
        return;
    }
    const int i = blockIdx.x * ROWS + wv / WPR;
    const int part = wv % WPR;
    T s = T(0), gx = T(0), gy = T(0), gz = T(0);
    T xi = T(0), yi = T(0), zi = T(0);
    if (i < n) {
        xi = Xin[3 * (int64_t)i]; yi = Xin[3 * (int64_t)i + 1]; zi = Xin[3 * (int64_t)i + 2];
        const T *row = full + (int64_t)i * ld;
        constexpr int COLS = RowTrip<T>::COLS;
        const int trips = ((int)(ld / COLS) - part + WPR - 1) / WPR;   // trips part, part + WPR, ...
        auto trip = [&](int tr) __attribute__((always_inline)) {
            using Vec = typename Traits<T>::Vec;
            const int c = (part + tr * WPR) * COLS + lane * Traits<T>::VPL;
            const Vec dv = *reinterpret_cast<const Vec *>(row + c);
            const Vec *px = reinterpret_cast<const Vec *>(Xin + 3 * (int64_t)c);
            const Vec a = px[0], b = px[1], q = px[2];
            if constexpr (sizeof(T) == 4) {      // x0 y0 z0 x1 | y1 z1 x2 y2 | z2 x3 y3 z3
                pair_row<T, Q>(dv.x, xi, yi, zi, a.x, a.y, a.z, gx, gy, gz, s);
                pair_row<T, Q>(dv.y, xi, yi, zi, a.w, b.x, b.y, gx, gy, gz, s);
                pair_row<T, Q>(dv.z, xi, yi, zi, b.z, b.w, q.x, gx, gy, gz, s);
                pair_row<T, Q>(dv.w, xi, yi, zi, q.y, q.z, q.w, gx, gy, gz, s);
            } else {                             // x0 y0 | z0 x1 | y1 z1
                pair_row<T, Q>(dv.x, xi, yi, zi, a.x, a.y, b.x, gx, gy, gz, s);
                pair_row<T, Q>(dv.y, xi, yi, zi, b.y, q.x, q.y, gx, gy, gz, s);
            }
        };
        // fp32: 4 trips (8 pairs per lane) in flight; fp64: unrolling costs more in
        // registers than it hides (N=2,500: 18.3 us per iteration unrolled, 14.4 rolled)
        if constexpr (sizeof(T) == 4) {
#pragma unroll 4
            for (int tr = 0; tr < trips; ++tr) trip(tr);
        } else {
#pragma nounroll
            for (int tr = 0; tr < trips; ++tr) trip(tr);
        }
        wave_sum_hi3(gx, gy, gz);
        s = wave_sum_hi(s);
    }
    if constexpr (WPR > 1) {
        if (lane == 63) { red[wv][0] = gx; red[wv][1] = gy; red[wv][2] = gz; red[wv][3] = s; }
        __syncthreads();
        if (part == 0 && lane == 63) {
#pragma unroll
            for (int p = 1; p < WPR; ++p) {
                gx += red[wv + p][0]; gy += red[wv + p][1]; gz += red[wv + p][2];
                s += red[wv + p][3];
            }
        }
    }
    if (i < n && part == 0 && lane == 63) {
        // SPEC 2.3 / 2.4: g = 2 * sum (2.4.1: times the bin's factor); V <- mu V - lr g; X <- X + V
        const int64_t o = 3 * (int64_t)i;
        T g0 = T(2) * gx, g1 = T(2) * gy, g2 = T(2) * gz;
        if (bin_scale) {
            const T c = bin_scale[i];
            g0 = c * g0; g1 = c * g1; g2 = c * g2;
        }
        const T vx = momentum_velocity(mu, V[o], lr, g0);
        const T vy = momentum_velocity(mu, V[o + 1], lr, g1);
        const T vz = momentum_velocity(mu, V[o + 2], lr, g2);
        V[o] = vx; V[o + 1] = vy; V[o + 2] = vz;
        Xout[o] = xi + vx; Xout[o + 1] = yi + vy; Xout[o + 2] = zi + vz;
    }
    if (lane == 63) sh[wv] = (part == 0 && i < n) ? (double)s : 0.0;
    __syncthreads();
    if (tid == 0) part_out[blockIdx.x] = (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

// --------------------------------------------------------------------------
// The 24-bit stream of the fp32 sweep (SPEC 3.7): built from the units once per map
// --------------------------------------------------------------------------
// One workgroup per unit: the smallest and the largest of its 2,048 stored words, as uint32.
__global__ __launch_bounds__(256) void pk24_minmax_kernel(const uint4 *__restrict__ units,
                                                          uint2 *__restrict__ minmax) {
    __shared__ unsigned lo_s[4], hi_s[4];
    const uint4 *p = units + (int64_t)blockIdx.x * 512 + threadIdx.x;
    const uint4 a = p[0], b = p[256];
    unsigned lo = min(min(min(a.x, a.y), min(a.z, a.w)), min(min(b.x, b.y), min(b.z, b.w)));
    unsigned hi = max(max(max(a.x, a.y), max(a.z, a.w)), max(max(b.x, b.y), max(b.z, b.w)));
    for (int o = 32; o > 0; o >>= 1) {
        lo = min(lo, (unsigned)__shfl_xor((int)lo, o));
        hi = max(hi, (unsigned)__shfl_xor((int)hi, o));
    }
    if ((threadIdx.x & 63) == 0) lo_s[threadIdx.x >> 6] = lo, hi_s[threadIdx.x >> 6] = hi;
    __syncthreads();
    if (threadIdx.x == 0)
        minmax[blockIdx.x] = make_uint2(min(min(lo_s[0], lo_s[1]), min(lo_s[2], lo_s[3])),
                                        max(max(hi_s[0], hi_s[1]), max(hi_s[2], hi_s[3])));
}

// One workgroup per unit: its place in the stream from the table ({., ., KiB offset | packed
// << 31, base}); a raw unit is copied, a packed one written in the layout process_unit_f32
// decodes -- dword c of lane l of load L (0..5) holds the code of word L*256 + 4l + c and, on
// top, byte kPk24Byte[L] of the code of the row-3 word of load kPk24Load[L].
__global__ __launch_bounds__(256) void pk24_pack_kernel(const uint4 *__restrict__ units,
                                                        const int4 *__restrict__ table,
                                                        uint4 *__restrict__ stream) {
    const int4 e = table[blockIdx.x];
    const uint4 *src = units + (int64_t)blockIdx.x * 512;
    uint4 *dst = stream + (int64_t)(e.z & 0x7fffffff) * 64;
    const int t = threadIdx.x;
    if (e.z >= 0) {
        dst[t] = src[t];
        dst[t + 256] = src[t + 256];
        return;
    }
    const unsigned base = (unsigned)e.w;
    // thread t packs lane l = t & 63 of loads L = t >> 6 (0..3) and, t < 128, L + 4
    for (int L = t >> 6; L < 6; L += 4) {
        const int l = t & 63;
        const int k3 = L < 3 ? 0 : 1;                       // kPk24Load
        const int sh = 8 * (L < 3 ? L : (L == 3 ? 2 : L - 4));   // 8 * kPk24Byte
        const uint4 w = src[L * 64 + l], r3 = src[(6 + k3) * 64 + l];
        dst[L * 64 + l] = make_uint4((w.x - base) | ((((r3.x - base) >> sh) & 0xffu) << 24),
                                     (w.y - base) | ((((r3.y - base) >> sh) & 0xffu) << 24),
                                     (w.z - base) | ((((r3.z - base) >> sh) & 0xffu) << 24),
                                     (w.w - base) | ((((r3.w - base) >> sh) & 0xffu) << 24));
    }
}

template <typename T>
__global__ void f64_to_T_kernel(const double *__restrict__ in, T *__restrict__ out, int64_t n) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e < n) out[e] = (T)in[e];
}
template <typename T>
__global__ void T_to_f64_kernel(const T *__restrict__ in, double *__restrict__ out, int64_t n) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e < n) out[e] = (double)in[e];
}

}  // namespace
