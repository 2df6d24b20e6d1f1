// bb_sweep_body.inc -- the body of the sweep kernels of bb_solver_kernels.h (stress_grad_kernel,
// stream24_grad_kernel), which include it with T, W, NT, OP, WPB and PK in scope and the
// parameters named as there.  Not a translation unit of its own.
    using Vec = typename Traits<T>::Vec;
    constexpr int VW = Lay<T, W>::VW;
    constexpr bool DEFER = sizeof(T) == 4 || W;
    const int lane = threadIdx.x & 63;
    const int wib = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // wave in workgroup
    // workgroup b sweeps the b-th run of WPB chunks (permuting that map by XCD changed
    // nothing: docs/EXPERIMENTS.md)
    const int wg = (int)blockIdx.x;
    const int w = wg * WPB + wib;
    // wave w owns units [w*q + min(w, r), +q (+1 if w < r)): arithmetic, not a table --
    // one dependent memory round trip less before the wave's first matrix load
    const int ua = w * chunk_q + (w < chunk_r ? w : chunk_r);
    const int ub = ua + chunk_q + (w < chunk_r ? 1 : 0);
    double stress = 0.0;
    // the shared column slots of this workgroup's waves (epilogue), read NOW: behind the
    // fences further down the compiler no longer takes them through the scalar cache, and a
    // vector load there waits -- vmcnt is in order -- for every store the wave has in flight
    int ws_shared[WPB];
#pragma unroll
    for (int k = 0; k < WPB; ++k) ws_shared[k] = wave_slots[(int64_t)wg * WPB + k].y;
    // DEFER: this wave's parking space, cap_units * 12 floats + 4 dummy words
    extern __shared__ __attribute__((aligned(16))) float row_lds[];
    // this wave's LDS region: row-sum parking while it sweeps, its last column partial at
    // the end (lds_wave_floats >= cap_units * 12 + 4 and >= 3 * VW elements of T)
    const int stage0 = wib * lds_wave_floats;
    // WPB = 8: progress words of the 8 waves, behind the regions
    int *progress = reinterpret_cast<int *>(row_lds + WPB * lds_wave_floats);
    int partner_done = 0;
    const int park_from = (ub - ua) > cap_units ? (ub - ua) - cap_units : 0;
    // fp64 2 x 512 units: column selectors of the MFMA row reduction (process_unit_f64w)
    double sel[6];
#pragma unroll
    for (int v = 0; v < 6; ++v) sel[v] = (lane & 15) == v ? 1.0 : 0.0;

    if (ua < ub) {
        int slot = wave_slots[w].x;
        Vec d[8];  // the unit's 8 wave-loads (8 KiB), in memory order
        // column-strip state: coordinates + gradient accumulators of this lane's columns
        using Strip = typename std::conditional<sizeof(T) == 4, StripF32,
                                                StripF64<Lay<T, W>::LPR>>::type;
        Strip st;
        // (closures on purpose: with load_strip / store_strip called directly at the two sites
        // hipcc allocates the registers of 18 of the 40 instantiations differently, three words
        // of scratch in the fp32 weighted ones -- tools/kernel_resources.sh --digest)
        auto strip_load = [&](int j0) __attribute__((always_inline)) { load_strip(st, X, j0, lane); };
        auto strip_store = [&](int sl) __attribute__((always_inline)) {
            store_strip(st, colpart + (int64_t)sl * (3 * VW), lane);
        };

        // The wave's FIRST unit stands between the kernel's arguments and its first
        // coordinate loads: a cold descriptor load there is one more dependent memory round
        // trip (0.8 us of every launch).  A dense layout (dense_u0 >= 0: this rank's first
        // global unit) has tile t = J (J + 1) / 2 + I in strip-major order (SPEC 3.1,
        // bb_layout_dense_tiles), so that descriptor is arithmetic; the later ones come from
        // the table as before, one unit ahead of their use.
        using Desc = typename std::conditional<PK, int4, int2>::type;
        const Desc *__restrict__ const table = reinterpret_cast<const Desc *>(udesc);
        Desc dc;
        if (dense_u0 >= 0) {
            constexpr int UPT = VW / Lay<T, W>::RPU;
            const unsigned g = (unsigned)dense_u0 + (unsigned)ua;
            const unsigned t = g / UPT, sub = g % UPT;
            unsigned J = (unsigned)((__builtin_sqrtf(8.0f * (float)t + 1.0f) - 1.0f) * 0.5f);
            while (J * (J + 1) / 2 > t) --J;
            while ((J + 1) * (J + 2) / 2 <= t) ++J;
            const unsigned I = t - J * (J + 1) / 2;
            if constexpr (PK) {
                dc = table[ua];     // (where the unit lies in the stream is no arithmetic)
                dc.x = (int)(I * VW + sub * Lay<T, W>::RPU), dc.y = (int)(J * VW);
            } else {
                dc = make_int2((int)(I * VW + sub * Lay<T, W>::RPU), (int)(J * VW));
            }
        } else {
            dc = table[ua];                                    // current unit
        }
        Desc dn = table[ua + 1 < ub ? ua + 1 : ua];            // next unit
        // Prologue: the x rows of the first unit, then its 8 matrix rows.
        // Row coordinates of a unit, one unit ahead.  XRowS: 3*RPU wave-uniform scalars
        // fetched through the scalar cache (X is read-only in this kernel) -- no VMEM
        // slot, no v_readlane (fp64 wide, 6 doubles: 12 SGPRs, double-buffered).
        // XRowS32 (fp32, 12 floats): six scalar pairs that the subtracts read as they are, ONE
        // set of 12 SGPRs -- the unit body loads the next unit's over them row by row
        // (xrow_refresh), so after a unit xr holds the rows of the descriptor that was `dn`.
        // XRowV (fp64 narrow: 24 doubles): one per-lane load, v_readlane per use.
        struct XRowS {
            T v[3 * Lay<T, W>::RPU];
            __device__ __forceinline__ T get(int q) const { return v[q]; }
        };
        struct XRowV {
            T v;
            __device__ __forceinline__ T get(int q) const { return lane_value(v, q); }
        };
        using XRow = typename std::conditional<
            sizeof(T) == 4, XRowS32,
            typename std::conditional<Lay<T, W>::SCALAR_XROW, XRowS, XRowV>::type>::type;
        // fp32: a unit's rows begin at a multiple of 4 bins, 48 bytes: the pairs are aligned
        auto xrow_pairs = [&](int i0) __attribute__((always_inline)) {
            return reinterpret_cast<const f32x2 *>(X + (int64_t)i0 * 3);
        };
        auto xrow_load = [&](int i0) __attribute__((always_inline)) {
            XRow x;
            if constexpr (std::is_same<XRow, XRowS32>::value) {
                const f32x2 *px = xrow_pairs(i0);
#pragma unroll
                for (int q = 0; q < 6; ++q) x.p[q] = px[q];
            } else if constexpr (std::is_same<XRow, XRowS>::value) {
                const T *px = X + (int64_t)i0 * 3;
#pragma unroll
                for (int q = 0; q < 3 * Lay<T, W>::RPU; ++q) x.v[q] = px[q];
            } else {
                x.v = load_xrow<T, W>(X, i0, lane);
            }
            return x;
        };
        XRow xr = xrow_load(dc.x);
        // fp32: a scalar base and the lane's byte offset (WinBase32); fp64: a pointer per lane
        using Win = typename std::conditional<sizeof(T) == 4, WinBase32, WinPtr<Vec>>::type;
        [[maybe_unused]] const unsigned lane_off = (unsigned)lane * 16u;
        auto window_of = [&](int u_next) __attribute__((always_inline)) {
            // The refills of the wave's LAST unit are never consumed.  They stay in the
            // loop (a branch around them would cost every unit its exact wait counts),
            // but all lanes ask for the same 16 bytes of the chunk's last unit: 8 lines
            // instead of 8 KiB per wave and launch (1.3-2.7 % of the bytes of a 1/8 share
            // of N=50k), back at once, so the epilogue gets the window's registers early.
            const bool real = u_next < ub;
            if constexpr (PK) {
                // dn is the table's entry of u_next, or -- clamped -- of the chunk's last unit
                return Win{units, pk24_word_offset(dn) * 16,
                           real ? lane_off : 0u};
            } else if constexpr (sizeof(T) == 4) {
                return Win{units, (int64_t)(real ? u_next : ub - 1) * 8192,
                           real ? lane_off : 0u};
            } else {
                return Win{unit_ptr<T>(units, real ? u_next : ub - 1, real ? lane : 0)};
            }
        };
        // PK: the window of the CURRENT unit (the prologue, and the two loads a raw run is
        // short of when it begins)
        auto window_here = [&]() __attribute__((always_inline)) {
            if constexpr (sizeof(T) == 4)
                return Win{units, pk24_word_offset(dc) * 16,
                           lane_off};
            else
                return Win{reinterpret_cast<const Vec *>(units) + pk24_word_offset(dc) + lane};
        };
        if constexpr (PK) {
            const Win first = window_here();
#pragma unroll
            for (int r = 0; r < 6; ++r) d[r] = first.template load<NT>(r);
        } else {
            const Win first = window_of(ua);
#pragma unroll
            for (int r = 0; r < 8; ++r) d[r] = first.template load<NT>(r);
        }
        // this wave's row partials: 3*RPU elements per unit of its group's chunk
        constexpr unsigned kRowBytes = 3 * Lay<T, W>::RPU * sizeof(T);
        const __amdgpu_buffer_rsrc_t row_rsrc = __builtin_amdgcn_make_buffer_rsrc(
            rowpart + (int64_t)ua * (3 * Lay<T, W>::RPU), 0, (int)((unsigned)(ub - ua) * kRowBytes),
            0x00020000);

        // fp32: which of a unit's 12 row sums this lane holds after the unit's reduction
        // (row16_sum3: every lane holds one, lanes 0, 4 and 8 of every 16-lane row store it)
        // and what follows from it for the unit's store offset and parking slot
        const int f32_sl12 = swap_rowsum_slot(lane);
        const unsigned f32_voff_lane = swap_rowsum_stores(lane) ? (unsigned)f32_sl12 * 4u : 0x40000000u;
        const int f32_lds_lane = stage0 + f32_sl12;
        auto unit_step = [&](int u, auto packed_body) __attribute__((always_inline)) {
            if constexpr (WPB == 8) {
                // pace keeping (see the kernel's comment): the partner's count was read
                // one unit ago, so nothing here waits on LDS
                const int mine = u - ua;
                if (__builtin_amdgcn_readfirstlane(partner_done) > mine)
                    __builtin_amdgcn_s_setprio(1);
                else
                    __builtin_amdgcn_s_setprio(0);
                __hip_atomic_store(progress + wib, mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                partner_done = __hip_atomic_load(progress + (wib ^ 4), __ATOMIC_RELAXED,
                                                 __HIP_MEMORY_SCOPE_WORKGROUP);
            }
            // (the descriptors of the units behind the wave's last one are never used)
            const int un = u + 1 < ub ? u + 1 : u;
            // (fp32: the unit body fetches them itself, into xr)
            [[maybe_unused]] XRow xrn;
            if constexpr (sizeof(T) != 4) xrn = xrow_load(dn.x);
            const Desc dnn = table[un + 1 < ub ? un + 1 : un];
            // the unit, in the form of <T, W>: where its row sums go, then its math
            const int k = u - ua;
            const bool parked = k >= park_from;
            if constexpr (sizeof(T) == 4) {
                // fp32: every lane holds one of the unit's 12 sums.  Units before
                // park_from are stored directly; the later ones are parked in LDS slot
                // (k - park_from) and their store is dropped (every lane out of range).
                // Per-lane parts are loop constants (f32_voff_lane, f32_lds_lane: below the
                // lambda's captures), per-unit parts scalar: one v_add each per unit.  A store
                // is out of range (dropped) unless the lane is the one that stores its sum AND
                // the unit is not parked: 0x40000000 from either side puts the offset beyond
                // any chunk.  The LDS write of a unit that is stored directly goes to slot 0:
                // the parked units come after it, and the first of them overwrites that slot
                // (LDS operations of one wave execute in program order).  The lanes that hold
                // the same sum write the same bits to the same word.
                const unsigned row_voff =
                    f32_voff_lane + (parked ? 0x40000000u : (unsigned)k * kRowBytes);
                const int stage_slot = f32_lds_lane + (parked ? k - park_from : 0) * 12;
                if constexpr (decltype(packed_body)::value) {
                    process_unit_f32<NT, OP, true>(d, xr, X, (unsigned)dn.x * 12u, window_of(u + 1), st, stress,
                                                   row_rsrc, row_voff, stage_slot, pk24_base(dc));
                } else {
                    process_unit_f32<NT, OP>(d, xr, X, (unsigned)dn.x * 12u, window_of(u + 1), st, stress,
                                             row_rsrc, row_voff, stage_slot);
                }
            } else if constexpr (W) {
                // fp64, 2 x 512 units: lanes 48..53 hold one of the unit's 6 sums each
                // (parking as in fp32; an LDS slot is 4 bytes, a sum takes two)
                const bool mine = lane >= 48 && lane < 54;
                const unsigned row_voff =
                    (mine && !parked) ? (unsigned)k * kRowBytes + (unsigned)(lane - 48) * 8u
                                      : kDropOffset;
                const int stage_slot =
                    stage0 + ((mine && parked) ? (k - park_from) * 12 + (lane - 48) * 2
                                               : cap_units * 12 + 2 * (lane & 1));
                process_unit_f64w<NT, OP>(d, xr, window_of(u + 1), st.xj, st.gc, sel, stress,
                                          row_rsrc, row_voff, stage_slot);
            } else {                        // fp64, 8 x 128: lane 63 stores each row's three sums
                const unsigned row_voff = lane == 63 ? (unsigned)k * kRowBytes : kDropOffset;
                process_unit_f64n<NT, OP>(d, xr, window_of(u + 1), st.xj, st.gc, stress,
                                          row_rsrc, row_voff);
            }
            if constexpr (sizeof(T) != 4) xr = xrn;
            dc = dn;
            dn = dnn;
        };
        // Outer loop: one trip per column strip the wave's sweep crosses (rare).
        // Inner loop: the units of that strip, with NO branch in the body.
        int u = ua;
        if constexpr (PK) {
            // One trip of the outer loop per strip as below, and within it one per run of units
            // of one format: the strip's state stays across a change of format.  Each format has
            // its copy of the unit body, entered with nothing in flight.  A refill goes to window
            // register k from KiB k of the next unit whichever body issues it, so a packed run
            // finds its 6 loads there (what a raw body fetched beyond them is not looked at: the
            // stream ends in 8 KiB of padding), and a raw run asks for the two it is short of.
            // The packed body has no empty-pair mask and runs the packed units with base != 0,
            // which hold no zero (process_unit_f32).  A packed unit with base 0 is all zeros, 6 KiB
            // of zero dwords in the stream: window registers 0..5 hold its distances (+0.0) as they
            // are, 6 and 7 are set, and the RAW body computes what it computes on such a unit
            // without the stream, the signs of its zero sums included.  That run is one unit
            // long: the body's refills 6 and 7 come from beyond the next unit's 6 KiB if that
            // one is packed, so whatever follows enters its run afresh.
            for (;;) {
                const int curj = dc.y;
                strip_load(curj);
                for (;;) {
                    if (pk24_packed_body(dc)) {
                        __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0)
                        do {
                            unit_step(u, std::true_type{});
                            ++u;
                        } while (u < ub && dc.y == curj && pk24_packed_body(dc));
                    } else {
                        const bool zeros = pk24_packed(dc);
                        if (zeros) {
                            d[6] = d[7] = make_float4(0.f, 0.f, 0.f, 0.f);
                        } else {
                            const Win here = window_here();
                            d[6] = here.template load<NT>(6);
                            d[7] = here.template load<NT>(7);
                        }
                        __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0)
                        do {
                            unit_step(u, std::false_type{});
                            ++u;
                        } while (!zeros && u < ub && dc.y == curj && !pk24_packed(dc));
                    }
                    if (u >= ub || dc.y != curj) break;
                }
                if (u >= ub) break;
                strip_store(slot);
                const double sv = wave_sum_hi(stress);
                if (lane == 63) stress_slot[slot] = sv;
                stress = 0.0;
                ++slot;
            }
        } else {
            for (;;) {
                const int curj = dc.y;
                strip_load(curj);
                // ONE copy of the unit body, entered with nothing in flight: hipcc's s_waitcnt
                // counts are static and merged over every entry of a loop header, and a
                // prologue- or strip-change-shaped entry would drain most of the 8-row prefetch
                // window on every iteration.  The strip's coordinates have to be here anyway,
                // and they were asked for after the window, so the wait counts inside the loop
                // are those of the back edge alone.  Same speed as peeling the first unit at
                // every size (profiles/archive/r02_peel_ab.txt), a third less code.
                __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0)
                do {
                    unit_step(u, std::false_type{});
                    ++u;
                } while (u < ub && dc.y == curj);
                if (u >= ub) break;      // the wave's last strip: its column partial goes out below
                strip_store(slot);
                // the stress of the strip left behind goes with its slot (rare: once per strip a
                // wave crosses), so that every stress partial belongs to ONE strip -- and with
                // several maps in one solver (bb_solver_set_maps) to one map
                {
                    const double sv = wave_sum_hi(stress);
                    if (lane == 63) stress_slot[slot] = sv;
                    stress = 0.0;
                }
                ++slot;
            }
        }
        if constexpr (WPB == 8) {
            // done: the partner stops yielding
            __hip_atomic_store(progress + wib, 0x7fffffff, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            __builtin_amdgcn_s_setprio(0);
        }
        if constexpr (DEFER) {
            // the chunk's row sums, 48 bytes per unit in either precision (12 floats or
            // 6 doubles), in one contiguous burst.
            // Lanes read what other lanes of this wave parked: LDS operations of one
            // wave execute in program order; the fence is for the compiler.
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            const int n4 = ((ub - ua) - park_from) * 3;   // float4 count
            float4 *dst = reinterpret_cast<float4 *>(rowpart + ((int64_t)ua + park_from) *
                                                                   (3 * Lay<T, W>::RPU));
            // (the lane number afresh: hipcc otherwise keeps the prologue's 64-bit `lane` alive
            // through the whole sweep for this loop's index, two registers the fp32 unit
            // does not have -- scratch in the 4-wave matvec form)
            const int lane_q = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
            for (int q = lane_q; q < n4; q += 64) {
                const float *src = row_lds + stage0 + 4 * q;
                dst[q] = make_float4(src[0], src[1], src[2], src[3]);
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");   // the region is free again
            __builtin_amdgcn_wave_barrier();
        }
        // the column partial of the wave's LAST strip: into its LDS region (same layout as a
        // slot in HBM), to be added to its neighbours' below
        store_strip(st, reinterpret_cast<T *>(row_lds + stage0), lane);
    }
    // One column partial per WORKGROUP and strip, not per wave: consecutive waves sweep
    // consecutive chunks, almost always of the same strip, so the 4 or 8 partials of a
    // workgroup are added here, in wave order (fixed), and leave as one slot -- an eighth
    // of the bytes for the sweep to write and for the reduce to read back.  wave_slots[].y
    // names the shared slot; waves of one workgroup that end in the same strip carry the
    // same number (the host deals them).
    // The barrier orders LDS only: __syncthreads() is also a release of the wave's global
    // stores, and waiting here for the acknowledgement of the row-sum burst (s_waitcnt vmcnt
    // in front of s_barrier) kept every wave 1-2 us at the end of every launch.
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
    {
        constexpr int CH = 3 * VW, NTH = 64 * WPB;
        int k = 0;
        while (k < WPB) {
            const int sl = ws_shared[k];       // wave-uniform (scalar registers)
            if (sl < 0) { ++k; continue; }
            int k2 = k + 1;
            while (k2 < WPB && ws_shared[k2] == sl) ++k2;
            T *dst = colpart + (int64_t)sl * CH;
#pragma unroll
            for (int j = 0; j < (CH + NTH - 1) / NTH; ++j) {
                const int e = (int)threadIdx.x + NTH * j;
                if (CH % NTH == 0 || e < CH) {
                    T acc = T(0);
                    for (int q = k; q < k2; ++q)
                        acc += reinterpret_cast<const T *>(row_lds + q * lds_wave_floats)[e];
                    dst[e] = acc;
                }
            }
            k = k2;
        }
    }

    // per-wave stress: fixed DPP tree, total in lane 63 (no LDS round trips at the very end
    // of the launch: six __shfl_down steps of a double are twelve ds_bpermute)
    stress = wave_sum_hi(stress);
    if (lane == 63) stresspart[w] = stress;
