// bb_solver_plan.cpp -- the sweep plan and the 24-bit stream's table (bb_solver_plan.h): plain
// integer code that decides every offset the sweep and the reduce kernels read and write.  It
// calls no device function and reads no environment, so all of it runs -- and is tested --
// without a GPU; a wrong slot, list entry or LDS size here would be a fault there.
#include "bb_solver_plan.h"

#include <algorithm>
#include <string>

namespace bb {

namespace {

// Waves per CU (4 waves = one workgroup).  Measured on MI355X: with the rolling
// 8-KiB window one wave per SIMD already keeps enough bytes in flight, and fewer,
// longer chunks mean fewer column-partial slots and less prologue per byte; two
// waves per SIMD overlap one wave's VALU work with the other's waits.  With the
// current kernel (profiles/archive/r01_sweep_wpc.txt): 8/CU is 2-4 % faster from ~150k units
// per rank (N=24,926) up, 4 and 8 tie at 77k units (1/8 of the N=50k matrix, where
// 4 means half as many column partials for the reduce), 6 is always worse (a
// workgroup count that is not a multiple of the CU count), 16 is 2 % slower.
// Round 3, with the one-launch reduce (whose time no longer grows with the number of
// column slots) and by the kernel trace (tools/wpc_timeline.sh, profiles/r03_wpc_ab.txt): 8
// per CU takes 110.3-111.9 us per iteration at N=17,700 against 116.3-116.5 with 4, and ties
// at N=12,000 and 14,500: the switch is at 65k units (N ~ 16,200 on one rank).
// The knob (BB_WAVES_PER_CU) overrides.
int waves_per_cu(const SweepKnobs &knobs, int64_t n_local) {
    const int v = knobs.waves_per_cu != 0 ? knobs.waves_per_cu : (n_local >= 65000 ? 8 : 4);
    return std::max(1, std::min(v, 32));
}

// The 24-bit stream pays only where it takes bytes off the sweep: its kernel carries a second
// copy of the unit body and drains its window at every change of format (an all-zero packed
// unit is a run of its own in the raw body), and a packed unit costs 15 more VALU instructions
// than a raw one (383 against 368: 48 of decode, less the empty-pair mask a unit without a zero
// does without; it was 52 more with the mask).  Below a saving of an eighth of the raw bytes
// (all a sparse raw map with zeros in most units can offer is 0) the solver keeps reading
// d_units with the kernel it always had.
constexpr int64_t kPk24MinSavingDiv = 8;   // stream bytes <= raw bytes * (1 - 1/8)

}  // namespace

int check_tile_list(const char *who, const bb_layout_info &L, const int32_t *tile_I, const int32_t *tile_J,
                    int64_t n_tiles) {
    // blocked-sparse: validate order (J, then I ascending; I <= J < n_blocks)
    for (int64_t t = 0; t < n_tiles; ++t) {
        const bool in_range = tile_I[t] >= 0 && tile_I[t] <= tile_J[t] && tile_J[t] < L.n_blocks;
        const bool ordered = t == 0 || tile_J[t] > tile_J[t - 1] ||
                             (tile_J[t] == tile_J[t - 1] && tile_I[t] > tile_I[t - 1]);
        if (!in_range || !ordered)
            return fail(BB_ERR_INVALID, std::string(who) + ": tile list must be strictly ordered by "
                                                           "(J, I) with 0 <= I <= J < n_blocks");
    }
    return BB_OK;
}

// Build every index the kernels need from (tile list, unit range).
int sweep_plan(const char *who, const bb_layout_info &L, int dtype, bool wide, const int32_t *tile_I,
               const int32_t *tile_J,
               int64_t u_begin, int64_t u_end, int cus, const SweepKnobs &knobs, SweepPlan *plan) {
    SweepPlan &p = *plan;
    p = SweepPlan();
    const int64_t upt = L.units_per_tile, vw = L.vw;
    const int64_t ch = 3 * vw;
    p.n_local = u_end - u_begin;
    if (p.n_local >= ((int64_t)1 << 31))
        return fail(BB_ERR_INVALID, std::string(who) + ": more than 2^31 units on one rank");
    p.t_first = p.n_local > 0 ? u_begin / upt : 0;
    const int64_t t_last = p.n_local > 0 ? (u_end - 1) / upt : -1;
    p.n_local_tiles = p.n_local > 0 ? t_last - p.t_first + 1 : 0;

    p.udesc.resize((size_t)std::max<int64_t>(p.n_local, 1));
    for (int64_t ul = 0; ul < p.n_local; ++ul) {
        const int64_t u = u_begin + ul, t = u / upt, sub = u % upt;
        p.udesc[ul] = make_int2((int)(tile_I[t] * vw + sub * L.rows_per_unit), (int)(tile_J[t] * vw));
    }

    const int wpc = waves_per_cu(knobs, p.n_local);
    int64_t nw = std::max<int64_t>(1, std::min<int64_t>((int64_t)cus * wpc, p.n_local));
    // 8 waves per CU: put the two waves of a SIMD into one workgroup so that they can
    // keep each other's pace (stress_grad_kernel, WPB = 8).  The pair knob (BB_PAIR=0) turns it off.
    p.wpb = (knobs.pair && (dtype == BB_F32 || wide) && wpc >= 8 && nw >= 8) ? 8 : 4;
    nw = round_up(nw, p.wpb);
    p.n_waves = (int)nw;

    // Matrix loads are non-temporal (measured: +2.5 % on the kernel, +9 % on a pure read
    // sweep at N=50k) unless this rank's units fit the 256-MB Infinity Cache: then they
    // are read again from it on the next iteration, and plain loads keep them there
    // (N=8,000 / 10,000: kernel -8 %, step -3.5 / -6 %; equal at N=12,000 = 288 MB;
    // non-temporal 3-4 % better at N=17,700; profiles/archive/r02_nt_ab.txt).
    p.nontemporal = p.n_local * kUnitBytes > ((int64_t)240 << 20);
    // wave w owns the contiguous chunk [w*q + min(w, r), +q (+1 if w < r)), q = n_local / nw,
    // r = n_local % nw: the kernels compute it the same way (no table to load)
    p.chunk_q = (int)(p.n_local / nw);
    p.chunk_r = (int)(p.n_local % nw);
    std::vector<int2> wave_range(nw);
    int64_t chunk_max = 0;
    for (int64_t w = 0; w < nw; ++w) {
        const int64_t a = w * p.chunk_q + std::min<int64_t>(w, p.chunk_r);
        wave_range[w] = make_int2((int)a, (int)(a + p.chunk_q + (w < p.chunk_r ? 1 : 0)));
        chunk_max = std::max<int64_t>(chunk_max, wave_range[w].y - wave_range[w].x);
    }
    {
        // fp32 / fp64 wide: a wave parks the row sums of (the last cap units of) its chunk
        // in LDS until it has finished reading (stress_grad_kernel, DEFER); cap is what the
        // workgroups sharing a CU can hold, 0 only on a rank without units.
        const int64_t wgs_per_cu = std::max<int64_t>(1, (nw / p.wpb + cus - 1) / cus);
        const int64_t budget = 156 * 1024 / wgs_per_cu;               // of the CU's 160 KiB
        const int64_t cap = std::min<int64_t>(chunk_max, (budget / p.wpb - 16 - 8) / 48);
        if ((dtype == BB_F32 || wide) && cap > 0) p.defer_cap_units = (int)cap;
        // a wave's LDS region: the parked row sums while it sweeps, its last column partial
        // (3 * vw elements) at the end; + the 8 progress words of a paired workgroup
        const int64_t col_words = 3 * vw * elem_size(dtype) / 4;
        p.lds_wave_floats = (int)std::max<int64_t>((int64_t)p.defer_cap_units * 12 + 4, col_words);
        p.defer_lds_bytes = (int64_t)p.wpb * p.lds_wave_floats * 4 + 32;
    }
    // Column-partial slots.  A wave's strips but the last get private slots (it writes them
    // itself, mid-sweep: rare); the strip a wave ENDS in shares one slot with the other
    // waves of its workgroup that end in the same strip (summed in LDS by the sweep's
    // epilogue).
    std::vector<int32_t> &slot_strip = p.slot_strip;
    p.wave_last_strip.assign((size_t)nw, -1);
    std::vector<int2> &wave_slots = p.wave_slots;
    wave_slots.resize((size_t)nw);
    for (int64_t w = 0; w < nw; ++w) {
        wave_slots[w] = make_int2((int)slot_strip.size(), -1);
        if (wave_range[w].x >= wave_range[w].y) continue;           // no units
        int cur = -1;
        std::vector<int> strips;
        for (int64_t ul = wave_range[w].x; ul < wave_range[w].y; ++ul) {
            const int J = p.udesc[ul].y / (int)vw;
            if (J != cur) { strips.push_back(J); cur = J; }
        }
        for (size_t q = 0; q + 1 < strips.size(); ++q) slot_strip.push_back(strips[q]);
        const int Jlast = strips.back();
        p.wave_last_strip[(size_t)w] = Jlast;
        const bool same_wg = w % p.wpb != 0;
        if (same_wg && wave_slots[w - 1].y >= 0 &&
            slot_strip[(size_t)wave_slots[w - 1].y] == Jlast) {
            wave_slots[w].y = wave_slots[w - 1].y;
        } else {
            wave_slots[w].y = (int)slot_strip.size();
            slot_strip.push_back(Jlast);
        }
    }
    p.n_slots = (int)slot_strip.size();
    p.rowpart_elems = p.n_local_tiles * ch;
    p.colpart_elems = (int64_t)p.n_slots * ch;

    // reduce CSR: block b <- row chunks of local tiles with I == b, then column slots of strip b
    const int64_t nb = L.n_blocks;
    std::vector<int64_t> blk_ptr(nb + 1, 0);
    for (int64_t lt = 0; lt < p.n_local_tiles; ++lt) blk_ptr[tile_I[p.t_first + lt] + 1]++;
    for (int sl = 0; sl < p.n_slots; ++sl) blk_ptr[slot_strip[sl] + 1]++;
    for (int64_t b = 0; b < nb; ++b) blk_ptr[b + 1] += blk_ptr[b];
    std::vector<int64_t> blk_chunk((size_t)std::max<int64_t>(blk_ptr[nb], 1));
    std::vector<int64_t> fill(blk_ptr.begin(), blk_ptr.end() - 1);
    for (int64_t lt = 0; lt < p.n_local_tiles; ++lt)
        blk_chunk[fill[tile_I[p.t_first + lt]]++] = lt * ch;
    for (int sl = 0; sl < p.n_slots; ++sl)
        blk_chunk[fill[slot_strip[sl]]++] = p.rowpart_elems + (int64_t)sl * ch;

    // Reduce (reduce_sliced_kernel): every block's whole list in one table of fixed stride,
    // padded with the offset of a chunk of zeros that sits behind the column partials; 4
    // slices per workgroup while no list is longer than 64 chunks, else 8
    int64_t longest = 0;
    for (int64_t b = 0; b < nb; ++b) longest = std::max(longest, blk_ptr[b + 1] - blk_ptr[b]);
    p.zero_off = p.rowpart_elems + p.colpart_elems;
    p.part_total = p.zero_off + ch;
    p.red_slices = knobs.reduce_slices != 0 ? (knobs.reduce_slices == 4 ? 4 : 8) : (longest <= 64 ? 4 : 8);
    const int64_t quantum = 16 * p.red_slices;
    p.red_stride = (int)round_up(std::max<int64_t>(longest, 1), quantum);
    p.red_lists.assign((size_t)(nb * p.red_stride), p.zero_off);
    for (int64_t b = 0; b < nb; ++b)
        for (int64_t k = blk_ptr[b]; k < blk_ptr[b + 1]; ++k)
            p.red_lists[(size_t)(b * p.red_stride + (k - blk_ptr[b]))] = blk_chunk[k];

    if (knobs.row_owner) {
        // a whole number of trips per row: 256 columns in fp32, 128 in fp64 (RowTrip<T>::COLS)
        p.full_ld = round_up(L.n_bins, row_trip_cols(dtype));
        // waves per row: enough of them that a small map still covers the chip with
        // about 16 waves per CU (N=963: 4 per row)
        p.ro_wpr = L.n_bins <= 1024 ? 4 : (L.n_bins <= 2048 ? 2 : 1);
        const int rows_per_wg = 4 / p.ro_wpr;
        p.ro_blocks = (int)((L.n_bins + rows_per_wg - 1) / rows_per_wg);
    }
    return BB_OK;
}

void pk24_table(const uint2 *mm, const int2 *udesc, int64_t n, int64_t min_run, int mode, Pk24Table *out) {
    // packable: max - min < 2^24; stored packed: inside a run of >= min_run packable units
    std::vector<int4> &table = out->table;
    table.resize((size_t)n);
    int64_t kib = 0, packed = 0, switches = 0;
    for (int64_t a = 0; a < n;) {
        const bool pk = mm[(size_t)a].y - mm[(size_t)a].x < (1u << 24);
        int64_t b = a + 1;
        while (b < n && (mm[(size_t)b].y - mm[(size_t)b].x < (1u << 24)) == pk) ++b;
        const bool store_packed = pk && b - a >= min_run;
        for (int64_t u = a; u < b; ++u) {
            table[(size_t)u] = make_int4(udesc[(size_t)u].x, udesc[(size_t)u].y,
                                         (int)((uint32_t)kib | (store_packed ? 0x80000000u : 0u)),
                                         store_packed ? (int)mm[(size_t)u].x : 0);
            kib += store_packed ? kPk24PackedKiB : kPk24RawKiB;
        }
        if (store_packed) packed += b - a;
        a = b;
    }
    for (int64_t u = 1; u < n; ++u) switches += (table[(size_t)u].z < 0) != (table[(size_t)u - 1].z < 0);
    const int64_t raw_kib = n * kPk24RawKiB;
    const bool pays = mode == 1 ? packed > 0 : kib * kPk24MinSavingDiv <= raw_kib * (kPk24MinSavingDiv - 1);
    out->kib = kib, out->packed = packed, out->switches = switches;
    // (the table holds a unit's offset in 31 bits of KiB)
    out->pays = n > 0 && mode != 0 && pays && kib < ((int64_t)1 << 31);
}

}  // namespace bb

extern "C" {

int bb_layout_sweep_plan(int64_t n_bins, int dtype, const int32_t *tile_I, const int32_t *tile_J,
                         int64_t n_tiles, int64_t u_begin, int64_t u_end, int cus, const bb_sweep_knobs *knobs,
                         bb_sweep_plan *plan, int32_t *udesc, int32_t *wave_slots, int32_t *slot_strip,
                         int32_t *wave_last_strip, int64_t *red_lists) {
    BB_REQUIRE(plan != nullptr && knobs != nullptr, "bb_layout_sweep_plan: NULL argument");
    BB_REQUIRE((tile_I == nullptr) == (tile_J == nullptr) && (tile_I != nullptr || n_tiles == 0),
               "bb_layout_sweep_plan: tile_I/tile_J/n_tiles inconsistent");
    BB_REQUIRE(cus >= 1 && cus <= 65536, "bb_layout_sweep_plan: cus must be in [1, 65536]");
    bb_layout_info L;
    BB_TRY(bb_layout_dense_info(n_bins, dtype, &L));
    std::vector<int32_t> dense_I, dense_J;
    if (tile_I == nullptr) {
        dense_I.resize((size_t)L.n_tiles), dense_J.resize((size_t)L.n_tiles);
        BB_TRY(bb_layout_dense_tiles(n_bins, dtype, dense_I.data(), dense_J.data(), L.n_tiles));
        tile_I = dense_I.data(), tile_J = dense_J.data();
    } else {
        BB_REQUIRE(n_tiles >= 0, "bb_layout_sweep_plan: n_tiles < 0");
        BB_TRY(bb::check_tile_list("bb_layout_sweep_plan", L, tile_I, tile_J, n_tiles));
        L.n_tiles = n_tiles;
        L.n_units = n_tiles * L.units_per_tile;
    }
    BB_REQUIRE(0 <= u_begin && u_begin <= u_end && u_end <= L.n_units,
               "bb_layout_sweep_plan: need 0 <= u_begin <= u_end <= n_units");
    bb::SweepKnobs k;
    k.waves_per_cu = knobs->waves_per_cu, k.pair = knobs->pair != 0;
    k.reduce_slices = knobs->reduce_slices, k.row_owner = knobs->row_owner != 0;
    bb::SweepPlan p;
    BB_TRY(bb::sweep_plan("bb_layout_sweep_plan", L, dtype, bb::wide_layout(dtype, n_bins), tile_I, tile_J, u_begin, u_end, cus, k, &p));
    *plan = bb_sweep_plan{p.n_local, p.t_first, p.n_local_tiles, p.n_waves, p.wpb, p.chunk_q, p.chunk_r,
                          p.n_slots, p.rowpart_elems, p.colpart_elems, p.zero_off, p.part_total,
                          p.red_slices, p.red_stride, L.n_blocks, p.defer_cap_units, p.lds_wave_floats,
                          p.defer_lds_bytes, p.nontemporal ? 1 : 0, p.full_ld, p.ro_wpr, p.ro_blocks};
    static_assert(sizeof(int2) == 2 * sizeof(int32_t), "udesc and wave_slots leave as pairs of int32");
    if (udesc) std::copy_n((const int32_t *)p.udesc.data(), 2 * p.n_local, udesc);
    if (wave_slots) std::copy_n((const int32_t *)p.wave_slots.data(), 2 * (int64_t)p.n_waves, wave_slots);
    if (slot_strip) std::copy(p.slot_strip.begin(), p.slot_strip.end(), slot_strip);
    if (wave_last_strip) std::copy(p.wave_last_strip.begin(), p.wave_last_strip.end(), wave_last_strip);
    if (red_lists) std::copy(p.red_lists.begin(), p.red_lists.end(), red_lists);
    return BB_OK;
}

int bb_layout_pk24_table(const uint32_t *min_max, const int32_t *udesc, int64_t n, int64_t min_run, int mode,
                         int32_t *table, int64_t *stream_kib, int64_t *packed_units,
                         int64_t *format_switches, int *pays) {
    BB_REQUIRE(n >= 0 && (n == 0 || (min_max != nullptr && udesc != nullptr)),
               "bb_layout_pk24_table: NULL argument");
    BB_REQUIRE(min_run >= 1, "bb_layout_pk24_table: min_run must be >= 1");
    static_assert(sizeof(uint2) == 8 && sizeof(int2) == 8 && sizeof(int4) == 16, "the arrays are plain words");
    bb::Pk24Table t;
    bb::pk24_table((const uint2 *)min_max, (const int2 *)udesc, n, min_run, mode, &t);
    if (table) std::copy_n((const int32_t *)t.table.data(), 4 * n, table);
    if (stream_kib) *stream_kib = t.kib;
    if (packed_units) *packed_units = t.packed;
    if (format_switches) *format_switches = t.switches;
    if (pays) *pays = t.pays ? 1 : 0;
    return BB_OK;
}

}  // extern "C"
