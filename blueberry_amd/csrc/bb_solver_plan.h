// bb_solver_plan.h -- the sweep plan of the 3D-structure solver as pure host arithmetic: from
// (layout, tile list, unit range, CU count, knobs) every index, slot, list and LDS size the
// sweep and the reduce kernels read and write (docs/SPEC.md 3.3-3.5), and the run rule and
// table of the 24-bit stream (SPEC 3.7).  No device, no environment: bb_solver.hip reads the
// knobs (solver_env) and does the allocating and uploading; the C ABI shows both as
// bb_layout_sweep_plan / bb_layout_pk24_table, which tests/test_sweep_plan_cpu.py holds against
// an independent statement.
#pragma once

#include <stdint.h>

#include <vector>

#include "bb_common.h"

namespace bb {

struct SweepKnobs {
    int waves_per_cu = 0;    // BB_WAVES_PER_CU, 1..32; 0: the 65,000-unit rule
    bool pair = true;        // BB_PAIR: workgroups of 8 waves at 8 waves per CU
    int reduce_slices = 0;   // BB_REDUCE_SLICES, 4 or 8; 0: by the longest reduce list
    bool row_owner = false;  // the solver is built with the row-owner buffers
};

struct SweepPlan {
    int64_t n_local = 0;
    int64_t t_first = 0, n_local_tiles = 0;
    std::vector<int2> udesc;               // per local unit {first row, first column}; never empty
    int n_waves = 0, wpb = 4;              // waves, and waves per workgroup (4, or 8: paired)
    int chunk_q = 0, chunk_r = 0;          // units per wave: n_local = n_waves * q + r
    bool nontemporal = true;
    int defer_cap_units = 0;               // units of row sums a wave can park in LDS
    int lds_wave_floats = 0;               // LDS region per wave, in 4-byte words
    int64_t defer_lds_bytes = 0;           // dynamic LDS per workgroup
    std::vector<int2> wave_slots;          // per wave {first private slot, the shared slot or -1}
    std::vector<int32_t> slot_strip;       // strip (block column) of every column slot
    std::vector<int32_t> wave_last_strip;  // strip each wave ends in, -1: no units
    int n_slots = 0;
    int64_t rowpart_elems = 0, colpart_elems = 0;
    int64_t zero_off = 0, part_total = 0;  // the chunk of zeros behind the partials; their size
    int red_slices = 0, red_stride = 0;    // reduce: slices per workgroup; entries per block
    std::vector<int64_t> red_lists;        // n_blocks * red_stride offsets into the partials
    int64_t full_ld = 0;                   // row-owner path (knobs.row_owner), else 0
    int ro_wpr = 1, ro_blocks = 0;
};

// Columns a wave covers per trip of the row-owner kernel: full_ld is a multiple of it.
constexpr int64_t row_trip_cols(int dtype) { return 64 * (16 / (dtype == BB_F64 ? 8 : 4)); }

// BB_OK, or BB_ERR_INVALID: the list is not strictly ordered by (J, I) with 0 <= I <= J < n_blocks.
int check_tile_list(const char *who, const bb_layout_info &L, const int32_t *tile_I, const int32_t *tile_J,
                    int64_t n_tiles);

// The plan of the units [u_begin, u_end) of the tile list (L.n_tiles tiles) on `cus` CUs.
int sweep_plan(const char *who, const bb_layout_info &L, int dtype, bool wide, const int32_t *tile_I,
               const int32_t *tile_J,
               int64_t u_begin, int64_t u_end, int cus, const SweepKnobs &knobs, SweepPlan *plan);

struct Pk24Table {
    std::vector<int4> table;   // per unit {row, column, offset in KiB | packed << 31, base}
    int64_t kib = 0, packed = 0, switches = 0;
    bool pays = false;         // the stream is worth building (and addressable: < 2^31 KiB)
};

// The 24-bit stream of n units from their (smallest, largest) words: which are stored packed,
// where each begins, and whether the stream pays.  mode: 0 never, 1 whenever a unit packs, else
// the saving rule.
void pk24_table(const uint2 *min_max, const int2 *udesc, int64_t n, int64_t min_run, int mode, Pk24Table *out);

// 24-bit stream: a packable unit is stored packed only inside a run of at least this many
// (docs/MEASUREMENTS.md, "fp32 sweep: the 24-bit stream")
constexpr int64_t kPk24MinRun = 64;
constexpr int64_t kPk24PackedKiB = 6, kPk24RawKiB = kUnitBytes / 1024;

}  // namespace bb
