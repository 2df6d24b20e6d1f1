#!/bin/bash
# Build libblueberry_hip.so (gfx950), the tests' probe of its fp64 routines and the CPU oracle.  Used by
# __graft_entry__.build(); safe to run by hand.  hipcc cross-compiles without a GPU.
# THE list of the library's sources is here.  BB_EXTRA_FLAGS: more compiler flags; BB_OUT:
# where the library goes (tools/build_variant.sh sets both for its A/B builds).
set -euo pipefail
cd "$(dirname "$0")"
OUT="${BB_OUT:-blueberry_amd/libblueberry_hip.so}"
# -fno-slp-vectorize: the SLP vectorizer fuses the pair math of all 8 rows of a
# unit into long v_pk_* trees and spills ~500 B/lane in stress_grad_kernel;
# without it the kernel needs 104 VGPRs and no scratch.
SRC=""
for f in bb_api.cpp bb_comm.cpp bb_solver_plan.cpp bb_solver.hip bb_solver_inputs.hip \
         bb_solver_exchange.hip bb_solver_queries.hip bb_solver_anchors.hip \
         bb_solver_spectral.hip bb_group.hip bb_score.hip bb_compare.hip bb_band.hip \
         bb_contactmap.hip bb_shortest.hip bb_balance.hip bb_triples_balance.hip bb_triples_paths.hip \
         bb_significance.hip bb_coarsen.hip bb_insulation.hip bb_sort.hip bb_misc.hip; do
    SRC="$SRC blueberry_amd/csrc/$f"
done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared -fvisibility=hidden \
    -Wno-unused-value -Wno-unused-result -fno-slp-vectorize \
    -Iinclude -Iblueberry_amd/csrc ${BB_EXTRA_FLAGS:-} \
    -o "$OUT" $SRC -ldl
# test-only: the refined fp64 routines of the pair arithmetic behind one entry point
# (tests/test_gpu_pair_math.py).  BB_PROBE_OUT: where it goes; a variant build (BB_OUT alone)
# leaves the tree's probe alone.
if [ -n "${BB_PROBE_OUT:-}" ] || [ -z "${BB_OUT:-}" ]; then
    /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared -fvisibility=hidden \
        -Wno-unused-value -Wno-unused-result -Wno-unused-function -fno-slp-vectorize \
        -Iinclude -Iblueberry_amd/csrc ${BB_EXTRA_FLAGS:-} \
        -o "${BB_PROBE_OUT:-tests/probes/librefined_f64_probe.so}" tests/probes/refined_f64_probe.hip
fi
make -s -C oracle
echo "built $OUT and oracle/libbb_oracle.so"
