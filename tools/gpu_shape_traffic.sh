#!/bin/bash
# Per-shape GEMM table with PMC HBM bytes (tools/gemm_shape_traffic.py): the recorded step's
# distinct GEMMs replayed between markers under the two passes of tools/profile.sh traffic, times
# from an unprofiled run.  bash tools/gpu_shape_traffic.sh <tag>
set -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd); OUT=${TOOLS_OUT:-$R/tools_out}
TAG=${1:?usage: bash tools/gpu_shape_traffic.sh <tag>}; mkdir -p $OUT; cd $R
timeout -k 10 300 python tools/gemm_step_profile.py --iters 5 > $OUT/shape_times_$TAG.txt 2>&1 || { echo "times rc=$?"; tail -5 $OUT/shape_times_$TAG.txt; exit 1; }
bash tools/profile.sh traffic sp_$TAG -- python3 tools/gemm_step_profile.py --iters 5 --markers $OUT/shapes_$TAG.json > /dev/null || exit 1
python3 tools/gemm_shape_traffic.py $OUT/shapes_$TAG.json $OUT/sp_${TAG}_FETCH_SIZE/pmc_counter_collection.csv $OUT/sp_${TAG}_WRITE_SIZE/pmc_counter_collection.csv $OUT/shape_times_$TAG.txt > $OUT/shape_traffic_$TAG.md
head -50 $OUT/shape_traffic_$TAG.md
