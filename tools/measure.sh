#!/bin/bash
# A tree's measurement pass: smoke, the default bench line, the single-branch and Grad-CAM
# configs, the per-shape GEMM table, then the kernel trace and the PMC traffic of the default
# (parity) step (tools/profile.sh).  Summaries: tools/prof_summary.py, tools/pmc_by_kernel.py.
#   bash tools/measure.sh <tag>
set -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd); OUT=${TOOLS_OUT:-$R/tools_out}
TAG=${1:?usage: bash tools/measure.sh <tag>}; mkdir -p $OUT; cd $R
timeout -k 10 300 python -u -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke_$TAG.log 2>&1 || { echo "smoke rc=$?"; tail -20 $OUT/smoke_$TAG.log; exit 1; }
tail -2 $OUT/smoke_$TAG.log
timeout -k 10 900 python bench.py --full > $OUT/bench_$TAG.json 2> $OUT/bench_$TAG.err || { echo "bench rc=$?"; tail -20 $OUT/bench_$TAG.err; exit 1; }
cat $OUT/bench_$TAG.json
for c in rgb thermal; do
  timeout -k 10 400 python bench.py --full --config $c --no-cpu-baseline > $OUT/bench_${TAG}_$c.json 2> $OUT/bench_${TAG}_$c.err || { echo "bench $c rc=$?"; tail -20 $OUT/bench_${TAG}_$c.err; exit 1; }
done
timeout -k 10 600 python bench.py --full --config gradcam > $OUT/bench_${TAG}_gradcam.json 2> $OUT/bench_${TAG}_gradcam.err || { echo "bench gradcam rc=$?"; tail -20 $OUT/bench_${TAG}_gradcam.err; exit 1; }
timeout -k 10 300 python tools/gemm_step_profile.py > $OUT/gemm_step_$TAG.log 2>&1 || { echo "shapes rc=$?"; exit 1; }
bash tools/profile.sh trace $TAG > /dev/null || exit 1
bash tools/profile.sh traffic $TAG || exit 1
echo measure-done
