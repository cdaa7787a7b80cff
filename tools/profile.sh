#!/bin/bash
# One rocprofv3 measurement of a program, into $TOOLS_OUT (default: tools_out/ in this tree).  Counters and traces never share a run.
#   bash tools/profile.sh <mode> <tag> [VAR=value ...] [-- <program>]
# mode:
#   trace     kernel trace with stats -> prof_<tag>/ (bench_kernel_trace.csv, bench_kernel_stats.csv)
#             and the program's output in prof_<tag>_bench.json, for tools/trace_*.py,
#             kernel_breakdown.py and prof_summary.py.  Default program: ten bench steps.
#   traffic   HBM bytes: FETCH_SIZE, then WRITE_SIZE, each a run of its own -> <tag>_FETCH_SIZE/,
#             <tag>_WRITE_SIZE/, joined per kernel by tools/pmc_by_kernel.py -> pmc_by_kernel_<tag>.txt
#   counters  the two SQ passes (PMC_A, PMC_B below) -> <tag>_a/, <tag>_b/ (<tag>a/, <tag>b/ for a
#             tag that ends in "/"), the layout tools/gemm_counters_summary.py reads
# Default program of traffic and counters: one bench step.  A single GEMM's counter passes:
#   bash tools/profile.sh counters ctr/fc1_fwd_t8 -- python3 tools/gemm_one.py fc1_fwd --tile 8 --iters 5
# The program runs from the repository root, with every VAR=value in its environment.
set -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd); OUT=${TOOLS_OUT:-$R/tools_out}
[ $# -ge 2 ] || { sed -n '2,3p' "$0"; exit 2; }
MODE=$1; TAG=$2; shift 2; mkdir -p "$(dirname "$OUT/${TAG}x")"; cd $R
while [ $# -gt 0 ] && [ "$1" != -- ]; do export "$1"; shift; done
[ "$1" = -- ] && shift
STEP="python3 bench.py --full --no-cpu-baseline --no-alt-precision --no-parity"
PMC_A=${PMC_A:-SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_WAIT_INST_LDS SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CYCLES GRBM_GUI_ACTIVE}
PMC_B=${PMC_B:-SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_INSTS_LDS SQ_INSTS_VALU SQ_INSTS_SALU SQ_ACTIVE_INST_LDS SQ_ACTIVE_INST_VALU SQ_INSTS_MFMA}

pmc() {  # <counters> <output directory> <program...>: one counter-collection run
  local ctr=$1 dir=$2; shift 2
  timeout -k 10 400 rocprofv3 --pmc $ctr --output-format csv -d $dir -o pmc -- "$@" > $dir.log 2>&1 \
    || { echo "pmc [$ctr] rc=$?"; tail -5 $dir.log; exit 1; }
}

case $MODE in
trace)
  [ $# -gt 0 ] || set -- $STEP --steps 10 --warmup 3
  timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_$TAG -o bench -- "$@" \
    > $OUT/prof_${TAG}_bench.json 2> $OUT/prof_${TAG}_bench.err \
    || { echo "rocprof trace rc=$?"; tail -5 $OUT/prof_${TAG}_bench.err; exit 1; }
  cat $OUT/prof_${TAG}_bench.json
  find $OUT/prof_$TAG -name "*.csv" | head ;;
traffic)
  [ $# -gt 0 ] || set -- $STEP --steps 1 --warmup 1 --no-graph
  pmc FETCH_SIZE $OUT/${TAG}_FETCH_SIZE "$@" && pmc WRITE_SIZE $OUT/${TAG}_WRITE_SIZE "$@" || exit 1
  python3 tools/pmc_by_kernel.py $OUT/${TAG}_FETCH_SIZE/pmc_counter_collection.csv \
    $OUT/${TAG}_WRITE_SIZE/pmc_counter_collection.csv > $OUT/pmc_by_kernel_$TAG.txt || exit 1
  head -45 $OUT/pmc_by_kernel_$TAG.txt ;;
counters)
  [ $# -gt 0 ] || set -- $STEP --steps 1 --warmup 1 --no-graph
  P=$OUT/$TAG; [[ $TAG == */ ]] || P=${P}_
  pmc "$PMC_A" ${P}a "$@" && pmc "$PMC_B" ${P}b "$@" || exit 1
  echo "counters -> ${P}a ${P}b" ;;
*) echo "unknown mode $MODE (trace | traffic | counters)"; exit 2 ;;
esac
