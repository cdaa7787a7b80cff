#!/bin/bash
# Same-box A/B: two or more sides run alternately, N rounds, one process per run.
#   bash tools/ab.sh <tag> <rounds> [--tests "<pytest files>"] <side> <side> ...
# A side is one (quoted) argument: [dir=<tree>] [VAR=value ...] [-- <command>]
#   dir      the tree to run in (default: this one; e.g. ab_old, a git-ignored copy of an earlier
#            tree with its own built library)
#   VAR=...  environment of that side ("X=0" for a side that changes nothing)
#   command  default: the short bench line below; its "<label> <number> ms" figures, or the bench
#            JSON's value / ms_per_step / gpu_step_ms.median, are what is compared
#   e.g. bash tools/ab.sh beside 3 "X=0" "DFU_RESNET_WGRAD_BESIDE=1"
#        bash tools/ab.sh lib 3 --tests "tests/test_kernels_gpu.py" "X=0" "DFU_HIP_LIB=$PWD/x.so"
#        bash tools/ab.sh host 3 "dir=ab_old -- python -u tools/host_step_time.py --steps 60 --pin" \
#                                "-- python -u tools/host_step_time.py --steps 60 --pin"
# Outputs go to $TOOLS_OUT (default: tools_out/ in this tree).
# Prints one line per run, then per side the median and the spread (max - min) of each figure.
# --tests: those GPU tests first, in the last side's tree and environment (the candidate).
set -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd); OUT=${TOOLS_OUT:-$R/tools_out}
[ $# -ge 4 ] || { sed -n '2,4p' "$0"; exit 2; }
TAG=$1; N=$2; shift 2; mkdir -p $OUT
TESTS=; if [ "$1" = --tests ]; then TESTS=$2; shift 2; fi
BENCH="bench.py --no-alt-precision --no-parity --no-cpu-baseline --steps 30 --warmup 5 $BENCH_EXTRA"

run_side() {  # <side> <time limit s> <output stem> [command in place of the side's]: one run
  local d=$R envs=() cmd=() w incmd=0 limit=$2 stem=$3
  for w in $1; do
    if [ $incmd = 1 ]; then cmd+=("$w")
    elif [ "$w" = -- ]; then incmd=1
    elif [[ $w == dir=* ]]; then d=${w#dir=}
    else envs+=("$w"); fi
  done
  [ $# -gt 3 ] && cmd=("${@:4}")
  [ ${#cmd[@]} -gt 0 ] || cmd=(python $BENCH)
  (cd $R && cd "$d" && env "${envs[@]}" timeout -k 10 $limit "${cmd[@]}" > $stem.out 2> $stem.err)
}

FIGS='
import json, re, statistics, sys
def figs(path):
    text = open(path).read()
    try:
        d = json.loads(text)
        return [("value", d["value"]), ("ms_per_step", d["ms_per_step"]),
                ("gpu_step_ms.median", d["gpu_step_ms"]["median"])]
    except ValueError:
        return [(m.group(1), float(m.group(2)))
                for m in re.finditer(r"(?:^|, )([A-Za-z][^,\n]*?) (\d+\.\d+) ms", text, re.M)]
label, runs = sys.argv[1], [figs(p) for p in sys.argv[2:]]
if len(runs) == 1:
    print(label, *[v for _, v in runs[0]])
else:
    col = lambda j: [r[j][1] for r in runs]
    print(label, "; ".join("%s median %.4g spread %.3g" % (
        name, statistics.median(col(j)), max(col(j)) - min(col(j)))
        for j, (name, _) in enumerate(runs[0])))
'

if [ -n "$TESTS" ]; then
  run_side "${!#}" 600 $OUT/ab_${TAG}_tests python -u -m pytest -x -q --timeout 300 --timeout-method thread $TESTS \
    || { echo "tests rc=$?"; tail -30 $OUT/ab_${TAG}_tests.out; exit 1; }
  tail -1 $OUT/ab_${TAG}_tests.out
fi
for i in $(seq 1 $N); do
  k=0
  for side in "$@"; do
    k=$((k + 1)); stem=$OUT/ab_${TAG}_${k}_$i
    run_side "$side" 300 $stem || { echo "[$side] rc=$?"; tail -5 $stem.err; exit 1; }
    python -c "$FIGS" "[$side] $i" $stem.out || exit 1
  done
done
k=0
for side in "$@"; do  # per side: median and spread (max - min) of each figure over the rounds
  k=$((k + 1))
  python -c "$FIGS" "[$side]" $(for i in $(seq 1 $N); do echo $OUT/ab_${TAG}_${k}_$i.out; done) || exit 1
done
