#!/bin/bash
# hipBLASLt vs dfu on the ViT shapes: per case the unprofiled times,
# hipBLASLt's kernel names (kernel trace), and the two counter passes of tools/profile.sh for
# both libraries.  tools/blas_counters_summary.py reads the directories.
#   [CTR=blasctr] [CASES="fc2_fwd ..."] bash tools/blas_counters.sh
set -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd); CTR=${CTR:-blasctr}; OUT=${TOOLS_OUT:-$R/tools_out}/$CTR
mkdir -p $OUT; cd $R
export PMC_A="SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CYCLES GRBM_GUI_ACTIVE GRBM_COUNT"
export PMC_B="SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_INSTS_LDS SQ_INSTS_VALU SQ_INSTS_SALU SQ_WAIT_INST_LDS SQ_ACTIVE_INST_VALU SQ_INSTS_MFMA"
: > $OUT/times.txt
for c in ${CASES:-fc2_fwd fc1_fwd qkv_fwd fc1_dgrad_t qkv_dgrad_t}; do
  timeout -k 10 120 python3 tools/blas_one.py $c --iters 30 >> $OUT/times.txt 2>&1 || { echo "blas time $c rc=$?"; exit 1; }
  timeout -k 10 120 python3 tools/gemm_one.py $c --iters 30 >> $OUT/times.txt 2>&1 || { echo "dfu time $c rc=$?"; exit 1; }
  timeout -k 10 120 rocprofv3 --kernel-trace --output-format csv -d $OUT/${c}_blas_kt -o k -- python3 tools/blas_one.py $c --iters 5 > /dev/null 2>&1 || { echo "kt $c rc=$?"; exit 1; }
  for lib in blas gemm; do
    bash tools/profile.sh counters $CTR/${c}_${lib} -- python3 tools/${lib}_one.py $c --iters 5 || exit 1
  done
  echo "$c done"
done
cat $OUT/times.txt
