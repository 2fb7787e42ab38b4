#!/bin/bash
# PMC passes of ONE conv launch: tools/pmc_conv.sh <tag> <arguments of `conv_probe.py loop`>   (on a machine with the GPU, from the repository root), e.g.
#   tools/pmc_conv.sh w6s --row OSA2_x -v 6/64/1        tools/pmc_conv.sh pw --shape 8,50,80,1472,768,1,1 -v 8/32/4
# Every counter set runs in a pass of its own, with --kernel-trace and nothing else.  PMC_SETS="A B;C D" replaces the default passes.
# Prints the mean of each counter over the dispatches of the conv kernels; raw output under $PMC_OUT/pmc_<tag>/ (default: build/, which git ignores).
TAG=$1; shift
ROOT=$(cd "$(dirname "$0")/.." && pwd); OUT=${PMC_OUT:-$ROOT/build}/pmc_$TAG; mkdir -p $OUT; export TMPDIR=/tmp; cd /tmp
DEFAULT="SQ_WAVE_CYCLES SQ_BUSY_CU_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_VALU_MFMA_BUSY_CYCLES GRBM_GUI_ACTIVE;\
SQ_INSTS_VALU SQ_INSTS_MFMA SQ_INSTS_LDS SQ_INSTS_VMEM_RD SQ_INSTS_SALU SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_LDS SQ_WAIT_INST_LDS;\
SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_INST_CYCLES_VMEM SQ_ACTIVE_INST_MISC SQ_ACTIVE_INST_SCA SQ_INSTS_VALU_MFMA_MOPS_F32 SQ_VALU_MFMA_COEXEC_CYCLES;\
TCP_TCC_READ_REQ_sum TCP_TOTAL_CACHE_ACCESSES_sum TCC_HIT_sum TCC_MISS_sum TCC_EA0_RDREQ_sum TCC_REQ_sum"
IFS=';' read -ra SETS <<< "${PMC_SETS:-$DEFAULT}"
i=0
for SET in "${SETS[@]}"; do
  i=$((i+1))
  rocprofv3 --kernel-trace --output-format csv --pmc $SET -d $OUT/p$i -o c -- python3 $ROOT/tools/conv_probe.py loop --iters 3 "$@" > $OUT/p$i.out 2> $OUT/p$i.err \
    || { tail -2 $OUT/p$i.out $OUT/p$i.err; echo "pass $i failed: no further pass is run"; exit 1; }
done
python3 - <<PY
import csv, glob, collections
acc = collections.defaultdict(list)
for f in glob.glob("$OUT/p*/c_counter_collection.csv"):
    for r in csv.DictReader(open(f)):
        if "cmk::conv_" in r["Kernel_Name"]:
            acc[r["Counter_Name"]].append(float(r["Counter_Value"]))
for k in sorted(acc): print("%-32s %.4g  (n=%d)" % (k, sum(acc[k]) / len(acc[k]), len(acc[k])))
PY
rm -rf $OUT/p*/c_kernel_trace.csv
