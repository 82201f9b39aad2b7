#!/bin/bash
# Where gm_gemm_kernel's waves spend their time: three rocprofv3 --pmc passes of their own (no tracing beside them; the SQ block
# has eight slots per pass) over tools/gemm_pmc.py's probe launches, merged into one table.
# usage: tools/gemm_pmc.sh <tag> [outdir=.]  -> <outdir>/<tag>_counters.txt      (AMC3D_LIB names another build of the library)
set -e
TAG=$1
OUT=${2:-.}
TMP=${TMPDIR:-/tmp}
mkdir -p "$OUT"
A="SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_WAIT_INST_LDS SQ_ACTIVE_INST_ANY SQ_VALU_MFMA_BUSY_CYCLES SQ_WAVES GRBM_GUI_ACTIVE"
B="SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_ACTIVE_INST_LDS SQ_ACTIVE_INST_VMEM SQ_INSTS_LDS SQ_INSTS_VMEM SQ_INSTS_VALU_MFMA_MOPS_F32 SQ_ACTIVE_INST_VALU"
C="SQ_INST_LEVEL_VMEM SQ_INST_LEVEL_LDS"
i=0
for CS in "$A" "$B" "$C"; do
  i=$((i+1))
  rm -rf "$TMP/gemm_pmc_${TAG}_$i"
  timeout -k 10 300 rocprofv3 --pmc $CS --output-format csv -d "$TMP/gemm_pmc_${TAG}_$i" -o r -- python3 tools/gemm_pmc.py run > "$OUT/${TAG}_pmc_$i.log" 2>&1
done
python3 tools/gemm_pmc.py table "$OUT/${TAG}_counters.txt" "$TMP/gemm_pmc_${TAG}_1" "$TMP/gemm_pmc_${TAG}_2" "$TMP/gemm_pmc_${TAG}_3"
cat "$OUT/${TAG}_counters.txt"
