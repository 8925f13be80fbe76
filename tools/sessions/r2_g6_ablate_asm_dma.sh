#!/bin/bash
# ablation of the phase-staggered kernels after the LDS-DMA went to inline assembly (dense sizes, f16)
cd $GRAFT_REPO_ROOT
OUT=${OUT:-bench_out}; mkdir -p "$OUT"    # where the results go
export TMPDIR=/tmp
for ab in 0 1 2 4 8 3 6 7; do
  VV_GEMM_VARIANT=5 VV_ABLATE=$ab timeout 300 python bench.py --full --steps 40 --warmup 5 --no-cpu-baseline --no-extra-legs > $OUT/abl.log 2>&1
  echo "ablate $ab: $(python3 -c "
import json
l=[x for x in open('$OUT/abl.log') if x.startswith('{')]
d=json.loads(l[-1]); print('fwd', d['kernels_ms']['fwd_gemm'], 'wgrad', d['kernels_ms']['wgrad_gemm'])")"
done 2>&1 | tee $OUT/r2_ablate_asm_dma.txt
