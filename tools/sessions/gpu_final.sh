#!/bin/bash
# round-end style run: full GPU test suite, smoke, bench, rocprofv3 kernel trace + PMC passes (both execution modes)
cd $GRAFT_REPO_ROOT
OUT=${OUT:-bench_out}; mkdir -p "$OUT"    # where the results go
export TMPDIR=/tmp
TAG=${1:-r01}
timeout 1500 python -m pytest tests -m gpu -q > $OUT/${TAG}_pytest.log 2>&1
echo "pytest exit $?" >> $OUT/${TAG}_pytest.log
timeout 300 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/${TAG}_smoke.log 2>&1
echo "smoke exit $?" >> $OUT/${TAG}_smoke.log
timeout 600 python bench.py --full > $OUT/${TAG}_bench.log 2>&1
echo "bench exit $?" >> $OUT/${TAG}_bench.log
timeout 600 python bench.py --full --dedup off --no-cpu-baseline > $OUT/${TAG}_bench_dense.log 2>&1
VV_PREC=bf16 timeout 600 python bench.py --full --no-cpu-baseline > $OUT/${TAG}_bench_bf16.log 2>&1
rm -rf $OUT/prof_${TAG} && mkdir -p $OUT/prof_${TAG}
for mode in on off; do
  P=$OUT/prof_${TAG}/dedup_${mode}
  timeout 600 rocprofv3 --kernel-trace --stats --output-format csv -d $P/trace -o kt -- python3 bench.py --full --steps 20 --warmup 5 --no-cpu-baseline --no-dense-leg --dedup $mode > $OUT/${TAG}_prof_trace_${mode}.log 2>&1
  timeout 600 rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d $P/pmc_fetch -o pf -- python3 bench.py --full --steps 6 --warmup 2 --no-cpu-baseline --no-dense-leg --dedup $mode > $OUT/${TAG}_prof_fetch_${mode}.log 2>&1
  timeout 600 rocprofv3 --pmc WRITE_SIZE --kernel-trace --output-format csv -d $P/pmc_write -o pw -- python3 bench.py --full --steps 6 --warmup 2 --no-cpu-baseline --no-dense-leg --dedup $mode > $OUT/${TAG}_prof_write_${mode}.log 2>&1
  python3 tools/summarize_prof.py $P > $OUT/${TAG}_prof_summary_dedup_${mode}.txt 2>&1
done
python3 tools/make_pmc_json.py $OUT/prof_${TAG} > $OUT/${TAG}_pmc.json 2> $OUT/${TAG}_pmc.err
for mode in on off; do cp $(find $OUT/prof_${TAG}/dedup_${mode}/trace -name "*kernel_stats.csv" | head -1) $OUT/${TAG}_kernel_stats_dedup_${mode}.csv; done
find $OUT/prof_${TAG} -name "*kernel_trace.csv" -size +2M -delete
find $OUT/prof_${TAG} -name "*counter_collection.csv" -size +2M -delete
tail -3 $OUT/${TAG}_pytest.log; tail -2 $OUT/${TAG}_smoke.log; grep '^{' $OUT/${TAG}_bench.log | cut -c1-300; grep '^{' $OUT/${TAG}_bench_dense.log | cut -c1-200; grep '^{' $OUT/${TAG}_bench_bf16.log | cut -c1-200
grep -E "k_fwd|k_wgrad|k_score|k_reduce|k_sgd|k_seg|k_dd" $OUT/${TAG}_prof_summary_dedup_on.txt | head -30
