R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${OUT:-$R/out}  # where the runs below write
mkdir -p "$OUT"
cd /tmp && export TMPDIR=/tmp
export PMH_BENCH_NO_TIMING=1
name=c2; rx="k_spmv_stream|k_spmv_ell|k_step_update|k_dir_update"
mkdir -p $OUT/pmc_$name
for C in FETCH_SIZE WRITE_SIZE; do
  rocprofv3 --pmc $C --kernel-include-regex "$rx" --output-format csv -d $OUT/pmc_$name/pmc_$C -- python3 $R/bench.py --full --workload c2 --no-cpu-baseline --steps 50 --warmup 5 > $OUT/pmc_${name}_$C.log 2>&1
  tail -n 1 $OUT/pmc_${name}_$C.log | cut -c1-160
done
python3 $R/scripts/pmc_parse.py $OUT/pmc_$name "$PMH_GIT" "rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE (separate passes, FETCH_SIZE x2) --kernel-include-regex '$rx' -- python3 bench.py --full --workload c2 --no-cpu-baseline --steps 50 --warmup 5" && cp $OUT/pmc_$name/pmc_traffic.json $OUT/r02_pmc_traffic_$name.json
rm -rf $OUT/pmc_$name/pmc_FETCH_SIZE $OUT/pmc_$name/pmc_WRITE_SIZE
