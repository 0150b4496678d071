# one GPU round: parity tests, smoke, the default bench line, rocprof kernel stats of both workloads
set -x
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${OUT:-$R/out}  # where the runs below write
mkdir -p "$OUT"
python -m pytest tests -x -q -m gpu 2>&1 | grep -E "passed|failed|error" | tail -3
python -c "import __graft_entry__ as g; g.smoke()" 2>&1 | grep smoke | tail -2
mkdir -p $OUT
python bench.py --full > $OUT/bench_default.json 2> $OUT/bench_default.err; tail -2 $OUT/bench_default.err; cut -c1-600 $OUT/bench_default.json
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_c2 -- python3 $R/bench.py --full --workload c2 --steps 100 --warmup 10 --no-cpu-baseline > $OUT/prof_c2.log 2>&1
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_feti -- python3 $R/bench.py --full --steps 3 --warmup 1 --no-cpu-baseline --no-c2 > $OUT/prof_feti.log 2>&1
# keep only the stats summaries (kernel traces are large)
find $OUT/prof_c2 $OUT/prof_feti -name "*kernel_trace.csv" -delete
find $OUT -name "*kernel_stats.csv" | head
