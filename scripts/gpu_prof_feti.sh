# rocprofv3 kernel stats of the configs[2] bench step (MG-preconditioned K^+); summary only
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${OUT:-$R/out}  # where the runs below write
mkdir -p "$OUT"
mkdir -p $OUT
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_feti_mg -- python3 $R/bench.py --full --steps 6 --warmup 1 --no-cpu-baseline --no-c2 > $OUT/prof_feti_mg.log 2>&1
find $OUT/prof_feti_mg -name "*kernel_trace.csv" -delete
find $OUT/prof_feti_mg -name "*kernel_stats.csv" | head
