# GPU-busy time per bench step: kernel-time difference of a 22-step and a 12-step run (same set-up)
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${OUT:-$R/out}  # where the runs below write
mkdir -p "$OUT"
cd /tmp && export TMPDIR=/tmp
for n in 12 22; do
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/busy_$n -- python3 $R/bench.py --full --steps $n --warmup 2 --no-cpu-baseline --no-c2 > $OUT/busy_$n.json 2> $OUT/busy_$n.err
find $OUT/busy_$n -name "*kernel_trace.csv" -delete
done
