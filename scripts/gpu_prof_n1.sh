# kernel stats per step of the default N=1 workload: difference of a 22- and a 12-step run = 10 steps
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${OUT:-$R/out}  # where the runs below write
mkdir -p "$OUT"
cd /tmp && export TMPDIR=/tmp
for n in 12 22; do
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/n1_$n -- python3 $R/bench.py --full --steps $n --warmup 2 --no-cpu-baseline --no-c2 > $OUT/n1_$n.json 2> $OUT/n1_$n.err
find $OUT/n1_$n -name "*kernel_trace.csv" -delete
done
