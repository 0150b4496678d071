# kernel stats of the 1-block-per-GPU rehearsal (rank 0's share of an 8-GPU run): difference of a 22- and a 12-step run = 10 steps
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${OUT:-$R/out}  # where the runs below write
mkdir -p "$OUT"
cd /tmp && export TMPDIR=/tmp
for n in 12 22; do
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/reh8_$n -- python3 $R/bench.py --full --sim-world 8 --steps $n --warmup 2 --no-cpu-baseline --no-c2 > $OUT/reh8_$n.json 2> $OUT/reh8_$n.err
find $OUT/reh8_$n -name "*kernel_trace.csv" -delete
done
