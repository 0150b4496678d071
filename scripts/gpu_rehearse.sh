# strong-scaling rehearsal on ONE GPU: rank 0's share of an N-GPU run (8/N blocks, no collective), plain timing + kernel stats at N=8
set -x
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${OUT:-$R/out}  # where the runs below write
mkdir -p "$OUT"
mkdir -p $OUT
for n in 1 2 4 8; do
  python3 $R/bench.py --full --sim-world $n --steps 20 --warmup 2 --no-cpu-baseline --no-c2 > $OUT/reh_$n.json 2> $OUT/reh_$n.err
  python3 -c "import json;d=json.load(open('$OUT/reh_$n.json'));print('sim-world',$n,'ms/step',d['ms_per_step'])"
done
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_reh8 -- python3 $R/bench.py --full --sim-world 8 --steps 20 --warmup 2 --no-cpu-baseline --no-c2 > $OUT/prof_reh8.log 2>&1
find $OUT/prof_reh8 -name "*kernel_trace.csv" -delete
find $OUT/prof_reh8 -name "*kernel_stats.csv"
