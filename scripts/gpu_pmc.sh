# HBM traffic of the dominant kernel from PMC counters (separate passes, as MI355X_MICROARCH.md prescribes)
set -x
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${OUT:-$R/out}  # where the runs below write
mkdir -p "$OUT"
cd /tmp && export TMPDIR=/tmp
for C in FETCH_SIZE WRITE_SIZE; do
  rocprofv3 --pmc $C --kernel-trace --output-format csv -d $OUT/pmc_$C -- python3 $R/bench.py --full --steps 48 --warmup 4 --no-cpu-baseline > $OUT/pmc_$C.log 2>&1
  tail -1 $OUT/pmc_$C.log | cut -c1-200
done
python3 $R/scripts/pmc_parse.py $OUT
