# xgmi engine at N = 1 on itself, with and without per-destination dedup, on
# uniform and Zipf(1.05) keys (bench.py legs off), then the 2-rank rehearsal
# tests.  Tag $1.
set -o pipefail
OUT=${OUT:-bench_out}   # where the logs and result lines go
T=${1:-dd}
mkdir -p $OUT/$T
B="python -u bench.py --full --engine xgmi --no-deepfm --no-criteo --no-dcn --train-steps 0 --cpu-seconds 0 --steps 20"
for z in 0 1.05; do
  for d in "" "--dedup"; do
    n=z${z}${d}
    timeout -k 10 300 $B --zipf $z $d > $OUT/$T/$n.json 2> $OUT/$T/$n.err || exit 1
    python3 -c "import json;d=json.load(open('$OUT/$T/$n.json'));print('$n',d['ms_per_step'],d['value'],d['config']['engine'],d['config']['engine_check'])"
  done
done
timeout -k 10 500 python -u -m pytest tests/test_gpu_bench_rehearsal.py -m gpu -x -q --timeout 200 --timeout-method thread > $OUT/$T/rehearsal.log 2>&1
rc=$?; tail -3 $OUT/$T/rehearsal.log; exit $rc
