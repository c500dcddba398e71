# usage: bash tools/gpu_run1.sh TAG  -- GPU test suite, then bench.py, then a rocprof kernel-stats pass of bench
set -o pipefail
OUT=${OUT:-bench_out}   # where the logs and result lines go
T=${1:-x}
mkdir -p $OUT
timeout -k 10 500 python -u -m pytest tests -m gpu -x -q --timeout 200 --timeout-method thread > $OUT/gpu_tests_$T.log 2>&1
rc=$?
tail -25 $OUT/gpu_tests_$T.log
[ $rc -ne 0 ] && exit $rc
timeout -k 10 400 python -u bench.py --full > $OUT/bench_$T.json 2> $OUT/bench_$T.err
rc=$?
tail -20 $OUT/bench_$T.err; cat $OUT/bench_$T.json
[ $rc -ne 0 ] && exit $rc
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_$T -o run -- python3 bench.py --full --cpu-seconds 0 --steps 10 --warmup 3 > $OUT/bench_prof_$T.log 2>&1
rc=$?
tail -3 $OUT/bench_prof_$T.log
exit $rc
