# rows-path GPU check: its tests, the whole GPU suite, train probe (eager,
# graph), rocprof of the graph probe, bench
set -o pipefail
OUT=${OUT:-bench_out}   # where the logs and result lines go
T=${1:-x}
mkdir -p $OUT
timeout -k 10 300 python -u -m pytest tests/test_gpu_rows_grad.py -x -v --timeout 120 --timeout-method thread > $OUT/rows_tests_$T.log 2>&1
rc=$?; tail -30 $OUT/rows_tests_$T.log; [ $rc -ne 0 ] && exit $rc
timeout -k 10 400 python -u -m pytest tests -m gpu -x -q --timeout 200 --timeout-method thread > $OUT/gpu_tests_$T.log 2>&1
rc=$?; tail -5 $OUT/gpu_tests_$T.log; [ $rc -ne 0 ] && exit $rc
timeout -k 10 200 python -u tools/train_probe.py > $OUT/train_$T.log 2>&1 && \
timeout -k 10 200 python -u tools/train_probe.py --graph >> $OUT/train_$T.log 2>&1
rc=$?; cat $OUT/train_$T.log; [ $rc -ne 0 ] && exit $rc
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
timeout -k 10 200 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_train_$T -o run -- python3 tools/train_probe.py --graph > $OUT/train_prof_$T.log 2>&1
rc=$?; [ $rc -ne 0 ] && exit $rc
timeout -k 10 400 python -u bench.py --full > $OUT/bench_$T.json 2> $OUT/bench_$T.err
rc=$?; tail -5 $OUT/bench_$T.err; cat $OUT/bench_$T.json; exit $rc
