# Round measurement: GPU test suite, full bench line, rocprofv3 kernel stats of
# a short bench, and the dominant kernel's FETCH_SIZE / WRITE_SIZE in separate
# --pmc passes (summarised on the host by tools/pmc_summary.py).  Tag $1.
set -o pipefail
OUT=${OUT:-bench_out}   # where the logs and result lines go
T=${1:-final}
mkdir -p $OUT/$T
timeout -k 10 500 python -u -m pytest tests -m gpu -x -q --timeout 200 --timeout-method thread > $OUT/$T/gpu_tests.log 2>&1
rc=$?; tail -3 $OUT/$T/gpu_tests.log; [ $rc -ne 0 ] && exit $rc
timeout -k 10 400 python -u bench.py --full > $OUT/$T/bench.json 2> $OUT/$T/bench.err
rc=$?; tail -2 $OUT/$T/bench.err; [ $rc -ne 0 ] && exit $rc
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
B="bench.py --full --no-graph --steps 2 --kernel-iters 3 --cpu-seconds 0 --train-steps 0 --no-deepfm --no-criteo --no-dcn"
# kernel stats of the headline path (steps + checks + the dominant kernel's timing loop)
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/$T/stats -o run -- python3 bench.py --full --cpu-seconds 0 --steps 10 --warmup 3 --train-steps 0 --no-deepfm --no-criteo --no-dcn > $OUT/$T/prof.log 2>&1 || exit 1
timeout -s KILL 200 rocprofv3 --pmc FETCH_SIZE --output-format csv -d $OUT/$T/fetch -o run -- python3 $B > $OUT/$T/fetch.log 2>&1 || exit 1
timeout -s KILL 200 rocprofv3 --pmc WRITE_SIZE --output-format csv -d $OUT/$T/write -o run -- python3 $B > $OUT/$T/write.log 2>&1 || exit 1
echo measured
