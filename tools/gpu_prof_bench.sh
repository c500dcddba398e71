set -o pipefail
OUT=${OUT:-bench_out}   # where the logs and result lines go
mkdir -p $OUT
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
timeout -k 10 200 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_train_r2 -o run -- python3 tools/train_probe.py --graph > $OUT/train_prof_r2.log 2>&1
rc=$?; tail -3 $OUT/train_prof_r2.log; [ $rc -ne 0 ] && exit $rc
timeout -k 10 400 python -u bench.py --full > $OUT/bench_r2.json 2> $OUT/bench_r2.err
rc=$?; tail -5 $OUT/bench_r2.err; cat $OUT/bench_r2.json; exit $rc
