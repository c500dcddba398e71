# A/B of the lookup kernel's lanes-per-row split (DR_LOOKUP_SPLIT): headline
# and DeepFM roofline fractions, alternating runs.
set -o pipefail
OUT=${OUT:-bench_out}   # where the logs and result lines go
mkdir -p $OUT/split
for r in 1 2; do
  for S in 1 2; do
    DR_LOOKUP_SPLIT=$S timeout -k 10 300 python -u bench.py --full --cpu-seconds 0 --train-steps 0 > $OUT/split/b_${S}_$r.json 2> $OUT/split/b_${S}_$r.err || exit 1
    python3 -c "
import json;d=json.load(open('$OUT/split/b_${S}_$r.json'))
print('split',$S,'run',$r,'headline',d['roofline']['frac'],d['roofline']['kernel_ms'],'deepfm',d['deepfm_config']['roofline']['frac'],d['deepfm_config']['roofline']['kernel_ms'])"
  done
done
