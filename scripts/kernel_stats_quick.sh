# Usage (on the GPU box): scripts/kernel_stats_quick.sh -- rocprofv3 kernel stats of one short `bench.py --full` run (inverse,
# forward and training-step kernels) and the three launch times of its line; output under $OUT_ROOT (default results/)
set -e
ROOT=$PWD
OUT=${OUT_ROOT:-$ROOT/results}
mkdir -p $OUT
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/gwprof -- python3 $ROOT/bench.py --full --no-cpu --no-share --steps 40 > $OUT/gw_bench.json 2> $OUT/gw.err
cd $ROOT
f=$(find $OUT/gwprof -name "*kernel_stats.csv" | head -1)
head -5 $f | cut -c1-230
rm -rf $OUT/gwprof
python3 -c "
import json; d=json.load(open('$OUT/gw_bench.json')); print('inv', d['roofline']['launch_ms'], 'fwd', d['forward']['launch_ms'], 'train', d['training_step']['ms_per_step'])"
