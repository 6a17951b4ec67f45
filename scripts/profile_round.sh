#!/bin/bash
# Usage (on the GPU box): scripts/profile_round.sh <tag> [benches|pmc]
# The round's judged evidence: `benches` -- bench lines (c3 default, c2, c5, c3_share8, c4, ref_timing), the other timing scripts and
# rocprofv3 kernel stats of the same bench command for c3, c3_share8 and c5; `pmc` -- the PMC passes for c3 (wavefront kernel),
# c3_share8 (role-split kernel, band split) and c5 (K-split inverse, F(2,5) forward).  Everything lands in $OUT_ROOT/<tag>/
# (default results/<tag>/); copy what is to be judged into profiles/.  The bench lines are `--full` ones: forward, training step,
# clock and the other legs beside the headline.  (rocprofv3 gets `python3 bench.py` directly after `--`; the profiled runs skip the
# clock probe, a kernel that runs beside the legs for their whole length.)
set -e
TAG=$1
WHAT=${2:-benches}
ROOT=${GRAFT_REPO_ROOT:-$(pwd)}
cd $ROOT
RES=${OUT_ROOT:-$ROOT/results}
OUT=$RES/${TAG}
mkdir -p $OUT
if [ "$WHAT" = "benches" ]; then
  python3 bench.py --full > $OUT/bench_c3.json 2> $OUT/bench_c3.err
  echo "bench c3 done"
  for w in c2 c5 c3_share8; do
    python3 bench.py --workload $w --steps 50 --full --no-cpu > $OUT/bench_$w.json 2>> $OUT/bench.err
    echo "bench $w done"
  done
  python3 bench.py --workload c4 --steps 20 --warmup 3 --full --no-cpu > $OUT/bench_c4.json 2>> $OUT/bench.err
  echo "bench c4 done"
  python3 bench.py --workload ref_timing > $OUT/bench_ref_timing_block16.json 2>> $OUT/bench.err
  python3 bench.py --workload ref_timing --ref-block-size 48 > $OUT/bench_ref_timing_block48.json 2>> $OUT/bench.err
  echo "ref_timing done"
  python3 scripts/f3_measure.py > $OUT/f3.json 2>> $OUT/bench.err
  python3 scripts/debug_big.py time > $OUT/big_banks.txt 2>> $OUT/bench.err
  python3 scripts/time_small.py > $OUT/small_batch.txt 2>> $OUT/bench.err
  python3 scripts/time_f64.py > $OUT/fp64_mfma.txt 2>> $OUT/bench.err
  scripts/chain_vs_split.sh > $OUT/chain_vs_split.txt 2>> $OUT/bench.err
  scripts/tiny_prof2.sh > $OUT/tiny_maps_kernel_time.txt 2>> $OUT/bench.err
  echo "other timings done"
  cd /tmp && export TMPDIR=/tmp
  for w in c3 c2 c3_share8 c5; do
    rocprofv3 --kernel-trace --stats --output-format csv -d $RES/${TAG}_prof_$w -- python3 $ROOT/bench.py --workload $w --full --no-cpu --no-share --no-clock > $OUT/bench_${w}_under_rocprof.json 2> $OUT/prof_$w.err
    cp $(find $RES/${TAG}_prof_$w -name "*kernel_stats.csv" | head -1) $OUT/${w}_kernel_stats.csv
    rm -rf $RES/${TAG}_prof_$w
    echo "rocprof $w done"
  done
else
  for w in c3 c2 c3_share8 c5; do
    scripts/pmc_run.sh ${TAG}_$w --workload $w --no-clock > $OUT/pmc_$w.log 2>&1
    cp $RES/pmc_${TAG}_$w/summary.json $OUT/${w}_pmc_summary.json
    rm -rf $RES/pmc_${TAG}_$w
    echo "pmc $w done"
  done
fi
ls -la $OUT
