#!/bin/bash
# run on the GPU box from the repo root:  scripts/evidence6.sh r06x   - the sweep kernel's evidence set (configs 6, 7, 8, 1) beside the headline's
R=${1:-r06}
OUT=${OUT:-evidence}  # output root, relative to the repo root
mkdir -p $OUT/$R
REPO=$(pwd)
for c in 6 7; do
  bash scripts/pmc_passes.sh $OUT/$R/pmc$c -- python3 $REPO/bench.py --config $c --steps 10 --warmup 2 --no-cpu --new-frames 0 --no-e2e --no-verify > $OUT/$R/pmc$c.log 2>&1
  cp $OUT/$R/pmc$c/summary.txt $OUT/$R/bench_config${c}_pmc_summary.txt
  python3 scripts/traffic.py $OUT/$R/bench_config${c}_pmc_summary.txt "profiles/${R}_bench_config${c}_pmc_summary.txt" "4096x4096 / $([ $c = 6 ] && echo 64 || echo 32)-px patches, 1 GPU" > $OUT/$R/traffic_config$c.json
  cp $OUT/$R/traffic_config$c.json profiles/traffic_config$c.json
  rm -rf $OUT/$R/pmc$c/pass*
done
python bench.py --full --steps 50 --warmup 5 > $OUT/$R/bench.json 2> $OUT/$R/bench.err; cut -c1-400 $OUT/$R/bench.json
for c in 6 7 8; do python bench.py --full --config $c --steps 50 --warmup 5 --no-cpu > $OUT/$R/bench_config$c.json 2>/dev/null; cut -c1-250 $OUT/$R/bench_config$c.json; done
python bench.py --full --config 1 --steps 50 --warmup 5 --new-frames 0 > $OUT/$R/bench_config1.json 2>/dev/null; cut -c1-250 $OUT/$R/bench_config1.json
python scripts/notebook_workload.py > $OUT/$R/notebook_workload.log 2>&1; grep frames $OUT/$R/notebook_workload.log
for c in 6 7; do
  (cd /tmp && export TMPDIR=/tmp && rocprofv3 --kernel-trace --stats --output-format csv -d $REPO/$OUT/$R/stats$c -- python3 $REPO/bench.py --config $c --steps 100 --warmup 5 --no-cpu --new-frames 0 --no-e2e --no-verify > $REPO/$OUT/$R/stats$c.log 2>&1)
  find $OUT/$R/stats$c -name "*kernel_stats.csv" | head -1 | xargs -I{} cp {} $OUT/$R/bench_config${c}_kernel_stats.csv
  head -3 $OUT/$R/bench_config${c}_kernel_stats.csv
  rm -rf $OUT/$R/stats$c
done
