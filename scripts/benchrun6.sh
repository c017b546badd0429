R=r06s
OUT=${OUT:-evidence}  # output root, relative to the repo root
mkdir -p $OUT/$R
python bench.py --full --steps 50 --warmup 5 > $OUT/$R/bench.json 2> $OUT/$R/bench.err; cut -c1-300 $OUT/$R/bench.json; tail -3 $OUT/$R/bench.err
for c in 6 7 8; do python bench.py --full --config $c --steps 50 --warmup 5 --no-cpu > $OUT/$R/bench_config$c.json 2>$OUT/$R/bench_config$c.err; cut -c1-200 $OUT/$R/bench_config$c.json; tail -2 $OUT/$R/bench_config$c.err; done
python bench.py --full --config 1 --steps 50 --warmup 5 --new-frames 0 > $OUT/$R/bench_config1.json 2>/dev/null; cut -c1-200 $OUT/$R/bench_config1.json
python bench.py --full --config 2 --steps 50 --warmup 5 --no-cpu > $OUT/$R/bench_config2.json 2>/dev/null; cut -c1-200 $OUT/$R/bench_config2.json
