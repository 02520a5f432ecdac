# the bench lines of the final build (default, driver-style, c3, c5) and the round-5 profile set (tools/prof_r05.sh); outputs in $OUT/
cd $GRAFT_REPO_ROOT
OUT=${OUT:-prof_out}; mkdir -p $OUT; export OUT      # output folder (git-ignored default)
python bench.py --full > $OUT/r05_bench_default_run.json 2> $OUT/bench_default.err
python bench.py --full --steps 20 --warmup 5 --no-cpu-baseline > $OUT/r05_bench_driver_style.json 2>/dev/null
python bench.py --full --config c3 --no-cpu-baseline --no-extras 2>/dev/null | grep '^{' > $OUT/r05_bench_c3.json
python bench.py --full --config c5 --no-cpu-baseline --no-extras 2>/dev/null | grep '^{' > $OUT/r05_bench_c5.json
bash tools/prof_r05.sh > $OUT/prof_r05.log 2>&1
tail -3 $OUT/prof_r05.log
