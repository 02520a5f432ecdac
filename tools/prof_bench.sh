# rocprofv3 kernel trace of the bench command; trimmed stats summary -> $OUT/ (copy into profiles/)
cd /tmp && export TMPDIR=/tmp
R=$GRAFT_REPO_ROOT
OUT=${OUT:-$R/prof_out}; mkdir -p $OUT; export OUT      # output folder (git-ignored default)
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_bench -o bench -- python $R/bench.py --full --steps 256 --warmup 64 --no-cpu-baseline --no-extras > $OUT/prof_bench.log 2>&1
grep "^{\"metric\"" $OUT/prof_bench.log | tail -1 > $OUT/bench_line_under_rocprof.json
python $R/tools/trim_stats.py $(find $OUT/prof_bench -name "*kernel_stats.csv" | head -1) $OUT/bench_kernel_stats.csv
head -8 $OUT/bench_kernel_stats.csv | cut -c1-200
