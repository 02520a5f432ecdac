# Round-2 profile set: rocprofv3 kernel trace of the bench command, PMC traffic of the decode kernel, kernel trace of
# the prefill probe.  Writes under $OUT/ (the PMC pass where tools/pmc_decode.sh writes; copy into profiles/ as r02_*).
cd /tmp && export TMPDIR=/tmp
R=$GRAFT_REPO_ROOT
OUT=${OUT:-$R/prof_out}; mkdir -p $OUT; export OUT      # output folder (git-ignored default)
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_bench -o bench -- python $R/bench.py --full --steps 256 --warmup 64 --no-cpu-baseline --no-extras > $OUT/prof_bench.log 2>&1
grep "^{\"metric\"" $OUT/prof_bench.log | tail -1 > $OUT/r02_bench_line_under_rocprof.json
python $R/tools/trim_stats.py $(find $OUT/prof_bench -name "*kernel_stats.csv" | head -1) $OUT/r02_bench_kernel_stats.csv
head -8 $OUT/r02_bench_kernel_stats.csv | cut -c1-200
bash $R/tools/pmc_decode.sh 2081 > $R/gpurun_out/pmc_decode.log 2>&1
cp $R/gpurun_out/pmc_decode.json $R/gpurun_out/r02_pmc_decode.json
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_pf -o pf -- python $R/tools/probe_prefill.py > $OUT/r02_prefill_probe_under_rocprof.txt 2>&1
python $R/tools/trim_stats.py $(find $OUT/prof_pf -name "*kernel_stats.csv" | head -1) $OUT/r02_prefill_kernel_stats.csv
