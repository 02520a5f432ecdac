cd $GRAFT_REPO_ROOT
OUT=${OUT:-prof_out}; mkdir -p $OUT; export OUT      # output folder (git-ignored default)
timeout 1500 python -m pytest tests/test_gpu_pq_profiles.py tests/test_gpu_graph_decode.py tests/test_gpu_fullsize.py -x -q 2>&1 | tail -4 > $OUT/c5_tests.log
for c in 128 256 512 1024; do
SPATTEN_PQV_COMPACT=$c timeout 900 python bench.py --full --config c5 --no-extras --no-cpu-baseline > $OUT/bench_c5_$c.json 2> $OUT/bench_c5_$c.err
python - <<PY >> $OUT/c5_tests.log
import json
d = json.loads([l for l in open("$OUT/bench_c5_$c.json") if l.startswith("{")][-1])
print("compact=$c", d["value"], d["ms_per_step"], d["config"]["pq_confidence"]["uniform_tokens_per_s"], d["roofline"]["avg_launch_us"])
PY
done
cat $OUT/c5_tests.log
