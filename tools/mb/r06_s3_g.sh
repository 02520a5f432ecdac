# session 3, call G: profile set of the grouped-query step, the chain's finer stamps on the final build, the driver-style bench line
cd $GRAFT_REPO_ROOT
OUT=${OUT:-prof_out}; mkdir -p $OUT; export OUT      # output folder (git-ignored default)
bash tools/prof_r06_gqa.sh
cd $GRAFT_REPO_ROOT
SPATTEN_LIB=$PWD/tools/mb/ab/lib_chaintrace.so timeout 300 python tools/mb/chain_trace.py 32 2081 32 2>&1 | grep -v amdgpu.ids > $OUT/r06_chain_phase_stamps.txt
tail -14 $OUT/r06_chain_phase_stamps.txt
timeout 1200 python bench.py --full --steps 20 --warmup 5 > $OUT/bench_driver_style.log 2>&1
grep "^{\"metric\"" $OUT/bench_driver_style.log | tail -1 > $OUT/r06_bench_driver_style.json
python - <<'PY'
import json, os
d = json.loads(open(os.environ["OUT"] + "/r06_bench_driver_style.json").read())
print(d["value"], d["ms_per_step"], d["roofline"]["frac"], d["per_layer_launch"]["tokens_per_s"])
print({k: v for k, v in d["extras"].items() if k.startswith("gqa") or "error" in k})
print(d["cpu_baseline"]["value"], d["cpu_baseline"]["cores"])
PY
