cd $GRAFT_REPO_ROOT
OUT=${OUT:-prof_out}; mkdir -p $OUT; export OUT      # output folder (git-ignored default)
timeout 900 python bench.py --full --steps 20 --warmup 5 > $OUT/bench_driver_style.json 2> $OUT/bench_driver_style.err
tail -c 3000 $OUT/bench_driver_style.err
timeout 900 python bench.py --full --config c3 --no-extras --no-cpu-baseline > $OUT/bench_c3.json 2> $OUT/bench_c3.err
timeout 900 python bench.py --full --config c5 --no-extras --no-cpu-baseline > $OUT/bench_c5.json 2> $OUT/bench_c5.err
python - <<'PY'
import json, os
for f in ("bench_driver_style", "bench_c3", "bench_c5"):
    try:
        d = json.loads([l for l in open(f"{os.environ['OUT']}/{f}.json") if l.startswith("{")][-1])
        print(f, d["value"], d["ms_per_step"], d["config"]["launch"][:40], d.get("per_layer_launch"), {k: d["roofline"][k] for k in ("frac", "avg_launch_us", "us_per_layer_step", "traffic")})
        if "cpu_baseline" in d:
            c = d["cpu_baseline"]; print("  cpu", c["value"], c["cores"], c["spread"], c.get("best_of_thread_counts"), c["one_thread"]["torch_mirror"]["value"], c["one_thread"].get("c_port", {}).get("value"))
        if "extras" in d:
            e = d["extras"]; print("  extras", {k: e[k] for k in e if "speedup" in k or "prefill_8192_causal_TF" in k or k == "per_rank_launch_us"})
    except Exception as e:
        print(f, "ERR", e)
PY
