# final check of a build: the whole GPU suite, smoke, the default bench line and the paired bench line (both with --full: their CPU
# baselines and the legs beside the headline) -> $OUT (default bench_out/final_check under the repository root)
set -e
cd "$(dirname "$0")/.."
OUT=${OUT:-bench_out/final_check}
mkdir -p $OUT
timeout -k 10 1000 python3 -m pytest tests -m gpu -x -q > $OUT/pytest_gpu.log 2>&1 || { tail -60 $OUT/pytest_gpu.log; exit 1; }
tail -2 $OUT/pytest_gpu.log
timeout -k 10 200 python3 -c "import __graft_entry__ as g; g.smoke()" 2>&1 | tail -1
timeout -k 10 500 python3 bench.py --full > $OUT/bench_default.json 2> $OUT/bench_default.log
OUT=$OUT python3 - <<'PY'
import json, os
d = json.loads(open(os.path.join(os.environ["OUT"], "bench_default.json")).read().strip().splitlines()[-1])
print("default", round(d["value"] / 1e6, 2), "M reads/s", round(d["ms_per_step"], 1), "ms; roofline", round(d["roofline"]["frac"], 3), "survey", round(d["roofline"]["survey_8d"]["frac"], 3), "cpu", round(d["cpu_baseline"]["value"]), d["cpu_baseline"]["sam_identical_on_sample"], "from_host", round(d["from_host"]["value"] / 1e6, 2), round(d["from_host"]["two_contexts"]["value"] / 1e6, 2))
PY
timeout -k 10 500 python3 bench.py --paired --full > $OUT/bench_paired.json 2> $OUT/bench_paired.log || { tail -20 $OUT/bench_paired.log; exit 1; }
OUT=$OUT python3 - <<'PY'
import json, os
d = json.loads(open(os.path.join(os.environ["OUT"], "bench_paired.json")).read().strip().splitlines()[-1])
print("paired", round(d["value"] / 1e6, 3), "M pairs/s", round(d["ms_per_step"], 1), "ms", d["stages_s_per_step"], "from_host", d.get("from_host"), "cpu", d.get("cpu_baseline", {}).get("value"), d.get("cpu_baseline", {}).get("sam_identical_on_sample"), d.get("cpu_baseline", {}).get("model_identical"))
PY
