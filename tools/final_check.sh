#!/bin/bash
# The end-of-work sequence, on the GPU box from the repo root:  bash tools/final_check.sh <outdir>
# Every step is joined with && -- a step that fails or is killed at its limit ends the call, no further GPU step behind it.
# The plain bench line is the headline figure alone; the --full line adds the roofline and the sub-records.
OUT=${1:?usage: bash tools/final_check.sh <outdir>}
mkdir -p "$OUT" &&
timeout -k 10 850 python -m pytest tests -m gpu -q -x --durations=8 > "$OUT/final_pytest.log" 2>&1 && tail -2 "$OUT/final_pytest.log" &&
timeout -k 10 120 python -c "import __graft_entry__ as g; g.smoke()" 2>&1 | tail -1 &&
timeout -k 10 300 python3 bench.py --gpus 1 --steps 20 --warmup 5 > "$OUT/final_bench.json" 2> "$OUT/final_bench.err" &&
timeout -k 10 600 python3 bench.py --gpus 1 --steps 20 --warmup 5 --full > "$OUT/final_bench_full.json" 2> "$OUT/final_bench_full.err" &&
python3 - "$OUT" <<'PY'
import json, os, sys
line = lambda name: json.loads(open(os.path.join(sys.argv[1], name)).read().strip().splitlines()[-1])
o, f = line("final_bench.json"), line("final_bench_full.json")
print(o["value"], o["unit"], o["ms_per_step"], "| --full:", f["value"], "roofline", f["roofline"]["frac"], "traffic", f["roofline"]["traffic"],
      "sub-record errors", f["config"].get("sub_record_errors"))
PY
