#!/bin/bash
# Refresh the round's evidence under <outdir> (run on the GPU box from the repo root; copy what is to be judged into
# profiles/ with tools/publish_profiles.sh).  Four parts, each within one visit to the box:
#   bash tools/collect_round.sh bench <outdir>   --full bench lines of every workload (cfg3 with its sub-records, cfg4, cfg2, cfg5, cfg3-f32)
#   bash tools/collect_round.sh stats <outdir>    rocprofv3 --kernel-trace --stats of cfg3 / cfg4 / cfg5 / cfg2, the iteration timeline
#   bash tools/collect_round.sh pmc <outdir>      FETCH_SIZE / WRITE_SIZE of every workload, matrix-pipe counters of the factorisation
#   bash tools/collect_round.sh gram <outdir>     the dense MFMA Gram (general-w path): kernel stats of a bench run WITH gram_general_path, SQ counters of gram_kernel
set -x
set -e   # a step that fails or is killed at its limit ends the call: no further GPU step behind it
PART=${1:-bench}
P=${2:?usage: bash tools/collect_round.sh bench|stats|pmc|gram <outdir>}
R=$(pwd)
mkdir -p "$R/$P"
cd "$R"
if [ "$PART" = bench ]; then
  timeout -k 10 400 python bench.py --full > $P/bench_cfg3.json 2> $P/bench_cfg3.err
  timeout -k 10 300 python bench.py --full --workload cfg4 > $P/bench_cfg4.json 2> $P/bench_cfg4.err
  timeout -k 10 300 python bench.py --full --workload cfg2 > $P/bench_cfg2.json 2> $P/bench_cfg2.err
  timeout -k 10 400 python bench.py --full --workload cfg5 > $P/bench_cfg5.json 2> $P/bench_cfg5.err
  timeout -k 10 300 python bench.py --full --dtype f32 --no-cpu-baseline --no-general-path --no-cfg4-strong --no-single-process > $P/bench_cfg3_f32.json 2> $P/bench_cfg3_f32.err
elif [ "$PART" = stats ]; then
  cd /tmp && export TMPDIR=/tmp
  timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$R/$P/k3" -o bench -- python3 "$R/bench.py" --steps 4 --warmup 1 --no-cpu-baseline --no-general-path --no-alt-storage --no-cfg4-strong --no-baseline-configs --no-concurrent --no-single-process > "$R/$P/k3.log" 2>&1
  timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$R/$P/k4" -o bench -- python3 "$R/bench.py" --workload cfg4 --steps 1 --warmup 1 --no-cpu-baseline > "$R/$P/k4.log" 2>&1
  timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$R/$P/k5" -o bench -- python3 "$R/bench.py" --workload cfg5 --steps 1 --warmup 0 --iters 500 --no-cpu-baseline > "$R/$P/k5.log" 2>&1
  timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$R/$P/k2" -o bench -- python3 "$R/bench.py" --workload cfg2 --steps 2 --warmup 1 --no-cpu-baseline --no-concurrent > "$R/$P/k2.log" 2>&1
  cd "$R"
  for k in k3 k4 k5 k2; do F=$(find $P/$k -name "*kernel_stats.csv" | head -1); python tools/trim_stats.py "$F" $P/${k}_kernel_stats.csv > /dev/null; rm -rf $P/$k; done
  timeout -k 10 120 python tools/iter_timeline.py > $P/iteration_timeline.txt 2> $P/iteration_timeline.err
elif [ "$PART" = gram ]; then
  cd /tmp && export TMPDIR=/tmp
  timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d "$R/$P/kg" -o bench -- python3 "$R/bench.py" --full --steps 2 --warmup 1 --no-cpu-baseline --no-alt-storage --no-cfg4-strong --no-baseline-configs --no-concurrent --no-single-process > "$R/$P/kg.log" 2>&1
  cd "$R"
  F=$(find $P/kg -name "*kernel_stats.csv" | head -1); python tools/trim_stats.py "$F" $P/kg_kernel_stats.csv > /dev/null; rm -rf $P/kg
  bash tools/collect_mfma_pmc.sh $P/pmc_gram > $P/pmc_gram.log 2>&1
else
  bash tools/collect_pmc.sh $P/pmc cfg3 > $P/pmc.log 2>&1
  for w in cfg2 cfg4 cfg5; do bash tools/collect_pmc.sh $P/pmc_$w $w > $P/pmc_$w.log 2>&1; done
  bash tools/collect_factor_pmc.sh $P/pmc_factor 8192 > $P/pmc_factor.log 2>&1
fi
ls -la $P
