#!/bin/bash
# End-of-round validation on the GPU box: the whole GPU suite, the full bench line, the strong-scaling line on one GPU,
# the 64..128-state timings.  Results under OUTDIR (the E-step profiles where tools/collect_profiles.sh writes them).
#   bash tools/final_run.sh OUTDIR
mkdir -p "${1:?usage: bash tools/final_run.sh OUTDIR}" && out=$(cd "$1" && pwd) || exit 1
cd "$(dirname "$0")/.." || exit 1
python -m pytest tests -x -q -m gpu > "$out"/r3_full8.log 2>&1; echo "pytest rc=$?"; tail -n 3 "$out"/r3_full8.log
python bench.py --full > "$out"/r03_bench_default.json 2> "$out"/r03_bench_default.err; echo "bench rc=$?"
python bench.py --scaling strong --full --no-extra > "$out"/r03_bench_strong_1gpu.json 2> "$out"/r03_bench_strong.err; echo "strong rc=$?"
python tools/config5_bench.py > "$out"/r03_config5.txt 2>&1; echo "c5 rc=$?"
python __graft_entry__.py --smoke > "$out"/smoke.log 2>&1; echo "smoke rc=$?"; tail -n 2 "$out"/smoke.log
bash tools/collect_profiles.sh r03 estep; echo "estep profile rc=$?"
