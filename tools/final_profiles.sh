#!/bin/bash
# The tracked evidence of a round at the CURRENT kernel sources.  Run ON THE GPU BOX from the repo root (two gpurun calls fit
# the 20-minute limit):   bash tools/final_profiles.sh r03 pmc     then     bash tools/final_profiles.sh r03 bench <out_dir>
#   pmc:   counter passes per bench leg (tools/pmc_legs.sh) and for the scorer (tools/pmc_scorer.sh)
#          -> gpurun_out/<round>_<leg>_pmc_counters.json, <round>_scorer_pmc.json      (copy them into profiles/ and commit)
#   bench: rocprofv3 --kernel-trace --stats of `bench.py --full` -> <out_dir>/<round>_kernel_stats.csv, then the
#          `bench.py --full` line (which quotes the counter summaries found under profiles/) -> <out_dir>/<round>_bench.json
set -e -o pipefail
R=${1:-r03}; WHAT=${2:-pmc}
ROOT=$(cd "$(dirname "$0")/.." && pwd)
cd "$ROOT"
if [ "$WHAT" = pmc ]; then
  shift; shift || true
  LEGS=${@:-"c2 c3 c4 c5 drn_train"}
  bash tools/pmc_legs.sh "$R" $LEGS
  for leg in $LEGS; do cp "profiles/${R}_${leg}_pmc_counters.json" gpurun_out/; done
  bash tools/pmc_scorer.sh "$R"
  ls -la gpurun_out/${R}_*pmc*.json
else
  OUT=${3:?usage: final_profiles.sh <round> bench <out_dir>}
  mkdir -p "$OUT" && OUT=$(cd "$OUT" && pwd)
  cd /tmp && export TMPDIR=/tmp
  rm -rf "$OUT/kstats"
  timeout -k 10 500 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/kstats" -o ks -- python3 "$ROOT/bench.py" --full --no-cpu-baseline > "$OUT/kstats.log" 2>&1 || { tail -5 "$OUT/kstats.log"; exit 1; }
  cd "$ROOT"
  find "$OUT/kstats" -name "*kernel_stats.csv" -exec cp {} "$OUT/${R}_kernel_stats.csv" \;
  rm -rf "$OUT/kstats"
  timeout -k 10 500 python3 bench.py --full > "$OUT/bench_final.log" 2>&1 || { tail -5 "$OUT/bench_final.log"; exit 1; }
  tail -n 1 "$OUT/bench_final.log" > "$OUT/${R}_bench.json"
  tail -c 400 "$OUT/bench_final.log"
  ls -la "$OUT/${R}_kernel_stats.csv" "$OUT/${R}_bench.json"
fi
