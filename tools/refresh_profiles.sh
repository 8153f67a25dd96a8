#!/bin/bash
# usage (after tools/profile_round.sh TAG has run on the GPU box and its $OUT_DIR/ is here): [OUT_DIR=results] bash tools/refresh_profiles.sh TAG OUT
# -> profiles/OUT_* (kernel stats + summaries of cfg3 / cfg2 / cfg4 / cfg5, SQ counter table, bench line) and profiles/<round>_traffic.json
TAG=${1:-r02}; OUT=${2:-r02_final}; OUT_DIR=${OUT_DIR:-results}
cd "$(dirname "$0")/.." || exit 1
python3 tools/summarize_rocprof.py $OUT $OUT_DIR/prof_$TAG $OUT_DIR/pmc_fetch_$TAG $OUT_DIR/pmc_write_$TAG $OUT_DIR/prof_${TAG}_bench.json $OUT_DIR/srchash_$TAG.txt cfg3 $OUT_DIR/pmc_sq1_$TAG || exit 1
for c in cfg2 cfg4 cfg5; do
  python3 tools/summarize_rocprof.py ${OUT}_$c $OUT_DIR/prof_${TAG}_$c "" "" $OUT_DIR/bench_${TAG}_$c.json || exit 1
done
cp $OUT_DIR/sq_counters_$TAG.txt profiles/${OUT}_sq_counters.txt
# (the bench line of the profile round was printed before this script refreshed the traffic file: run `python bench.py --full` once more on
#  the GPU afterwards and store its line as profiles/OUT_bench_with_cpu.json -- it then carries roofline.traffic)
python3 bench.py --print-src-hash; grep -o '"csrc_sha256": "[0-9a-f]*"' profiles/*_traffic.json
