#!/bin/bash
# usage (on the GPU box): [OUT_DIR=results] bash tools/profile_round.sh TAG
# One round's evidence, everything under $OUT_DIR/ (tools/summarize_rocprof.py then writes the tracked files under profiles/):
#   1. rocprofv3 --kernel-trace --stats of bench.py (cfg3 = the bench workload): per-kernel time
#   2. separate --pmc passes (the pool refuses --pmc together with other trace domains): FETCH_SIZE, WRITE_SIZE (HBM-side traffic),
#      and two SQ passes (instruction mix, VALU / LDS activity, waits, bank conflicts)
#   3. the bench line of `bench.py --full` (roofline, CPU baseline)
#   4. kernel stats + bench lines of the other single-GPU configurations (cfg2, cfg4, cfg5)
TAG=${1:-r02}
OUT_DIR=${OUT_DIR:-results}
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}" || exit 1
export TMPDIR=/tmp
mkdir -p "$OUT_DIR"
B="python3 bench.py --full --steps 50 --warmup 5 --no-cpu-baseline"
S="python3 bench.py --steps 3 --warmup 1 --prime 4 --no-cpu-baseline --no-profile-events"
P1="SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_INSTS_VMEM_RD SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_ACTIVE_INST_VALU SQ_WAIT_INST_ANY"
P2="SQ_ACTIVE_INST_LDS SQ_INST_LEVEL_LDS SQ_INST_LEVEL_VMEM SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_WAIT_INST_LDS SQ_ACTIVE_INST_VMEM SQ_ACTIVE_INST_SCA"
rm -rf $OUT_DIR/prof_$TAG $OUT_DIR/pmc_fetch_$TAG $OUT_DIR/pmc_write_$TAG $OUT_DIR/pmc_sq1_$TAG $OUT_DIR/pmc_sq2_$TAG
python3 bench.py --print-src-hash > $OUT_DIR/srchash_$TAG.txt &&
rocprofv3 --kernel-trace --stats -d $OUT_DIR/prof_$TAG -o run --output-format csv -- $B > $OUT_DIR/prof_${TAG}_bench.json 2> $OUT_DIR/prof_$TAG.err &&
rocprofv3 --kernel-trace --pmc FETCH_SIZE -d $OUT_DIR/pmc_fetch_$TAG -o run --output-format csv -- $S > /dev/null 2> $OUT_DIR/pmc_fetch_$TAG.err &&
rocprofv3 --kernel-trace --pmc WRITE_SIZE -d $OUT_DIR/pmc_write_$TAG -o run --output-format csv -- $S > /dev/null 2> $OUT_DIR/pmc_write_$TAG.err &&
rocprofv3 --kernel-trace --pmc $P1 -d $OUT_DIR/pmc_sq1_$TAG -o run --output-format csv -- $S > /dev/null 2> $OUT_DIR/pmc_sq1_$TAG.err &&
rocprofv3 --kernel-trace --pmc $P2 -d $OUT_DIR/pmc_sq2_$TAG -o run --output-format csv -- $S > /dev/null 2> $OUT_DIR/pmc_sq2_$TAG.err &&
python3 tools/pmc_table.py $OUT_DIR/pmc_sq1_$TAG $OUT_DIR/pmc_sq2_$TAG > $OUT_DIR/sq_counters_$TAG.txt &&
echo "profiles of cfg3 done" &&
python3 bench.py --full > $OUT_DIR/bench_$TAG.json 2> $OUT_DIR/bench_$TAG.err &&
tail -1 $OUT_DIR/bench_$TAG.json | cut -c1-300 &&
for c in cfg2 cfg4 cfg5; do
  rm -rf $OUT_DIR/prof_${TAG}_$c
  rocprofv3 --kernel-trace --stats -d $OUT_DIR/prof_${TAG}_$c -o run --output-format csv -- python3 bench.py --full --config $c --steps 50 --warmup 5 --no-cpu-baseline > $OUT_DIR/bench_${TAG}_$c.json 2> $OUT_DIR/prof_${TAG}_$c.err || exit 1
  echo "$c done"
done
