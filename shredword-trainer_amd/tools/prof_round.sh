# Round profile of bench.py --full (default config; every leg, so a summary holds every kernel) on
# one MI355X: kernel trace + stats, then the two PMC passes (separate runs: FETCH_SIZE,
# WRITE_SIZE), all under $OUT (default profile_out/).  Summaries go to
# profiles/ via tools/pmc_summary.py and tools/prof_summary.py.
#   CFG=c3 bash shredword-trainer_amd/tools/prof_round.sh
set -e
export TMPDIR=/tmp
cd "$GRAFT_REPO_ROOT"
CFG=${CFG:-c3}
OUT=${OUT:-profile_out}
mkdir -p $OUT
timeout -k 10 500 rocprofv3 --kernel-trace --stats -d $OUT/prof_$CFG -o run --output-format csv -- \
  python3 bench.py --full --config $CFG > $OUT/prof_bench_$CFG.json 2> $OUT/prof_bench_$CFG.err
for c in FETCH_SIZE WRITE_SIZE; do
  timeout -k 10 400 rocprofv3 --pmc $c -d $OUT/pmc_${c}_$CFG -o run --output-format csv -- \
    python3 bench.py --full --config $CFG --steps 1 --warmup 0 --pair-count-reps 2 --encode-reps 1 --no-cpu-baseline \
    > $OUT/pmc_${c}_$CFG.json 2> $OUT/pmc_${c}_$CFG.err
done
echo done
