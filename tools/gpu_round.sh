# GPU: full parity suite, the full bench line, rocprofv3 kernel-trace stats of the bench command.
# Optional: PMC=1 adds the per-kernel counter passes (tools/gpu_profile_round.sh, isolated-timing build).
# Logs, the bench line and the trace go to $OUT (default: bench_out/).
set -o pipefail
cd $GRAFT_REPO_ROOT
OUT=${OUT:-bench_out}
mkdir -p $OUT
export TMPDIR=/tmp
timeout -k 10 600 python -u -m pytest tests -v --timeout 200 --timeout-method thread -m gpu > $OUT/gpu_tests.log 2>&1 || { tail -40 $OUT/gpu_tests.log; exit 1; }
tail -2 $OUT/gpu_tests.log
timeout -k 10 600 python bench.py --full ${BENCH_ARGS} > $OUT/bench.json 2> $OUT/bench.err || { tail -30 $OUT/bench.err; exit 1; }
echo bench ok
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $OUT/prof -o run --output-format csv -- python bench.py --full --no-cpu-baseline --no-parity --matcher-steps 0 ${BENCH_ARGS} > $OUT/prof.log 2>&1 || { tail -30 $OUT/prof.log; exit 1; }
echo stats ok
if [ -n "$PMC" ]; then PREFIX=${PREFIX:-r03} bash tools/gpu_profile_round.sh; fi
