# The GPU test suite (every -m gpu test, product libraries), then the bench line with every leg (--full, into $OUT).
# Each step time-limited; the first failure ends the script.
cd $GRAFT_REPO_ROOT
mkdir -p gpurun_out
timeout -k 10 900 python -u -m pytest tests/ -m gpu -v -s --timeout 300 --timeout-method thread -rA \
    > gpurun_out/gpu_tests.log 2>&1
rc=$?; echo "pytest rc=$rc"; grep -E "^(FAILED|ERROR)|passed|failed|^E " gpurun_out/gpu_tests.log | head -20
[ $rc -eq 0 ] || exit $rc
OUT=${OUT:-bench_out}; mkdir -p $OUT
timeout -k 10 900 python -u bench.py --full > $OUT/bench_default.log 2>&1 || { echo "bench failed"; tail -20 $OUT/bench_default.log; exit 1; }
python tools/bench_summary.py $OUT/bench_default.log
