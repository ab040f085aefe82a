# Round close-out on one GPU: the full GPU suite, then the default config's --full
# bench line (C3 plus every other config's line under side_configs).
set -e
O=${OUT:-bench_out}/${ROUND:-r04}
mkdir -p $O
TAG=${ROUND:-r04}_tests bash tools/gpu_tests.sh
timeout -k 10 600 python -u bench.py --full > $O/bench_default.log 2>&1
tail -c 300 $O/bench_default.log
