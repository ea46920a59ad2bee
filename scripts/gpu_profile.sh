#!/usr/bin/env bash
# Benchmark + rocprofv3 passes on a GPU box; outputs under $O (default out/).
#   1. bench.py --full (default config, all legs)      -> $O/bench_<tag>.json
#   2. kernel trace + stats of a 2-step bench          -> $O/prof_<tag>/
#   3. PMC FETCH_SIZE pass, 4. PMC WRITE_SIZE pass      -> $O/pmc_{fetch,write}_<tag>/
# Stops at the first failing step (set -e); every GPU step has its own limit.
set -euo pipefail
TAG=${1:-r01}
cd "$(dirname "$0")/.."
O=${O:-out}
mkdir -p "$O"
export TMPDIR=${TMPDIR:-/tmp}
timeout -k 10 600 python bench.py --full > $O/bench_${TAG}.json 2> $O/bench_${TAG}.err
echo "bench ok" >> $O/steps_${TAG}.txt
timeout -k 10 600 rocprofv3 --kernel-trace --stats -T -d $O/prof_${TAG} -o kt --output-format csv \
    -- python3 bench.py --full --cpu-sample 0 --steps 2 --warmup 1 > $O/bench_prof_${TAG}.json 2> $O/bench_prof_${TAG}.err
echo "prof ok" >> $O/steps_${TAG}.txt
timeout -k 10 600 rocprofv3 --pmc FETCH_SIZE --kernel-trace -T -d $O/pmc_fetch_${TAG} -o pmc --output-format csv \
    -- python3 bench.py --full --cpu-sample 0 --steps 1 --warmup 0 > $O/bench_pmc1_${TAG}.json 2> $O/bench_pmc1_${TAG}.err
echo "pmc fetch ok" >> $O/steps_${TAG}.txt
timeout -k 10 600 rocprofv3 --pmc WRITE_SIZE --kernel-trace -T -d $O/pmc_write_${TAG} -o pmc --output-format csv \
    -- python3 bench.py --full --cpu-sample 0 --steps 1 --warmup 0 > $O/bench_pmc2_${TAG}.json 2> $O/bench_pmc2_${TAG}.err
echo "pmc write ok" >> $O/steps_${TAG}.txt
