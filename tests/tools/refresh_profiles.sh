#!/bin/bash
# Regenerates the measurements kept under profiles/ (run on the GPU box from the repo root; outputs go to the folder OUT
# given as the only argument, copy the ones to keep into profiles/):
#   tests/tools/refresh_profiles.sh OUT
#   1. bench.py --full (roofline pass, CPU baseline)   -> OUT/bench.json
#   2. rocprofv3 --kernel-trace --stats of bench.py    -> OUT/kernel_stats.csv, kernel_summary.txt
#   3. the same with the eager single-stream step      -> OUT/kernel_stats_eager_serial.csv, kernel_summary_eager_serial.txt
#   4. per-layer replay of every conv op               -> OUT/layers_c2.txt
#   5. (separate call) PMC passes: see tests/tools/pmc_hbm.py
set -e
R=${GRAFT_REPO_ROOT:-$(pwd)}
OUT=$(realpath -m "${1:?usage: tests/tools/refresh_profiles.sh OUT}")
mkdir -p "$OUT"
python3 $R/bench.py --full > "$OUT"/bench.json 2> "$OUT"/bench.err
tail -c 2500 "$OUT"/bench.json
cd /tmp && export TMPDIR=/tmp
rm -rf /tmp/prof_stats
rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/prof_stats -o r -- python3 $R/bench.py --steps 10 --warmup 3 --no-cpu-baseline --no-roofline > /tmp/prof_stats.log 2>&1
cp $(find /tmp/prof_stats -name "*kernel_stats.csv" | head -1) "$OUT"/kernel_stats.csv
python3 $R/tests/tools/trace_steps.py /tmp/prof_stats 6 60 > "$OUT"/kernel_summary.txt
head -12 "$OUT"/kernel_summary.txt
# the regime bench.py's roofline pass times kernels in: eager, one stream (kernel durations without co-runners)
rm -rf /tmp/prof_serial
MOPOE_GRAPH=0 MOPOE_NET_STREAMS=0 MOPOE_WGRAD_STREAM=0 rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/prof_serial -o r -- python3 $R/bench.py --steps 10 --warmup 3 --no-cpu-baseline --no-roofline > /tmp/prof_serial.log 2>&1
cp $(find /tmp/prof_serial -name "*kernel_stats.csv" | head -1) "$OUT"/kernel_stats_eager_serial.csv
python3 $R/tests/tools/trace_steps.py /tmp/prof_serial 6 60 > "$OUT"/kernel_summary_eager_serial.txt
head -8 "$OUT"/kernel_summary_eager_serial.txt
cd $R && python3 tests/tools/layer_replay.py c2 > "$OUT"/layers_c2.txt 2>&1
head -3 "$OUT"/layers_c2.txt
