#!/bin/bash
# Per-step-kind kernel breakdown of the graph-replayed timed region (run on the GPU box).
#   bash tools/profile_kinds.sh [kinds, default "1 2 3"]      outputs under $G2S_PROFILE_OUT/kinds/
set -e
export TMPDIR=/tmp G2S_BENCH_MARK=1
R=$(cd "$(dirname "$0")/.." && pwd)
O=${G2S_PROFILE_OUT:-$R/profile_out}/kinds
mkdir -p $O
cd /tmp
for K in ${1:-1 2 3}; do
  rocprofv3 --kernel-trace -d /tmp/prof_k$K -o k$K --output-format csv -- python3 $R/bench.py --full --only $K --steps 20 --warmup 10 --no-cpu-baseline > $O/bench_k$K.json 2> $O/bench_k$K.err
  F=$(find /tmp/prof_k$K -name "*kernel_trace.csv" | head -1)
  python3 $R/tools/window_trace.py $F 20 250 > $O/step$K.txt
  echo "step $K done"
done
