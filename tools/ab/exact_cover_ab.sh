#!/bin/bash
# Headline A/B of the exact-cover plan (profiles/exact_cover_ab.log): bench.py at 2^LOG_N with the tree's library and with a build of the commit before it,
# interleaved.  usage: tools/ab/exact_cover_ab.sh <parent libzl_backend.so> [rounds] [log_n]
set -u -o pipefail
P=$(readlink -f "$1"); ROUNDS=${2:-4}; LOG_N=${3:-24}
R=$(cd "$(dirname "$0")/../.." && pwd)
C=$R/openzl_amd/libzl_backend.so
cd "$R"
for r in $(seq 1 "$ROUNDS"); do
  for side in parent child; do
    lib=$C; [ $side = parent ] && lib=$P
    ZL_BACKEND_LIB=$lib timeout -k 10 300 python bench.py --gpus 1 --steps 20 --warmup 5 --log-n "$LOG_N" 2>/dev/null | python -c '
import json, sys
j = json.loads([l for l in sys.stdin if l.startswith("{")][-1])
print("round %s %-12s ms_per_step %.3f  value %s" % (sys.argv[1], sys.argv[2], j["ms_per_step"], j["value"]))' "$r" "$side" || exit 1
  done
done
