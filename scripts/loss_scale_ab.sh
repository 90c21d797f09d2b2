#!/bin/bash
# Static loss-scale mode must cost nothing: this tree against a checkout of its parent commit (both built), alternating on ONE box:
# bench.py (the fp32 headline) and the fp16 learner at 512 and 4096 rows, `pairs` times; then dynamic against static in one process.
#   usage: scripts/loss_scale_ab.sh PARENT_TREE [pairs]
# Every GPU step runs under its own time limit and the steps are chained: the first failure ends the script.
set -o pipefail
here=$(cd "$(dirname "$0")/.." && pwd)
parent=$(cd "$1" && pwd) || exit 2
pairs=${2:-3}
bench() { (cd "$1" && timeout -k 10 240 python bench.py --gpus 1 --steps 3000 --warmup 300 --no-cpu-baseline --no-env --no-subrecords --no-live-pmc 2>/dev/null | grep '^{' | tail -1 |
           python -c 'import json,sys; d=json.loads(sys.stdin.read()); print("bench", sys.argv[1], d["value"], d.get("unit", ""), d["ms_per_step"], "ms/step")' "$2"); }
fp16() { echo -n "fp16 $2 "; timeout -k 10 240 python "$here/scripts/loss_scale_ab.py" --root "$1" --modes static --reps 1 512 4096 | tr '\n' ' '; echo; }
for p in $(seq "$pairs"); do
  bench "$parent" parent && bench "$here" new && fp16 "$parent" parent && fp16 "$here" new || exit 1
done
timeout -k 10 300 python "$here/scripts/loss_scale_ab.py" --modes static,dynamic 512 4096
