#!/bin/bash
# fp16 acting of the fp16 learner.  (1) The default (fp32 acting) must cost what it cost: this tree against a checkout of its parent
# commit (both built), alternating processes on ONE box, `pairs` times, fp32 acting only.  (2) fp32 against fp16 acting, alternating
# inside one process (scripts/act_precision_ab.py), `pairs` pairs per point; its table goes to OUT (default profiles/fp16_acting_ab.md
# is written by hand from it, with the context of the run).
#   usage: scripts/act_precision_ab.sh PARENT_TREE [pairs] [OUT_DIR]
# Every GPU step runs under its own time limit and the steps are chained: the first failure ends the script.
set -o pipefail
here=$(cd "$(dirname "$0")/.." && pwd)
parent=$(cd "$1" && pwd) || exit 2
pairs=${2:-5}
out=${3:-$here}
one() { echo "== $2 (fp32 acting)"; timeout -k 10 300 python "$here/scripts/act_precision_ab.py" --root "$1" --modes fp32 --pairs 3; }
for p in $(seq "$pairs"); do
  one "$parent" parent && one "$here" new || exit 1
done > "$out/act_precision_parent_vs_new.txt"
timeout -k 10 600 python "$here/scripts/act_precision_ab.py" --modes fp32,fp16 --pairs "$pairs" --out "$out/act_precision_ab_table.md"
