#!/bin/bash
# usage (GPU box, repo root): tools/composition_rate.sh PARENT_TREE [OUT] [PARTS] [RUNS]   (OUT: profiles/composition_rate.txt; PARTS: a4b; RUNS: 3)
# What the composition of a stream costs, this commit against its parent.  PARENT_TREE = the parent commit, built (its bench.py,
# sketchy_amd/ with the built libraries, oracle/ and include/, in a folder git ignores).  Every GPU step runs under its own time limit
# and the steps are chained; PARTS picks sections, which append to OUT:
#   a  (a) ms per 98 304-read step at bench.py's default shapes (config c2) through skx_stream_enqueue_device: a stream that never enables
#      anything and one with depth, on the parent and on this commit, and one with composition; (c) the first enable (one species: no table)
#   4  (b) the same at config c4's shapes, five species resident; (c) the first enable there builds the species masks
#   b  (d) `python3 bench.py`, RUNS runs each, alternating: both medians and the parent's spread
# A stream that never enables composition executes no new code: the difference has to lie inside the parent's own run-to-run spread.
# The enabled cost is reported beside depth's, not bounded.
set -o pipefail
PARENT=${1:?usage: $0 PARENT_TREE [OUT] [PARTS] [RUNS]}
OUT=${2:-profiles/composition_rate.txt}
PARTS=${3:-a4b}
RUNS=${4:-3}
[ -f "$PARENT/sketchy_amd/libsketchy_hip.so" ] && [ -f "$PARENT/bench.py" ] || { echo "$PARENT is not a built tree of the parent commit" >&2; exit 2; }
mkdir -p "$(dirname "$OUT")" || exit 1
PARENT=$(cd "$PARENT" && pwd)
D=$(mktemp -d /dev/shm/skx_comp_XXXX) || exit 1
trap 'rm -rf $D' EXIT
[ -s "$OUT" ] || echo "tools/composition_rate.sh -- one MI355X (gfx950) box; parent = the commit before the composition of a stream" > "$OUT"
say() { echo "$@" | tee -a "$OUT"; }

if [[ $PARTS == *a* ]]; then
  say "(a), (c) per-step cost at bench.py's default shapes (config c2), streams fed by skx_stream_enqueue_device:"
  timeout -k 10 400 python3 tools/composition_rate.py step c2 $PARENT | tee -a "$OUT" || exit 1
  timeout -k 10 400 python3 tools/composition_rate.py step c2 | tee -a "$OUT" || exit 1
fi
if [[ $PARTS == *4* ]]; then
  say "(b), (c) the same at config c4's shapes (five species resident):"
  timeout -k 10 500 python3 tools/composition_rate.py step c4 $PARENT | tee -a "$OUT" || exit 1
  timeout -k 10 500 python3 tools/composition_rate.py step c4 | tee -a "$OUT" || exit 1
fi
if [[ $PARTS == *b* ]]; then
  for i in $(seq $RUNS); do
    (cd $PARENT && timeout -k 10 400 python3 bench.py --config c2 > $D/parent_$i.json 2> $D/parent_$i.err) || { echo "parent bench run $i failed" >&2; tail -3 $D/parent_$i.err >&2; exit 1; }
    timeout -k 10 400 python3 bench.py --config c2 > $D/this_$i.json 2> $D/this_$i.err || { echo "bench run $i failed" >&2; tail -3 $D/this_$i.err >&2; exit 1; }
    echo "bench c2 pair $i of $RUNS done" >&2
  done
  python3 tools/consensus_rate.py bench $D/parent_*.json > $D/parent.b && python3 tools/consensus_rate.py bench $D/this_*.json > $D/this.b || exit 1
  say "(d) python3 bench.py --config c2 (streams that never enable composition), $RUNS runs each, alternating; value = reads/s:"
  say "    parent  median $(cut -d' ' -f1 $D/parent.b)  max - min $(cut -d' ' -f2 $D/parent.b)  runs $(cut -d' ' -f3 $D/parent.b)"
  say "    this    median $(cut -d' ' -f1 $D/this.b)  max - min $(cut -d' ' -f2 $D/this.b)  runs $(cut -d' ' -f3 $D/this.b)"
fi
