#!/bin/bash
# usage (GPU box, repo root): tools/winners_rate.sh PARENT_TREE [OUT] [PARTS] [RUNS]     (OUT: profiles/winners_rate.txt; PARTS: ab2; RUNS: 3)
# What winner-takes-all breadth costs, this commit against its parent.  PARENT_TREE = the parent commit, built (its bench.py, sketchy_amd/
# with the built libraries and sketchy-hip, oracle/ and include/, in a folder git ignores).  Every GPU step runs under its own time limit
# and the steps are chained; PARTS picks sections, which append to OUT.
#   (a) ms per 98 304-read step at bench.py's default shapes through skx_stream_enqueue_device, coverage enabled, on the parent and on
#       this commit (a); then `python3 bench.py`, RUNS runs each, alternating (2): both medians and the parent's spread.  No pass code
#       changes and a stream that never asks for winners executes nothing new: the difference has to lie inside the parent's spread.
#   (b) the time of skx_stream_winners, skx_stream_winners_rank (top 5) and skx_stream_winners_rows (16 genomes) after the 20 batches,
#       each beside the coverage query of the same shape (printed by the same process as (a)'s figures of this commit); then one more
#       process with the experiments build, which prints the host's part of every query: copy down, sort, copy up.
set -o pipefail
PARENT=${1:?usage: $0 PARENT_TREE [OUT] [PARTS] [RUNS]}
OUT=${2:-profiles/winners_rate.txt}
PARTS=${3:-ab2}
RUNS=${4:-3}
[ -f "$PARENT/sketchy_amd/libsketchy_hip.so" ] && [ -f "$PARENT/bench.py" ] || { echo "$PARENT is not a built tree of the parent commit" >&2; exit 2; }
mkdir -p "$(dirname "$OUT")" || exit 1
PARENT=$(cd "$PARENT" && pwd)
D=$(mktemp -d /dev/shm/skx_win_XXXX) || exit 1
trap 'rm -rf $D' EXIT
[ -s "$OUT" ] || echo "tools/winners_rate.sh -- one MI355X (gfx950) box; parent = the commit before winner-takes-all breadth" > "$OUT"
say() { echo "$@" | tee -a "$OUT"; }

if [[ $PARTS == *a* ]]; then
  say "(a) per-step cost at bench.py's default shapes (config c2), a stream with coverage enabled fed by skx_stream_enqueue_device:"
  timeout -k 10 400 python3 tools/winners_rate.py step $PARENT | tee -a "$OUT" || exit 1
  timeout -k 10 400 python3 tools/winners_rate.py step | tee -a "$OUT" || exit 1
fi
if [[ $PARTS == *b* ]]; then
  SKX_LIB_PATH=$PWD/sketchy_amd/libsketchy_hip_exp.so SKX_WINNERS_TIMES=1 timeout -k 10 400 python3 tools/winners_rate.py step > $D/exp.out 2> $D/exp.err \
    || { tail -5 $D/exp.err >&2; exit 1; }
  say "(b) the host's part of a query (experiments build, one more process; the device is waited for in front of the copy down), the"
  say "    last nine of the process's queries -- winners, winners_rank, winners_rows, three rounds:"
  grep '^winners host:' $D/exp.err | tail -9 | sed 's/^/      /' | tee -a "$OUT"
  grep -A7 '^(b)' $D/exp.out | sed -n '2,7p' | sed 's/^/    (that process) /' | tee -a "$OUT"
fi
if [[ $PARTS == *2* ]]; then
  for i in $(seq $RUNS); do
    for who in $([ $((i % 2)) = 1 ] && echo parent this || echo this parent); do  # (odd pairs: the parent first; even pairs: this commit first)
      if [ $who = parent ]; then
        (cd $PARENT && timeout -k 10 400 python3 bench.py --gpus 1 > $D/parent_$i.json 2> $D/parent_$i.err) || { echo "parent bench run $i failed" >&2; tail -3 $D/parent_$i.err >&2; exit 1; }
      else
        timeout -k 10 400 python3 bench.py --gpus 1 > $D/this_$i.json 2> $D/this_$i.err || { echo "bench run $i failed" >&2; tail -3 $D/this_$i.err >&2; exit 1; }
      fi
    done
    echo "bench pair $i of $RUNS done" >&2
  done
  python3 tools/consensus_rate.py bench $D/parent_*.json > $D/parent.b && python3 tools/consensus_rate.py bench $D/this_*.json > $D/this.b || exit 1
  say "(a) python3 bench.py (config c2; its streams never ask for winners), $RUNS runs each, alternating, the first of a pair alternating too; value = reads/s:"
  say "    parent  median $(cut -d' ' -f1 $D/parent.b)  max - min $(cut -d' ' -f2 $D/parent.b)  runs $(cut -d' ' -f3 $D/parent.b)"
  say "    this    median $(cut -d' ' -f1 $D/this.b)  max - min $(cut -d' ' -f2 $D/this.b)  runs $(cut -d' ' -f3 $D/this.b)"
fi
