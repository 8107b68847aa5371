#!/bin/bash
# usage (GPU box, repo root): tools/call_rate.sh PARENT_TREE [OUT] [PARTS]     (OUT: profiles/call_rate.txt; PARTS: abc)
# What the species call costs and buys, this commit against its parent.  PARENT_TREE = the parent commit, built (from a `git worktree`
# beside this one: its bench.py, sketchy_amd/ with the built libraries and sketchy-hip, oracle/ and include/, in a folder git ignores).
# Every GPU step runs under its own time limit and the steps are chained; PARTS picks sections, which append to OUT.
#   (a) device time per 98 304-read step of a five-species stream (bench.py --config c4 shapes, skx_stream_enqueue_device): a stream
#       that never binds on the parent and on this commit, and one that binds the call and its event list to every batch.
#   (b) `python3 bench.py` and `python3 bench.py --config c4`, three runs each, alternating: both medians and the parent's spread.
#       A stream that never binds executes no new code: the difference has to lie inside the parent's own run-to-run spread.
#   (c) `sketchy-hip predict -s` with five -r on one FASTQ (-t 1, -c -t 5, -t 5 --changes) against the five single-reference runs one
#       after the other: wall time and reads/s of each, and whether the multi-reference text is the called species' own run.
set -o pipefail
PARENT=${1:?usage: $0 PARENT_TREE [OUT] [PARTS]}
OUT=${2:-profiles/call_rate.txt}
PARTS=${3:-abc}
[ -x "$PARENT/sketchy_amd/sketchy-hip" ] && [ -f "$PARENT/bench.py" ] || { echo "$PARENT is not a built tree of the parent commit" >&2; exit 2; }
mkdir -p "$(dirname "$OUT")" || exit 1
HERE=$PWD
PARENT=$(cd "$PARENT" && pwd)
D=$(mktemp -d /dev/shm/skx_call_XXXX) || exit 1
trap 'rm -rf $D' EXIT
[ -s "$OUT" ] || echo "tools/call_rate.sh -- one MI355X (gfx950) box; parent = the commit before the species call" > "$OUT"
say() { echo "$@" | tee -a "$OUT"; }
BIN=$HERE/sketchy_amd/sketchy-hip
N_READS=262144

if [[ $PARTS == *a* ]]; then
  say "(a) device time per step, five species resident (bench.py --config c4 shapes), streams fed by skx_stream_enqueue_device:"
  timeout -k 10 500 python3 tools/call_rate.py step $PARENT | tee -a "$OUT" || exit 1
  timeout -k 10 500 python3 tools/call_rate.py step | tee -a "$OUT" || exit 1
fi
if [[ $PARTS == *b* ]]; then
  for cfg in c2 c4; do
    for i in 1 2 3; do
      (cd $PARENT && timeout -k 10 400 python3 bench.py --config $cfg > $D/parent_${cfg}_$i.json 2> $D/parent_$i.err) || { echo "parent bench $cfg run $i failed" >&2; tail -3 $D/parent_$i.err >&2; exit 1; }
      timeout -k 10 400 python3 bench.py --config $cfg > $D/this_${cfg}_$i.json 2> $D/this_$i.err || { echo "bench $cfg run $i failed" >&2; tail -3 $D/this_$i.err >&2; exit 1; }
      echo "bench $cfg pair $i of 3 done" >&2
    done
    python3 tools/consensus_rate.py bench $D/parent_${cfg}_[123].json > $D/parent.b && python3 tools/consensus_rate.py bench $D/this_${cfg}_[123].json > $D/this.b || exit 1
    say "(b) python3 bench.py --config $cfg (streams that never bind), three runs each, alternating; value = reads/s:"
    say "    parent  median $(cut -d' ' -f1 $D/parent.b)  max - min $(cut -d' ' -f2 $D/parent.b)  runs $(cut -d' ' -f3 $D/parent.b)"
    say "    this    median $(cut -d' ' -f1 $D/this.b)  max - min $(cut -d' ' -f2 $D/this.b)  runs $(cut -d' ' -f3 $D/this.b)"
  done
fi
if [[ $PARTS == *c* ]]; then
  timeout -k 10 600 python3 tools/call_rate.py inputs $D || exit 1
  REFS=""; TABS=""
  for i in 0 1 2 3 4; do REFS="$REFS $D/sp$i.msh"; TABS="$TABS $D/sp$i.tsv"; done
  say "(c) sketchy-hip predict -s, $N_READS reads x 1.5 kb (a quarter from species 0's strain, then species 3's), five references of"
  say "    8 000 / 8 000 / 6 000 / 5 000 / 3 000 sketches (s = 1 000) with tables of 1 .. 5 columns; wall time of the whole command, three runs:"
  timed() {  # label, output file, command...: three runs, wall seconds of each
    local label=$1 out=$2; shift 2
    : > $D/$label.t
    for rep in 1 2 3; do
      local t0=$(date +%s%N)
      timeout -k 10 300 "$@" > $out 2> $D/$label.err || { echo "$label: run failed" >&2; tail -3 $D/$label.err >&2; return 1; }
      echo "$(( $(date +%s%N) - t0 )) $N_READS" >> $D/$label.t
    done
    python3 tools/call_rate.py spread $D/$label.t "$label" | tee -a "$OUT"
  }
  five_single() {  # prefix of the outputs, args...: the five single-reference runs one after the other
    local pre=$1; shift
    for i in 0 1 2 3 4; do timeout -k 10 300 $BIN predict -s -r $D/sp$i.msh -g $D/sp$i.tsv -i $D/reads.fq "$@" > $D/$pre$i.out || return 1; done
  }
  for leg in "t1:-t 1:1:rows" "c_t5:-c -t 5:5:consensus"; do
    IFS=: read name args top mode <<< "$leg"
    : > $D/single_$name.t
    for rep in 1 2 3; do
      t0=$(date +%s%N)
      five_single single $args || { echo "single-reference runs failed" >&2; exit 1; }
      echo "$(( $(date +%s%N) - t0 )) $N_READS" >> $D/single_$name.t
    done
    python3 tools/call_rate.py spread $D/single_$name.t "five_single_runs_$name" | tee -a "$OUT"
    timed "five_references_$name" $D/multi.out $BIN predict -s -r $REFS -g $TABS -i $D/reads.fq $args || exit 1
    [ $mode = consensus ] && { five_single lead -t 5 || exit 1; }
    say "    $name: $(python3 tools/call_rate.py agree $D $top $mode)"
  done
  timed "five_references_t5" $D/plain.out $BIN predict -s -r $REFS -g $TABS -i $D/reads.fq -t 5 || exit 1
  timed "five_references_t5_changes" $D/changes.out $BIN predict -s -r $REFS -g $TABS -i $D/reads.fq -t 5 --changes || exit 1
  say "    t5: $(python3 tools/call_rate.py filter $D/plain.out $D/changes.out 5)"
fi
