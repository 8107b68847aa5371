#!/bin/bash
# usage (GPU box, repo root): tools/changes_rate.sh PARENT_TREE [OUT] [PARTS]     (OUT: profiles/changes_rate.txt; PARTS: abc)
# What the per-batch change log costs and buys, this commit against its parent.  PARENT_TREE = the parent commit, built, as for
# tools/consensus_rate.sh (its bench.py, sketchy_amd/ with the built libraries and sketchy-hip, oracle/ and include/ in a folder git
# ignores).  Every GPU step runs under its own time limit and the steps are chained; PARTS picks sections, which append to OUT.
#   (a) `sketchy-hip predict -s --timing` with -t 1, -t 5, -t 16 and -c -t 5 on the million-read C2 set-up of tools/consensus_rate.sh:
#       the parent's binary, this one, and this one with --changes; three runs per leg; lines printed, and whether --changes printed
#       exactly the filtered text of the plain run.
#   (b) device time per 98 304-read step: a stream that never binds on the parent and on this commit, and streams that bind an event
#       list to every batch (index rows / codes).  "Nothing for a stream that never binds" stands if this - parent lies inside the
#       spread of the parent's three repetitions.
#   (c) plain `python3 bench.py`, three times each, alternating: both medians and the parent's spread.
set -o pipefail
PARENT=${1:?usage: $0 PARENT_TREE [OUT] [PARTS]}
OUT=${2:-profiles/changes_rate.txt}
PARTS=${3:-abc}
[ -x "$PARENT/sketchy_amd/sketchy-hip" ] && [ -f "$PARENT/bench.py" ] || { echo "$PARENT is not a built tree of the parent commit" >&2; exit 2; }
mkdir -p "$(dirname "$OUT")" || exit 1
HERE=$PWD
PARENT=$(cd "$PARENT" && pwd)
D=$(mktemp -d /dev/shm/skx_chg_XXXX) || exit 1
trap 'rm -rf $D' EXIT
[ -s "$OUT" ] || echo "tools/changes_rate.sh -- one MI355X (gfx950) box; parent = the commit before the change log" > "$OUT"
say() { echo "$@" | tee -a "$OUT"; }

cli_runs() {  # label, binary, args...: three runs of predict -s --timing; stdout of the last run is kept as $D/$label.out
  local label=$1 bin=$2; shift 2
  : > $D/$label.err
  for rep in 1 2 3; do
    timeout -k 10 300 $bin predict -r $D/ref.msh -g $D/geno.tsv -i $D/reads.fq -s --timing "$@" > $D/$label.out 2>> $D/$label.err || { echo "$label: run failed" >&2; tail -3 $D/$label.err >&2; return 1; }
  done
  python3 tools/changes_rate.py spread $D/$label.err "$label" | tee -a "$OUT"
}

if [[ $PARTS == *a* || $PARTS == *b* ]]; then
  timeout -k 10 900 python3 tools/consensus_rate.py inputs $D || exit 1
fi
if [[ $PARTS == *b* ]]; then
  say "(b) device time per step, streams fed by skx_stream_enqueue_device (event lists of 4 096 entries):"
  timeout -k 10 600 python3 tools/changes_rate.py step $D $PARENT | tee -a "$OUT" || exit 1
  timeout -k 10 600 python3 tools/changes_rate.py step $D | tee -a "$OUT" || exit 1
fi
if [[ $PARTS == *a* ]]; then
  timeout -k 10 600 python3 tools/consensus_rate.py msh $D || exit 1
  say "(a) sketchy-hip predict -s --timing, 1 081 344 reads x 1.5 kb from the truth strain, reference 40 000 x 10 000, 16 genotype columns:"
  for leg in "t1:-t 1" "t5:-t 5" "t16:-t 16" "c_t5:-c -t 5"; do
    name=${leg%%:*}; args=${leg#*:}; top=$(echo $args | awk '{print $NF}'); [[ $args == *-c* ]] && top=1
    cli_runs "parent_$name" $PARENT/sketchy_amd/sketchy-hip $args || exit 1
    cli_runs "this_$name" $HERE/sketchy_amd/sketchy-hip $args || exit 1
    cli_runs "this_${name}_changes" $HERE/sketchy_amd/sketchy-hip $args --changes || exit 1
    cmp -s $D/parent_$name.out $D/this_$name.out && same="identical to the parent's" || same="DIFFERENT from the parent's"
    say "    $name: plain output $same; $(python3 tools/changes_rate.py filter $D/this_$name.out $D/this_${name}_changes.out $top)"
    rm -f $D/*_$name.out $D/*_${name}_changes.out
  done
fi
rm -rf $D/*
if [[ $PARTS == *c* ]]; then
  for i in 1 2 3; do
    (cd $PARENT && timeout -k 10 400 python3 bench.py > $D/parent_$i.json 2> $D/parent_$i.err) || { echo "parent bench run $i failed" >&2; tail -3 $D/parent_$i.err >&2; exit 1; }
    timeout -k 10 400 python3 bench.py > $D/this_$i.json 2> $D/this_$i.err || { echo "bench run $i failed" >&2; tail -3 $D/this_$i.err >&2; exit 1; }
    echo "bench pair $i of 3 done" >&2
  done
  python3 tools/consensus_rate.py bench $D/parent_[123].json > $D/parent.b && python3 tools/consensus_rate.py bench $D/this_[123].json > $D/this.b || exit 1
  say "(c) plain python3 bench.py (streams that never bind), three runs each, alternating; value = reads/s:"
  say "    parent  median $(cut -d' ' -f1 $D/parent.b)  max - min $(cut -d' ' -f2 $D/parent.b)  runs $(cut -d' ' -f3 $D/parent.b)"
  say "    this    median $(cut -d' ' -f1 $D/this.b)  max - min $(cut -d' ' -f2 $D/this.b)  runs $(cut -d' ' -f3 $D/this.b)"
fi
