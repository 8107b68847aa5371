#!/bin/bash
# usage (GPU box, repo root): tools/consensus_rate.sh PARENT_TREE [OUT] [PARTS]     (OUT: profiles/consensus_rate.txt; PARTS: abc)
# What consensus calls on the device cost and buy, this commit against its parent.  PARENT_TREE = the parent commit, built: a
# `git worktree add ../parent HEAD~1` of it, `python3 -m sketchy_amd.build` there, and its bench.py, sketchy_amd/ (with the built
# libraries and sketchy-hip), oracle/ and include/ copied to a folder git ignores (out/parent).  One job; every GPU step runs under its
# own time limit and the steps are chained.  PARTS picks sections (a job of at most 20 minutes: "ac", then "b"); sections append to OUT.
#   (a) `sketchy-hip predict -s -c -t 5 --timing`, parent's binary and this one, on the same FASTQ of 1 081 344 reads x 1.5 kb against
#       a 40 000 x 10 000 reference with a genotype table of 16 columns: one warm-up, median reads_per_s of five, outputs compared
#       with cmp.  This commit must not be slower.
#   (b) plain `python3 bench.py`, three times each, alternating: this commit's median `value` must be at least the parent's median
#       minus the parent's own max - min.  (Streams that never bind a consensus output.)
#   (c) for information: ms per step of 20 enqueued C2 batches, top = 5, with and without 16 columns bound (tools/consensus_rate.py step).
set -o pipefail
PARENT=${1:?usage: $0 PARENT_TREE [OUT] [PARTS]}
OUT=${2:-profiles/consensus_rate.txt}
PARTS=${3:-abc}
[ -x "$PARENT/sketchy_amd/sketchy-hip" ] && [ -f "$PARENT/bench.py" ] || { echo "$PARENT is not a built tree of the parent commit" >&2; exit 2; }
mkdir -p "$(dirname "$OUT")" || exit 1
HERE=$PWD
PARENT=$(cd "$PARENT" && pwd)
D=$(mktemp -d /dev/shm/skx_cons_XXXX) || exit 1
trap 'rm -rf $D' EXIT
[ -s "$OUT" ] || echo "tools/consensus_rate.sh -- one MI355X (gfx950) box; parent = the commit before consensus calls moved to the device" > "$OUT"
say() { echo "$@" | tee -a "$OUT"; }

cli_runs() {  # label, binary: one warm-up + five runs of predict -s -c -t 5 --timing; stdout of the last run is kept
  local label=$1 bin=$2
  : > $D/$label.err
  for rep in 0 1 2 3 4 5; do
    timeout -k 10 300 $bin predict -r $D/ref.msh -g $D/geno.tsv -i $D/reads.fq -s -c -t 5 --timing > $D/$label.out 2>> $D/$label.err || { echo "$label: run failed" >&2; tail -3 $D/$label.err >&2; return 1; }
  done
  python3 tools/consensus_rate.py median $D/$label.err > $D/$label.med || return 1
  say "    $label  median reads_per_s $(cut -d' ' -f1 $D/$label.med)   all six runs (the first warms up): $(cut -d' ' -f2 $D/$label.med)"
}

if [[ $PARTS == *a* || $PARTS == *c* ]]; then
  timeout -k 10 900 python3 tools/consensus_rate.py inputs $D || exit 1
  if [[ $PARTS == *c* ]]; then
    timeout -k 10 600 python3 tools/consensus_rate.py step $D | tee -a "$OUT" || exit 1
  fi
fi
if [[ $PARTS == *a* ]]; then
  timeout -k 10 600 python3 tools/consensus_rate.py msh $D || exit 1
  say "(a) sketchy-hip predict -s -c -t 5 --timing, 1 081 344 reads x 1.5 kb, reference 40 000 x 10 000, 16 genotype columns:"
  cli_runs parent $PARENT/sketchy_amd/sketchy-hip && cli_runs this $HERE/sketchy_amd/sketchy-hip || exit 1
  cmp $D/parent.out $D/this.out && say "    outputs identical ($(wc -l < $D/this.out) lines, $(wc -c < $D/this.out) bytes)" || { say "    outputs DIFFER"; exit 1; }
  python3 - $D/parent.med $D/this.med <<'PY' | tee -a "$OUT" || exit 1
import sys
p, t = (float(open(f).read().split()[0]) for f in sys.argv[1:3])
print(f"    this / parent = {t / p:.3f}   criterion (this >= parent): {'met' if t >= p else 'NOT met'}")
sys.exit(0 if t >= p else 1)
PY
fi
rm -rf $D/*
if [[ $PARTS == *b* ]]; then
  for i in 1 2 3; do
    (cd $PARENT && timeout -k 10 400 python3 bench.py > $D/parent_$i.json 2> $D/parent_$i.err) || { echo "parent bench run $i failed" >&2; tail -3 $D/parent_$i.err >&2; exit 1; }
    timeout -k 10 400 python3 bench.py > $D/this_$i.json 2> $D/this_$i.err || { echo "bench run $i failed" >&2; tail -3 $D/this_$i.err >&2; exit 1; }
  done
  python3 tools/consensus_rate.py bench $D/parent_[123].json > $D/parent.b && python3 tools/consensus_rate.py bench $D/this_[123].json > $D/this.b || exit 1
  say "(b) plain python3 bench.py (streams that never bind), three runs each, alternating; value = reads/s:"
  say "    parent  median $(cut -d' ' -f1 $D/parent.b)  max - min $(cut -d' ' -f2 $D/parent.b)  runs $(cut -d' ' -f3 $D/parent.b)"
  say "    this    median $(cut -d' ' -f1 $D/this.b)  max - min $(cut -d' ' -f2 $D/this.b)  runs $(cut -d' ' -f3 $D/this.b)"
  python3 - $D/parent.b $D/this.b <<'PY' | tee -a "$OUT" || exit 1
import sys
(pm, ps), (tm, _) = ([float(x) for x in open(f).read().split()[:2]] for f in sys.argv[1:3])
ok = tm >= pm - ps
print(f"    this / parent = {tm / pm:.3f}   criterion (this >= parent median - parent spread = {pm - ps:.1f}): {'met' if ok else 'NOT met'}")
sys.exit(0 if ok else 1)
PY
fi
