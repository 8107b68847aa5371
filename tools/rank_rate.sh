#!/bin/bash
# usage (GPU box, repo root): tools/rank_rate.sh [OUT]     (OUT defaults to profiles/rank_rate.txt)
# Wall time of ranking 1 024 pooled sketches against a reference, two ways in one process on the same queries (tools/rank_rate.py):
# the counts of skx_common_hashes sorted on the host, and skx_rank_sketches.  Two shapes: a 64-genome toy (the floor: overheads)
# and C2's reference (40 000 genomes x s = 10 000).  Each step runs under its own time limit; the second needs the first.
set -o pipefail
OUT=${1:-profiles/rank_rate.txt}
mkdir -p "$(dirname "$OUT")" || exit 1
export PYTHONPATH=$PWD${PYTHONPATH:+:$PYTHONPATH}
{
  echo "tools/rank_rate.sh -- one job, one MI355X (gfx950) box; wall seconds around calls that end in a synchronised copy to the host."
  echo "old = ReferenceSketch.common_hashes + numpy stable argsort per row; new = ReferenceSketch.rank_sketches; same process, same queries"
  echo "(a reference column with 3 % of its hashes replaced: the pooled sketch of a sample that covers its strain)."
  echo
} > "$OUT"
timeout -k 10 300 python3 tools/rank_rate.py toy | tee -a "$OUT" &&
  timeout -k 10 1100 python3 tools/rank_rate.py c2 | tee -a "$OUT"
