#!/bin/bash
# usage (GPU box, repo root): tools/neighbours_rate.sh [OUT]     (OUT defaults to profiles/neighbours_rate.txt)
# Wall time of the leave-one-out neighbours of a whole resident reference (skx_ref_neighbours) and, for comparison, of the same rows pushed
# through skx_rank_sketches from the host in the same chunks with top + 1 (tools/neighbours_rate.py).  Two shapes: a 600-genome toy (the
# floor: overheads) and C2's reference (40 000 genomes x s = 10 000).  Each step runs under its own time limit; the second needs the first.
set -o pipefail
OUT=${1:-profiles/neighbours_rate.txt}
mkdir -p "$(dirname "$OUT")" || exit 1
export PYTHONPATH=$PWD${PYTHONPATH:+:$PYTHONPATH}
{
  echo "tools/neighbours_rate.sh -- one job, one MI355X (gfx950) box; wall seconds around calls that end in a synchronised copy to the host."
  echo "line 1 = ReferenceSketch.neighbours (skx_ref_neighbours: query rows rebuilt on the device, self left out inside the selection);"
  echo "line 2 = what existed before it: the same rows from the host through ReferenceSketch.rank_sketches, same chunks, top + 1 rows"
  echo "(self still among them wherever it ranks that high).  Same process, same reference, alternating."
  echo
} > "$OUT"
timeout -k 10 300 python3 tools/neighbours_rate.py toy | tee -a "$OUT" &&
  timeout -k 10 800 python3 tools/neighbours_rate.py c2 | tee -a "$OUT"
