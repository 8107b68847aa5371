#!/bin/bash
# usage (GPU box, repo root): tools/pool_rate.sh LABEL=BIN [LABEL=BIN ...]
# Wall time of the two subcommands that pool several records into one sketch, for each given `sketchy-hip` binary (each next to the
# libsketchy_hip.so it was linked against) on the same inputs, in the same job:
#   (a) `sketch`  of 64 genome files of 50 contigs x 50 kb at s = 10 000
#   (b) offline `predict` of 98 304 reads x 1.5 kb against a 512-genome reference at s = 10 000 (one batch: -b 98304)
# One warm-up run, then the median of five.  Inputs come from sketchy_amd.synth; the outputs of all binaries are compared byte for byte.
# A second binary = the parent commit's, built from a `git worktree` outside the tree and copied next to this one (out/ is ignored).
set -o pipefail
[ $# -ge 1 ] || { echo "usage: $0 LABEL=BIN [LABEL=BIN ...]" >&2; exit 2; }
D=$(mktemp -d /dev/shm/skx_pool_XXXX) || exit 1
trap 'rm -rf $D' EXIT
python3 - $D <<'PY' || exit 1
import sys
sys.path.insert(0, ".")
import numpy as np
from sketchy_amd import synth
from sketchy_amd.mshio import write_msh
d = sys.argv[1]
rng = np.random.default_rng(1)
for g in range(64):
    with open(f"{d}/genome{g:02d}.fa", "wb") as f:
        for c in range(50):
            f.write(b">contig%d\n" % c + synth.random_genome(50000, rng).tobytes() + b"\n")
ref = synth.make_reference(512, 10000, rng_seed=3, device="numpy")
names = [f"g{i:03d}" for i in range(512)]
write_msh(d + "/ref.msh", names, ref["ref"], kmer=16, seed=0, lengths=[len(ref["genome"])] * 512)
open(d + "/geno.tsv", "w").write("id\tmlst\n" + "".join(f"{n}\tST{i % 9}\n" for i, n in enumerate(names)))
L = 1500
with open(d + "/reads.fq", "wb") as f:
    for part in range(6):
        b, o = synth.make_reads(ref["genome"], 16384, L, rng_seed=10 + part)
        rec = np.empty((16384, 8 + L + 3 + L + 1), np.uint8)
        rec[:, :8] = np.frombuffer(b"@read/1\n", np.uint8); rec[:, 8:8 + L] = b.reshape(16384, L)
        rec[:, 8 + L:8 + L + 3] = np.frombuffer(b"\n+\n", np.uint8); rec[:, 8 + L + 3:8 + 2 * L + 3] = ord("I"); rec[:, -1] = 10
        rec.tofile(f)
PY
timed() {  # label, what, output file, command ...: one warm-up, median of 5 wall times
  local label=$1 what=$2 out=$3; shift 3
  local ts=()
  for rep in 0 1 2 3 4 5; do
    local t0=$(date +%s.%N)
    timeout -k 10 300 "$@" > $out.stdout || { echo "$label $what: run failed" >&2; return 1; }
    local t1=$(date +%s.%N)
    [ $rep -gt 0 ] && ts+=($(awk "BEGIN{print $t1 - $t0}"))
  done
  local med=$(printf '%s\n' "${ts[@]}" | sort -g | sed -n 3p)
  printf '%s %s median_wall_s=%.3f runs_s=%s\n' "$label" "$what" "$med" "$(printf '%.3f,' "${ts[@]}")"
}
first=""
for arg in "$@"; do
  label=${arg%%=*}; bin=${arg#*=}
  timed $label "(a) sketch 64 files x 50 contigs x 50 kb, s=10000" $D/a_$label $bin sketch -i $D/genome*.fa -o $D/a_$label.msh -s 10000 || exit 1
  timed $label "(b) offline predict 98304 reads x 1.5 kb, 512 genomes, s=10000" $D/b_$label $bin predict -r $D/ref.msh -g $D/geno.tsv -i $D/reads.fq -t 5 -b 98304 || exit 1
  if [ -z "$first" ]; then first=$label; else
    cmp $D/a_$first.msh $D/a_$label.msh && cmp $D/b_$first.stdout $D/b_$label.stdout && echo "$label: outputs identical to $first's" || { echo "$label: outputs DIFFER from $first's" >&2; exit 1; }
  fi
done
