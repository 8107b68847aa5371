#!/bin/bash
# usage (GPU box, repo root): tools/pool_rate.sh LABEL=BIN [LABEL=BIN ...]
# Wall time of the two subcommands that pool several records into one sketch, for each given `sketchy-hip` binary (each next to the
# libsketchy_hip.so it was linked against) on the same inputs, in the same job:
#   (a) `sketch`  of 64 genome files of 50 contigs x 50 kb at s = 10 000
#   (b) offline `predict` of 98 304 reads x 1.5 kb against a 512-genome reference at s = 10 000 (one batch: -b 98304)
# One warm-up run, then the median of five.  Inputs come from sketchy_amd.synth; the outputs of all binaries are compared byte for byte.
# A second binary = the parent commit's, built from a `git worktree` outside the tree and copied next to this one (out/ is ignored).
# A label that ends in +counts (this+counts=BIN) runs leg (a) with `sketch --counts` (the abundance of every hash: a second hashing
# walk over the bases on the device, counts32 in the file) and no leg (b); its hashes, lengths and valid k-mers must equal the first
# binary's, its counts must add up to no more than the valid k-mers.  POOL_RATE_API=1 adds the two library calls alone on the same 64
# genomes (api.sketch_groups without / with counts, inputs in memory, alternating, median of 21): what the counts cost without process start-up,
# parsing and the file.
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
  if [ "${label%+counts}" != "$label" ]; then
    timed $label "(a) sketch --counts 64 files x 50 contigs x 50 kb, s=10000" $D/a_$label $bin sketch -i $D/genome*.fa -o $D/a_$label.msh -s 10000 --counts || exit 1
    [ -n "$first" ] && { python3 - $D/a_$first.msh $D/a_$label.msh <<'PY' || exit 1
import sys
sys.path.insert(0, ".")
import numpy as np
from sketchy_amd.mshio import read_msh
a, b = read_msh(sys.argv[1]), read_msh(sys.argv[2])
assert a[:2] == b[:2] and len(a[2]) == len(b[2])
for x, y in zip(a[2], b[2]):
    assert x["name"] == y["name"] and x["length"] == y["length"] and x["num_valid_kmers"] == y["num_valid_kmers"]
    assert np.array_equal(x["hashes"], y["hashes"]) and len(x["counts"]) == 0 and len(y["counts"]) == len(y["hashes"])
    assert y["counts"].min() >= 1 and int(y["counts"].astype(np.uint64).sum()) <= y["num_valid_kmers"]
print("counts: hashes, lengths and valid k-mers identical to the plain file's; one count >= 1 per hash")
PY
    }
    continue
  fi
  timed $label "(a) sketch 64 files x 50 contigs x 50 kb, s=10000" $D/a_$label $bin sketch -i $D/genome*.fa -o $D/a_$label.msh -s 10000 || exit 1
  timed $label "(b) offline predict 98304 reads x 1.5 kb, 512 genomes, s=10000" $D/b_$label $bin predict -r $D/ref.msh -g $D/geno.tsv -i $D/reads.fq -t 5 -b 98304 || exit 1
  if [ -z "$first" ]; then first=$label; else
    cmp $D/a_$first.msh $D/a_$label.msh && cmp $D/b_$first.stdout $D/b_$label.stdout && echo "$label: outputs identical to $first's" || { echo "$label: outputs DIFFER from $first's" >&2; exit 1; }
  fi
done
if [ -n "$POOL_RATE_API" ]; then
  timeout -k 10 300 python3 - $D <<'PY' || exit 1
import glob, sys, time
sys.path.insert(0, ".")
import numpy as np
from sketchy_amd import api
recs, first = [], [0]
for path in sorted(glob.glob(sys.argv[1] + "/genome*.fa")):
    recs += [l for l in open(path, "rb").read().split(b"\n") if l and not l.startswith(b">")]
    first.append(len(recs))
bases = np.frombuffer(b"".join(recs), np.uint8)
offsets = np.concatenate([[0], np.cumsum([len(r) for r in recs])]).astype(np.uint64)
first = np.array(first, np.uint32)
ts = {False: [], True: []}
for rep in range(22):  # plain and counted calls alternate; the first pair warms up
    for counted in (False, True):
        t0 = time.perf_counter()
        out = api.sketch_groups(bases, offsets, first, k=16, seed=0, s=10000, want_valid_kmers=True, want_counts=counted)
        ts[counted].append(time.perf_counter() - t0)
        if counted:
            assert all(np.array_equal(x, y) for x, y in zip(po, out[:3]))
        else:
            po = out
pt, ct = ts[False][1:], ts[True][1:]
p, c = float(np.median(pt)), float(np.median(ct))
f = lambda ts: ",".join("%.3f" % t for t in ts)
print("api sketch_groups        64 groups x 50 records x 50 kb, s=10000 median_wall_s=%.3f runs_s=%s" % (p, f(pt)))
print("api sketch_groups+counts 64 groups x 50 records x 50 kb, s=10000 median_wall_s=%.3f runs_s=%s" % (c, f(ct)))
print("api ratio counted / plain = %.2f" % (c / p))
PY
fi
