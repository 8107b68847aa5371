"""Helper of tools/consensus_rate.sh (GPU box, repo root).  Sub-commands, each a process of its own (torch and the HIP library do
not share one):

  inputs DIR   C2's reference (40 000 genomes x s = 10 000, SURVEY 8(d)'s SNP tree) as DIR/ref.npy, 11 x 98 304 reads of 1.5 kb from
               its truth strain as DIR/reads.fq, a genotype table of 16 columns as DIR/geno.tsv            (torch, no library)
  step DIR     (c): ms per step of 20 enqueued batches of 98 304 reads, top = 5, with and without a consensus output of 16
               columns bound to every batch -- one process, one reference, alternating, table reset before each run
  msh DIR      DIR/ref.npy -> DIR/ref.msh (what the CLI reads); removes ref.npy
  median FILE  reads_per_s of the --timing lines in FILE: all of them, and the median of all but the first
  bench FILE.. `value` of the JSON result lines bench.py printed into the files: all of them, median, max - min
"""
import json
import os
import re
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
N, S, L, B, NB, F = 40000, 10000, 1500, 98304, 11, 16
REC = 8 + L + 3 + L + 1


def geno_columns(i):
    return [f"c{j}v{(i * (2 * j + 3)) % (j + 2)}" for j in range(F)]


def inputs(d):
    import torch
    from sketchy_amd import synth
    ref = synth.make_reference(N, S, rng_seed=1, device="cuda", mode="snp")
    np.save(d + "/ref.npy", ref["ref"])
    src = torch.from_numpy(ref["truth_genome"]).to("cuda")
    with open(d + "/reads.fq", "wb") as f:
        for i in range(NB):
            b, _ = synth.make_reads_torch(src, B, L, rng_seed=7000 + i, device="cuda")
            rec = np.empty((B, REC), np.uint8)
            rec[:, :8] = np.frombuffer(b"@read/1\n", np.uint8)
            rec[:, 8:8 + L] = b.cpu().numpy().reshape(B, L)
            rec[:, 8 + L:8 + L + 3] = np.frombuffer(b"\n+\n", np.uint8)
            rec[:, 8 + L + 3:8 + 2 * L + 3] = ord("I")
            rec[:, -1] = 10
            rec.tofile(f)
    with open(d + "/geno.tsv", "w") as f:
        f.write("id\t" + "\t".join(f"col{j}" for j in range(F)) + "\n")
        f.write("".join(f"genome{i:05d}.fa\t" + "\t".join(geno_columns(i)) + "\n" for i in range(N)))
    print(f"inputs: {N} x {S} reference, {NB * B} reads x {L} bases, {F} genotype columns")


def msh(d):
    from sketchy_amd import mshio
    ref = np.load(d + "/ref.npy", mmap_mode="r")
    mshio.write_msh(d + "/ref.msh", [f"genome{i:05d}.fa" for i in range(N)], ref, kmer=16, seed=0)
    os.remove(d + "/ref.npy")


def step(d):
    from sketchy_amd import api
    R = api.ReferenceSketch(np.load(d + "/ref.npy"))
    codes, _ = api.encode_genotypes([geno_columns(i) for i in range(N)])
    R.set_genotypes(codes)
    n_dist, steps, top = 10, 20, 5
    S_ = api.SumOfSharedHashes(R, top=top, max_batch_reads=B, max_batch_bases=B * L)
    d_off = api.DeviceBuffer.from_numpy(np.arange(B + 1, dtype=np.uint64) * L)
    fq = np.memmap(d + "/reads.fq", np.uint8, "r").reshape(-1, REC)
    d_bases = [api.DeviceBuffer.from_numpy(np.ascontiguousarray(fq[i * B:(i + 1) * B, 8:8 + L]).reshape(-1)) for i in range(n_dist)]
    d_i = [api.DeviceBuffer(B * top * 4) for _ in range(steps)]
    d_s = [api.DeviceBuffer(B * top * 8) for _ in range(steps)]
    d_c = [api.DeviceBuffer(B * F * 4) for _ in range(steps)]
    ms = {False: [], True: []}
    for rep in range(6):  # (the first pair warms up)
        for bound in (False, True):
            S_.reset()
            S_.sync()
            t0 = time.perf_counter()
            for i in range(steps):
                S_.enqueue_device(d_bases[i % n_dist].ptr, d_off.ptr, B, B * L, d_i[i].ptr, d_s[i].ptr, consensus=d_c[i].ptr if bound else None)
            S_.sync()
            if rep:
                ms[bound].append((time.perf_counter() - t0) * 1e3 / steps)
    med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
    print(f"(c) {steps} enqueued batches of {B} reads, top = {top}, ms per step, median of 5 (alternating, one process):")
    print(f"    nothing bound          {med[False]:.3f}   runs " + ",".join(f"{x:.3f}" for x in ms[False]))
    print(f"    {F} columns bound       {med[True]:.3f}   runs " + ",".join(f"{x:.3f}" for x in ms[True]))
    print(f"    difference per step    {med[True] - med[False]:+.3f} ms  ({B / med[False] / 1e3:.1f} -> {B / med[True] / 1e3:.1f} M reads/s)")


def median(path):
    vals = [json.loads(m)["sketchy_hip_timing"]["reads_per_s"] for m in re.findall(r'\{"sketchy_hip_timing".*\}', open(path).read())]
    later = sorted(vals[1:])
    print(f"{later[len(later) // 2]:.1f} " + ",".join(f"{v:.0f}" for v in vals))


def bench(paths):
    vals = []
    for p in paths:
        lines = [ln for ln in open(p).read().splitlines() if ln.startswith("{")]
        vals.append(float(json.loads(lines[-1])["value"]))
    print(f"{sorted(vals)[len(vals) // 2]:.1f} {max(vals) - min(vals):.1f} " + ",".join(f"{v:.0f}" for v in vals))


if __name__ == "__main__":
    cmd, args = sys.argv[1], sys.argv[2:]
    {"inputs": lambda: inputs(args[0]), "msh": lambda: msh(args[0]), "step": lambda: step(args[0]), "median": lambda: median(args[0]),
     "bench": lambda: bench(args)}[cmd]()
