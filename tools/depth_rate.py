"""Helper of tools/depth_rate.sh (GPU box, repo root).  Sub-command:

  step [TREE]    (a) + (b): at bench.py's default shapes (config c2: 40 000 genomes, s = 10 000, 1.5 kb reads from the truth strain,
                 top = 1) 20 batches of 98 304 reads through skx_stream_enqueue_device, ms per step -- a stream that never enables
                 anything, one with coverage and one with depth; three repetitions each after a warm-up, alternating, one process.
                 Then, on the depth stream after its 20 batches, the time of skx_stream_depth (whole table), skx_stream_depth_rows
                 (16 genomes) and skx_stream_coverage, five repetitions each; they are checked against each other and the table.
                 TREE: import sketchy_amd from there (the parent commit, which has no depth: the other two streams are timed)
"""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = 98304


def _med(v):
    return sorted(v)[len(v) // 2]


def step(tree):
    import torch  # first: its bundled HIP runtime must be the one the process ends up with
    sys.path.insert(0, tree or HERE)
    from sketchy_amd import _lib, api, synth
    sys.path.insert(0, HERE)
    from bench import CONFIGS
    species, s, read_len, sigma, _ = CONFIGS["c2"]
    has = any(n == "skx_stream_enable_depth" for n, _, _ in _lib.SYMBOLS)
    tdev, steps, n_dist, top = "cuda:0", 20, 10, 1
    ref = synth.make_reference(species[0], s, k=16, hash_seed=0, rng_seed=1, device=tdev, mode="snp")
    src = torch.from_numpy(ref["truth_genome"]).to(tdev)
    batches = [synth.make_reads_torch(src, B, read_len, err=0.05, rng_seed=1000 + i, lognormal_sigma=sigma, device=tdev) for i in range(n_dist)]
    n_bases = [int(o[-1].item()) for _, o in batches]
    R = api.ReferenceSketch(ref["ref"], ref["col_len"], k=16, seed=0, device=0)
    modes = ("plain", "coverage", "depth") if has else ("plain", "coverage")
    S = {m: api.SumOfSharedHashes(R, top=top, max_batch_reads=B, max_batch_bases=max(n_bases)) for m in modes}
    S["coverage"].enable_coverage()
    if has:
        S["depth"].enable_depth()
    d_ti = torch.zeros((steps, B, top), dtype=torch.int32, device=tdev)
    d_ts = torch.zeros((steps, B, top), dtype=torch.int64, device=tdev)
    torch.cuda.synchronize()
    ms = {m: [] for m in modes}
    for rep in range(4):  # (the first round warms up)
        for m in modes:
            S[m].reset()
            S[m].sync()
            t0 = time.perf_counter()
            for i in range(steps):
                bases, offs = batches[i % n_dist]
                S[m].enqueue_device(bases.data_ptr(), offs.data_ptr(), B, n_bases[i % n_dist], d_ti[i].data_ptr(), d_ts[i].data_ptr())
            S[m].sync()
            if rep:
                ms[m].append((time.perf_counter() - t0) * 1e3 / steps)
    label = "parent" if tree else "this"
    print(f"    {label}: {steps} enqueued batches of {B} reads against {species[0]} genomes (s = {s}), top = {top}, ms per step, "
          "three repetitions (alternating, one process):")
    for m in modes:
        v = ms[m]
        print(f"      {m:9s} median {_med(v):.3f}  max - min {max(v) - min(v):.3f}  runs " + ",".join(f"{x:.3f}" for x in v))
    if not has:
        return
    D = S["depth"]
    n = species[0]
    rows = np.array([(i * 2503 + 17) % n for i in range(16)], np.uint32)
    times = {"depth (40 000 genomes)": [], "depth_rows 16 genomes": [], "coverage (40 000 genomes)": []}
    for _ in range(6):  # (the first round warms up and allocates the select's scratch)
        t0 = time.perf_counter(); cov, med, tot = D.depth(); t1 = time.perf_counter()
        part = D.depth_rows(rows); t2 = time.perf_counter()
        only = D.coverage(); t3 = time.perf_counter()
        for k, dt in zip(times, (t1 - t0, t2 - t1, t3 - t2)):
            times[k].append(dt * 1e3)
    assert (only == cov).all() and all((p == a[rows]).all() for p, a in zip(part, (cov, med, tot))), "the queries disagree"
    assert (tot == D.table()).all(), "total differs from the table"
    h, c = D.depth_export()
    assert len(h) == D.depth_count() and int(c.max()) >= int(med.max())
    ki = R.rare_index
    print(f"(b) the queries on the depth stream after its {steps} batches ({steps * B} reads; key table of {ki['keys']} distinct hashes), "
          "host wall ms per call (flush found nothing pending), five repetitions:")
    for k, v in times.items():
        v = v[1:]
        print(f"      {k:26s} median {_med(v):.3f}  max - min {max(v) - min(v):.3f}  runs " + ",".join(f"{x:.3f}" for x in v))
    print(f"      median multiplicity: max {int(med.max())}, median over the genomes {int(np.median(med))}; deepest hash {int(c.max())} of "
          f"{steps * B} reads; {len(h)} distinct hashes seen; covered = coverage, total = table, rows = the table's entries")


if __name__ == "__main__":
    cmd, a = sys.argv[1], sys.argv[2:]
    {"step": lambda: step(a[0] if a else None)}[cmd]()
