"""Helper of tools/coverage_rate.sh (GPU box, repo root).  Sub-commands:

  step [TREE]    (a) + (b): at bench.py's default shapes (config c2: 40 000 genomes, s = 10 000, 1.5 kb reads from the truth strain,
                 top = 1) 20 batches of 98 304 reads through skx_stream_enqueue_device, ms per step -- a stream that never enables
                 coverage and one that does; three repetitions each after a warm-up, alternating, one process.  Then, on the enabled
                 stream after its 20 batches, the time of skx_stream_coverage, skx_stream_coverage_rank (top 5) and
                 skx_stream_coverage_rows (16 genomes), five repetitions each; the three are checked against each other.
                 TREE: import sketchy_amd from there (the parent commit, which has no coverage: only the plain stream is timed)
  compare        (c): config c1's reference (5 000 genomes, s = 1 000), 16 384 reads: the queries beside the only other way to the number
                 -- every read's debug sketch downloaded (push(want_sketches=True)), their union, numpy's isin over the reference --
                 which must give the same counts
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
    has = any(n == "skx_stream_enable_coverage" for n, _, _ in _lib.SYMBOLS)
    tdev, steps, n_dist, top = "cuda:0", 20, 10, 1
    ref = synth.make_reference(species[0], s, k=16, hash_seed=0, rng_seed=1, device=tdev, mode="snp")
    src = torch.from_numpy(ref["truth_genome"]).to(tdev)
    batches = [synth.make_reads_torch(src, B, read_len, err=0.05, rng_seed=1000 + i, lognormal_sigma=sigma, device=tdev) for i in range(n_dist)]
    n_bases = [int(o[-1].item()) for _, o in batches]
    R = api.ReferenceSketch(ref["ref"], ref["col_len"], k=16, seed=0, device=0)
    modes = ("plain", "coverage") if has else ("plain",)
    S = {m: api.SumOfSharedHashes(R, top=top, max_batch_reads=B, max_batch_bases=max(n_bases)) for m in modes}
    if has:
        S["coverage"].enable_coverage()
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
    C = S["coverage"]
    n = species[0]
    rows = np.array([(i * 2503 + 17) % n for i in range(16)], np.uint32)
    times = {"coverage (40 000 genomes)": [], "coverage_rank top 5": [], "coverage_rows 16 genomes": []}
    for _ in range(6):  # (the first round warms up)
        t0 = time.perf_counter(); cov = C.coverage(); t1 = time.perf_counter()
        idx, val = C.coverage_rank(5); t2 = time.perf_counter()
        part = C.coverage_rows(rows); t3 = time.perf_counter()
        for k, dt in zip(times, (t1 - t0, t2 - t1, t3 - t2)):
            times[k].append(dt * 1e3)
    order = np.lexsort((np.arange(n), -cov.astype(np.int64)))[:5]
    assert (idx[0] == order).all() and (val[0] == cov[order]).all() and (part == cov[rows]).all(), "the three queries disagree"
    table = C.table()
    assert (cov <= ref["col_len"]).all() and (cov <= table).all()
    ki = R.rare_index
    print(f"(b) the queries on the enabled stream after its {steps} batches ({steps * B} reads; key table of {ki['keys']} distinct hashes), "
          "host wall ms per call (flush found nothing pending), five repetitions:")
    for k, v in times.items():
        v = v[1:]
        print(f"      {k:26s} median {_med(v):.3f}  max - min {max(v) - min(v):.3f}  runs " + ",".join(f"{x:.3f}" for x in v))
    print(f"      covered: max {int(cov.max())} of col_len {int(ref['col_len'][int(cov.argmax())])}, median {int(np.median(cov))}; "
          f"{int((cov == ref['col_len']).sum())} full columns; the three queries agree, covered <= col_len and <= table")


def compare():
    import torch  # noqa: F401
    sys.path.insert(0, HERE)
    from sketchy_amd import api, synth
    from bench import CONFIGS
    species, s, read_len, sigma, _ = CONFIGS["c1"]
    n_reads = 16384
    ref = synth.make_reference(species[0], s, k=16, hash_seed=0, rng_seed=1, device="cuda:0", mode="snp")
    bases, offsets = synth.make_reads(ref["truth_genome"], n_reads, read_len, err=0.05, rng_seed=7)
    R = api.ReferenceSketch(ref["ref"], ref["col_len"], k=16, seed=0, device=0)
    S = api.SumOfSharedHashes(R, top=1, max_batch_reads=n_reads, max_batch_bases=len(bases))
    S.enable_coverage()
    t0 = time.perf_counter(); S.push(bases, offsets); t_push = time.perf_counter() - t0
    q = []
    for _ in range(4):
        t0 = time.perf_counter(); cov = S.coverage(); q.append((time.perf_counter() - t0) * 1e3)
    P = api.SumOfSharedHashes(R, top=1, max_batch_reads=n_reads, max_batch_bases=len(bases))
    t0 = time.perf_counter()
    out = P.push(bases, offsets, want_sketches=True)
    t_dbg = time.perf_counter() - t0
    t0 = time.perf_counter()
    sk, sl = out["sketches"], out["sketch_len"]
    seen = np.unique(sk[np.arange(sk.shape[1])[None, :] < sl[:, None]])
    valid = np.arange(ref["ref"].shape[1])[None, :] < ref["col_len"][:, None]
    by_hand = (np.isin(ref["ref"], seen) & valid).sum(axis=1)
    t_np = time.perf_counter() - t0
    assert (by_hand == cov).all(), "the queries and the debug sketches disagree"
    print(f"(c) the only other way to the number today, at a size where it finishes: {species[0]} genomes, s = {s}, {n_reads} reads of {read_len} bases")
    print(f"      skx_stream_coverage on the enabled stream: median {_med(q[1:]):.3f} ms per query (push of the reads, marks included: {t_push * 1e3:.1f} ms)")
    print(f"      per-read debug sketches downloaded (push with want_sketches: {t_dbg * 1e3:.1f} ms, {sk.nbytes / 1e6:.0f} MB) + union and numpy isin "
          f"over the reference on the host: {t_np * 1e3:.1f} ms; same counts for all {species[0]} genomes")


if __name__ == "__main__":
    cmd, a = sys.argv[1], sys.argv[2:]
    {"step": lambda: step(a[0] if a else None), "compare": compare}[cmd]()
