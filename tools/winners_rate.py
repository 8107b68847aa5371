"""Helper of tools/winners_rate.sh (GPU box, repo root).  Sub-command:

  step [TREE]    (a) + (b): at bench.py's default shapes (config c2: 40 000 genomes, s = 10 000, 1.5 kb reads from the truth strain,
                 top = 1) 20 batches of 98 304 reads through skx_stream_enqueue_device on a stream with coverage enabled, ms per step,
                 three repetitions after a warm-up.  Then, on this commit, after the 20 batches: the time of skx_stream_winners,
                 skx_stream_winners_rank (top 5) and skx_stream_winners_rows (16 genomes), each beside the coverage query of the same
                 shape, five repetitions; the three are checked against each other and against the invariants of the definition.  With
                 the experiments build (SKX_LIB_PATH) and SKX_WINNERS_TIMES=1 the library prints the host's part of every query -- the
                 copy down, the sort, the copy up -- to stderr; tools/winners_rate.sh collects those lines.
                 TREE: import sketchy_amd from there (the parent commit, which has no winners: only the steps are timed)
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
    has = any(n == "skx_stream_winners" for n, _, _ in _lib.SYMBOLS)
    tdev, steps, n_dist, top = "cuda:0", 20, 10, 1
    ref = synth.make_reference(species[0], s, k=16, hash_seed=0, rng_seed=1, device=tdev, mode="snp")
    src = torch.from_numpy(ref["truth_genome"]).to(tdev)
    batches = [synth.make_reads_torch(src, B, read_len, err=0.05, rng_seed=1000 + i, lognormal_sigma=sigma, device=tdev) for i in range(n_dist)]
    n_bases = [int(o[-1].item()) for _, o in batches]
    R = api.ReferenceSketch(ref["ref"], ref["col_len"], k=16, seed=0, device=0)
    C = api.SumOfSharedHashes(R, top=top, max_batch_reads=B, max_batch_bases=max(n_bases))
    C.enable_coverage()
    d_ti = torch.zeros((steps, B, top), dtype=torch.int32, device=tdev)
    d_ts = torch.zeros((steps, B, top), dtype=torch.int64, device=tdev)
    torch.cuda.synchronize()
    ms = []
    for rep in range(4):  # (the first round warms up)
        C.reset()
        C.sync()
        t0 = time.perf_counter()
        for i in range(steps):
            bases, offs = batches[i % n_dist]
            C.enqueue_device(bases.data_ptr(), offs.data_ptr(), B, n_bases[i % n_dist], d_ti[i].data_ptr(), d_ts[i].data_ptr())
        C.sync()
        if rep:
            ms.append((time.perf_counter() - t0) * 1e3 / steps)
    label = "parent" if tree else "this"
    print(f"    {label}: {steps} enqueued batches of {B} reads against {species[0]} genomes (s = {s}), top = {top}, coverage enabled, ms per step, "
          "three repetitions:")
    print(f"      median {_med(ms):.3f}  max - min {max(ms) - min(ms):.3f}  runs " + ",".join(f"{x:.3f}" for x in ms))
    if not has:
        return
    n = species[0]
    rows = np.array([(i * 2503 + 17) % n for i in range(16)], np.uint32)
    names = ("winners (40 000 genomes)", "coverage (40 000 genomes)", "winners_rank top 5", "coverage_rank top 5", "winners_rows 16 genomes",
             "coverage_rows 16 genomes")
    times = {k: [] for k in names}
    for _ in range(6):  # (the first round warms up and allocates the scratch)
        t = [time.perf_counter()]
        cov, won = C.winners(); t.append(time.perf_counter())
        plain = C.coverage(); t.append(time.perf_counter())
        idx, val = C.winners_rank(5); t.append(time.perf_counter())
        C.coverage_rank(5); t.append(time.perf_counter())
        pc, pw = C.winners_rows(rows); t.append(time.perf_counter())
        C.coverage_rows(rows); t.append(time.perf_counter())
        for k, a, b in zip(names, t[:-1], t[1:]):
            times[k].append((b - a) * 1e3)
    order = np.lexsort((np.arange(n), -won.astype(np.int64)))[:5]
    assert (cov == plain).all() and (idx[0] == order).all() and (val[0] == won[order]).all(), "the queries disagree"
    assert (pc == cov[rows]).all() and (pw == won[rows]).all(), "the list and the table disagree"
    assert (won <= cov).all()
    ki = R.rare_index
    print(f"(b) the queries after the {steps} batches ({steps * B} reads; key table of {ki['keys']} distinct hashes), host wall ms per call "
          "(flush found nothing pending), five repetitions:")
    for k, v in times.items():
        v = v[1:]
        print(f"      {k:26s} median {_med(v):.3f}  max - min {max(v) - min(v):.3f}  runs " + ",".join(f"{x:.3f}" for x in v))
    print(f"      won: sum {int(won.sum())} = distinct seen reference hashes, {int((won > 0).sum())} genomes win something, max {int(won.max())} "
          f"(genome {int(won.argmax())}, covered {int(cov[int(won.argmax())])}); top 5 by won {idx[0].tolist()} with {val[0].tolist()}; "
          f"top 5 by covered {np.lexsort((np.arange(n), -cov.astype(np.int64)))[:5].tolist()}; the queries agree, won <= covered")


if __name__ == "__main__":
    cmd, a = sys.argv[1], sys.argv[2:]
    {"step": lambda: step(a[0] if a else None)}[cmd]()
