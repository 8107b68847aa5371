"""Helper of tools/composition_rate.sh (GPU box, repo root).  Sub-command:

  step CONFIG [TREE]   at bench.py's shapes of CONFIG (c2: 40 000 genomes of one species; c4: five species resident, 150 000 genomes, a
                 mixed stream of log-normal read lengths; s = 10 000, reads from one truth strain per species, top = 1) 20 batches of
                 98 304 reads through skx_stream_enqueue_device, ms per step -- a stream that never enables anything, one with depth
                 and one with composition (min_hits = 1); three repetitions each after a warm-up, alternating, one process.  Before
                 that the wall time of the first skx_stream_enable_composition on the reference (the species masks are built there)
                 and of a second stream's; afterwards the composition of the 20 batches.
                 TREE: import sketchy_amd from there (the parent commit, which has no composition: the other two streams are timed)
"""
import os
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = 98304


def _med(v):
    return sorted(v)[len(v) // 2]


def step(config, tree):
    import torch  # first: its bundled HIP runtime must be the one the process ends up with
    sys.path.insert(0, tree or HERE)
    from sketchy_amd import _lib, api, synth
    sys.path.insert(0, HERE)
    from bench import CONFIGS
    species, s, read_len, sigma, _ = CONFIGS[config]
    n_sp = len(species)
    has = any(n == "skx_stream_enable_composition" for n, _, _ in _lib.SYMBOLS)
    tdev, steps, n_dist, top = "cuda:0", 20, 10, 1
    refs = [synth.make_reference(n, s, k=16, hash_seed=0, rng_seed=1 + i, device=tdev, mode="snp") for i, n in enumerate(species)]
    src = [torch.from_numpy(r["truth_genome"]).to(tdev) for r in refs]

    def make_batch(seed):  # (bench.py's make_batch)
        if n_sp == 1:
            return synth.make_reads_torch(src[0], B, read_len, err=0.05, rng_seed=seed, lognormal_sigma=sigma, device=tdev)
        per = [B // n_sp + (1 if i < B % n_sp else 0) for i in range(n_sp)]
        return synth.mix_reads_torch([synth.make_reads_torch(src[i], per[i], read_len, err=0.05, rng_seed=seed * 31 + i, lognormal_sigma=sigma,
                                                             device=tdev) for i in range(n_sp)], rng_seed=seed)
    batches = [make_batch(1000 + i) for i in range(n_dist)]
    n_bases = [int(o[-1].item()) for _, o in batches]
    R = api.ReferenceSketch([r["ref"] for r in refs], [r["col_len"] for r in refs], k=16, seed=0, device=0)
    modes = ("plain", "depth", "composition") if has else ("plain", "depth")
    S = {m: api.SumOfSharedHashes(R, top=top, max_batch_reads=B, max_batch_bases=max(n_bases)) for m in modes}
    S["depth"].enable_depth()
    label = f"{'parent' if tree else 'this'}, {config}"
    if has:
        torch.cuda.synchronize()
        t0 = time.perf_counter(); S["composition"].enable_composition(1); t1 = time.perf_counter()
        other = api.SumOfSharedHashes(R, top=top, max_batch_reads=B, max_batch_bases=max(n_bases))
        t2 = time.perf_counter(); other.enable_composition(1); t3 = time.perf_counter()
        other.close()
        keys = R.rare_index["keys"]
        print(f"    {label}: first skx_stream_enable_composition on the reference ({n_sp} species, {sum(species)} genomes, {keys} distinct hashes"
              f"{'' if n_sp > 1 else ': one species, no mask table'}) {1e3 * (t1 - t0):.3f} ms host wall, a second stream's {1e3 * (t3 - t2):.3f} ms")
    rows = top * n_sp
    d_ti = torch.zeros((steps, B, rows), dtype=torch.int32, device=tdev)
    d_ts = torch.zeros((steps, B, rows), dtype=torch.int64, device=tdev)
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
    print(f"    {label}: {steps} enqueued batches of {B} reads against {sum(species)} genomes ({n_sp} species, s = {s}), top = {top}, ms per step, "
          "three repetitions (alternating, one process):")
    for m in modes:
        v = ms[m]
        print(f"      {m:11s} median {_med(v):.3f}  max - min {max(v) - min(v):.3f}  runs " + ",".join(f"{x:.3f}" for x in v))
    if has:
        reads, pairs = S["composition"].composition()
        assert int(reads.sum()) == steps * B, "the classes do not add up to the reads"
        assert (S["composition"].table() == S["plain"].table()).all(), "the table moved"
        print(f"      composition of the {steps * B} reads: reads {reads.tolist()} (species, ambiguous, unclassified), pairs {pairs.tolist()}")


if __name__ == "__main__":
    cmd, a = sys.argv[1], sys.argv[2:]
    {"step": lambda: step(a[0], a[1] if len(a) > 1 else None)}[cmd]()
