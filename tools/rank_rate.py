"""tools/rank_rate.sh's driver: wall time of ranking N pooled sketches against a reference two ways in one process, on the same
queries --
  old   ReferenceSketch.common_hashes (n_query x n_genomes counts come back) + a stable argsort per row on the host
  new   ReferenceSketch.rank_sketches (counted and selected on the device, n_query x top rows come back)
and the un-timed check that both give identical rows.  One warm-up each, then the two alternate; medians.
usage: rank_rate.py SHAPE   (c2: 40 000 genomes x s = 10 000, N = 1 024; toy: 64 genomes x s = 1 000, N = 1 024)"""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {"c2": (40000, 10000, 1024, 3), "toy": (64, 1000, 1024, 7)}
TOP = 5


def main():
    shape = sys.argv[1]
    n_genomes, s, n_query, reps = SHAPES[shape]
    import torch  # first: its bundled HIP runtime must be the one the process ends up with
    import numpy as np
    from sketchy_amd import api, synth
    ref = synth.make_reference(n_genomes, s, rng_seed=1, device="cuda:0" if torch.cuda.is_available() else "numpy")
    # a sample that covers its strain pools to (nearly) the strain's own sketch: a reference column with 3 % of its hashes replaced
    rng = np.random.default_rng(7)
    q = ref["ref"][rng.integers(0, n_genomes, n_query)].copy()
    hi = int(ref["ref"].max())
    swap = rng.random(q.shape) < 0.03
    q[swap] = rng.integers(0, hi, int(swap.sum()), dtype=np.uint64)
    q.sort(axis=1)
    qlen = np.full(n_query, s, np.uint32)
    for i in range(n_query):  # (strictly ascending rows: duplicates dropped)
        u = np.unique(q[i])
        q[i, :len(u)], q[i, len(u):], qlen[i] = u, 0, len(u)
    if api.device_count() < 1:
        raise SystemExit("no HIP device (this measurement has no CPU path)")
    R = api.ReferenceSketch(ref["ref"], ref["col_len"])

    t_sort = []  # the host half of `old` (every call, the warm-up included)

    def old():
        c = R.common_hashes(q, qlen)
        t0 = time.perf_counter()
        order = np.argsort(-c.astype(np.int64), axis=1, kind="stable")[:, :TOP]
        t_sort.append(time.perf_counter() - t0)
        return order.astype(np.uint32), np.take_along_axis(c, order, axis=1)

    def new():
        idx, val = R.rank_sketches(q, qlen, top=TOP)
        return idx[:, 0], val[:, 0]

    a, b = old(), new()  # warm-up of both, and the check
    same = bool((a[0] == b[0]).all() and (a[1] == b[1]).all())
    t = {"old": [], "new": []}
    for _ in range(reps):
        for name, fn in (("old", old), ("new", new)):
            t0 = time.perf_counter()
            fn()  # (both end in a synchronised copy to the host)
            t[name].append(time.perf_counter() - t0)
    mo, mn = statistics.median(t["old"]), statistics.median(t["new"])
    print(f"{shape}: {n_genomes} genomes x s={s}, {n_query} queries, top={TOP}, {reps} alternating repetitions after one warm-up each")
    print(f"{shape} old common_hashes + host stable argsort  median_wall_s={mo:.4f} runs_s={','.join('%.4f' % x for x in t['old'])}")
    print(f"{shape}     of which the host argsort            median_wall_s={statistics.median(t_sort[1:]):.4f}")
    print(f"{shape} new rank_sketches                        median_wall_s={mn:.4f} runs_s={','.join('%.4f' % x for x in t['new'])}")
    print(f"{shape} rows identical: {same}   ratio old / new = {mo:.4f} / {mn:.4f} = {mo / mn:.1f}x")
    R.close()
    if not same:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
