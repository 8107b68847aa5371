"""Helper of tools/changes_rate.sh (GPU box, repo root).  Inputs come from tools/consensus_rate.py (inputs / msh).  Sub-commands:

  step DIR [TREE]   (b): ms per step of 20 enqueued batches of 98 304 reads, top = 5 -- a stream that never binds, one that binds an
                    event list of 4 096 entries to every batch (index rows), one that binds it in codes mode; three repetitions each
                    after a warm-up, alternating, one process.  TREE: import sketchy_amd from there (the parent commit, which has no
                    event lists: only the unbound stream is timed)
  filter PLAIN CHANGES TOP   the blocks of PLAIN (`predict -s`, TOP lines per read) that differ from the block before them in anything
                    but the read number and the shared_hashes column, compared with CHANGES byte for byte; line counts of both
  spread FILE LABEL          reads_per_s of the --timing lines in FILE (three runs): all, median, max - min
"""
import json
import os
import re
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, S, L, B, F = 40000, 10000, 1500, 98304, 16
REC = 8 + L + 3 + L + 1
CAP = 4096


def step(d, tree):
    sys.path.insert(0, tree or HERE)
    from sketchy_amd import _lib, api
    sys.path.insert(0, os.path.join(HERE, "tools"))
    from consensus_rate import geno_columns
    has = any(n == "skx_stream_bind_changes" for n, _, _ in _lib.SYMBOLS)
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
    ev = [[api.DeviceBuffer(n) for n in (4, CAP * 4, CAP * top * 4, CAP * top * 8, CAP * F * 4)] for _ in range(steps)]
    modes = ("unbound", "rows", "codes") if has else ("unbound",)
    ms = {m: [] for m in modes}
    n_ev = {m: [] for m in modes}
    for rep in range(4):  # (the first round warms up)
        for mode in modes:
            S_.reset()
            S_.sync()
            t0 = time.perf_counter()
            for i in range(steps):
                kw = {}
                if mode != "unbound":
                    e = ev[i]
                    kw["changes"] = (CAP, e[0].ptr, e[1].ptr, e[2].ptr, e[3].ptr, e[4].ptr if mode == "codes" else None)
                S_.enqueue_device(d_bases[i % n_dist].ptr, d_off.ptr, B, B * L, d_i[i].ptr, d_s[i].ptr, **kw)
            S_.sync()
            if rep:
                ms[mode].append((time.perf_counter() - t0) * 1e3 / steps)
            if mode != "unbound" and rep == 1:
                n_ev[mode] = [int(e[0].to_numpy(np.uint32, 1)[0]) for e in ev]
    label = "parent" if tree else "this"
    print(f"    {label}: {steps} enqueued batches of {B} reads, top = {top}, ms per step, three repetitions (alternating, one process):")
    for m in modes:
        v = ms[m]
        print(f"      {m:8s} median {sorted(v)[1]:.3f}  max - min {max(v) - min(v):.3f}  runs " + ",".join(f"{x:.3f}" for x in v)
              + (f"   events per batch {min(n_ev[m])} .. {max(n_ev[m])}" if n_ev[m] else ""))


def filter_(plain, changes, top):
    kept, n_plain, prev, block = [], 0, None, []
    with open(plain, "rb") as f, open(changes, "rb") as g:
        same = True
        for ln in f:
            n_plain += 1
            block.append(ln)
            if len(block) < top:
                continue
            key = [b.split(b"\t", 3)[1::2] for b in block]
            if key != prev:
                for b in block:
                    kept.append(1)
                    same = same and g.readline() == b
            prev, block = key, []
        same = same and g.readline() == b""
    print(f"lines {n_plain} -> {len(kept)} with --changes, filtered text {'matches' if same else 'DIFFERS'}")
    sys.exit(0 if same else 1)


def spread(path, label):
    vals = [json.loads(m)["sketchy_hip_timing"]["reads_per_s"] for m in re.findall(r'\{"sketchy_hip_timing".*\}', open(path).read())]
    print(f"    {label:28s} median {sorted(vals)[len(vals) // 2] / 1e6:6.2f} M reads/s  max - min {(max(vals) - min(vals)) / 1e6:5.2f}  runs "
          + ",".join(f"{v / 1e6:.2f}" for v in vals))


if __name__ == "__main__":
    cmd, a = sys.argv[1], sys.argv[2:]
    {"step": lambda: step(a[0], a[1] if len(a) > 1 else None), "filter": lambda: filter_(a[0], a[1], int(a[2])),
     "spread": lambda: spread(a[0], a[1])}[cmd]()
