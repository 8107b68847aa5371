"""Helper of tools/call_rate.sh (GPU box, repo root).  Sub-commands:

  step [TREE]       (a): ms per step of 20 enqueued batches of 98 304 reads against the five species of `bench.py --config c4` (150 000
                    genomes, s = 10 000, log-normal read lengths, a stream mixed over all five), top = 1 -- a stream that never binds
                    and one that binds the species call and its event list (4 096 entries) to every batch; three repetitions each
                    after a warm-up, alternating, one process.  TREE: import sketchy_amd from there (the parent commit, which has no
                    call: only the unbound stream is timed)
  inputs DIR        (c): five references of 8 000 / 8 000 / 6 000 / 5 000 / 3 000 genomes (s = 1 000) as DIR/sp{i}.msh + DIR/sp{i}.tsv
                    (tables of 1 .. 5 columns) and DIR/reads.fq: 262 144 reads of 1.5 kb, a quarter from species 0's truth strain, then
                    three quarters from species 3's -- the call flips once species 3 has caught up
  agree DIR TOP MODE   the multi-reference output DIR/multi.out against the five single-reference outputs DIR/single{i}.out: per read
                    the block of the species called by the rule, species field removed (MODE rows | consensus; for consensus the
                    called species comes from DIR/lead{i}.out, the same runs' rows)
  filter PLAIN CHANGES TOP   the blocks of PLAIN (multi-reference `predict -s`) that differ from the block before in anything but the read
                    number and the shared_hashes column, compared with CHANGES byte for byte
  spread FILE LABEL    wall time of the runs listed in FILE ("nanoseconds reads" per line): reads/s of each, median, max - min
"""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, CAP = 98304, 4096
SIZES_CLI, S_CLI, L, N_READS = (8000, 8000, 6000, 5000, 3000), 1000, 1500, 262144


def step(tree):
    import torch  # first: its bundled HIP runtime must be the one the process ends up with
    sys.path.insert(0, tree or HERE)
    from sketchy_amd import _lib, api, synth
    sys.path.insert(0, HERE)
    from bench import CONFIGS
    species, s, read_len, sigma, _ = CONFIGS["c4"]
    has = any(n == "skx_stream_bind_call" for n, _, _ in _lib.SYMBOLS)
    tdev, n_sp, steps, n_dist, top = "cuda:0", len(species), 20, 10, 1
    refs = [synth.make_reference(n, s, k=16, hash_seed=0, rng_seed=1 + i, device=tdev, mode="snp") for i, n in enumerate(species)]
    sources = [torch.from_numpy(r["truth_genome"]).to(tdev) for r in refs]

    def make_batch(seed):
        per = [B // n_sp + (1 if i < B % n_sp else 0) for i in range(n_sp)]
        parts = [synth.make_reads_torch(sources[i], per[i], read_len, err=0.05, rng_seed=seed * 31 + i, lognormal_sigma=sigma, device=tdev)
                 for i in range(n_sp)]
        return synth.mix_reads_torch(parts, rng_seed=seed)
    batches = [make_batch(1000 + i) for i in range(n_dist)]
    n_bases = [int(o[-1].item()) for _, o in batches]
    R = api.ReferenceSketch([r["ref"] for r in refs], [r["col_len"] for r in refs], k=16, seed=0, device=0)
    S_ = api.SumOfSharedHashes(R, top=top, max_batch_reads=B, max_batch_bases=max(n_bases))
    d_ti = torch.zeros((steps, B, n_sp * top), dtype=torch.int32, device=tdev)
    d_ts = torch.zeros((steps, B, n_sp * top), dtype=torch.int64, device=tdev)
    call = [[api.DeviceBuffer(n) for n in (B * 4, B * top * 4, B * top * 8)] for _ in range(steps)]
    ev = [[api.DeviceBuffer(n) for n in (4, CAP * 4, CAP * 4, CAP * top * 4, CAP * top * 8)] for _ in range(steps)]
    torch.cuda.synchronize()
    modes = ("unbound", "call") if has else ("unbound",)
    ms, n_ev = {m: [] for m in modes}, []
    for rep in range(4):  # (the first round warms up)
        for mode in modes:
            S_.reset()
            S_.sync()
            t0 = time.perf_counter()
            for i in range(steps):
                kw = {}
                if mode == "call":
                    c, e = call[i], ev[i]
                    kw = dict(call=(c[0].ptr, c[1].ptr, c[2].ptr), call_changes=(CAP, e[0].ptr, e[1].ptr, e[2].ptr, e[3].ptr, e[4].ptr))
                bases, offs = batches[i % n_dist]
                S_.enqueue_device(bases.data_ptr(), offs.data_ptr(), B, n_bases[i % n_dist], d_ti[i].data_ptr(), d_ts[i].data_ptr(), **kw)
            S_.sync()
            if rep:
                ms[mode].append((time.perf_counter() - t0) * 1e3 / steps)
            if mode == "call" and rep == 1:
                n_ev = [int(e[0].to_numpy(np.uint32, 1)[0]) for e in ev]
                sp = call[steps - 1][0].to_numpy(np.uint32, B)
                lead = d_ts[steps - 1].cpu().numpy().astype(np.uint64).reshape(B, n_sp, top)[:, :, 0]
                assert (sp == np.argmax(lead, axis=1)).all(), "the call of the last batch is not the argmax of its leads"
    label = "parent" if tree else "this"
    print(f"    {label}: {steps} enqueued batches of {B} reads against {n_sp} species ({sum(species)} genomes, s = {s}), top = {top}, ms per step, "
          "three repetitions (alternating, one process):")
    for m in modes:
        v = ms[m]
        print(f"      {m:8s} median {sorted(v)[1]:.3f}  max - min {max(v) - min(v):.3f}  runs " + ",".join(f"{x:.3f}" for x in v)
              + (f"   call events per batch {min(n_ev)} .. {max(n_ev)}; the last batch's call checked against its rows" if m == "call" else ""))


def inputs(d):
    import torch
    sys.path.insert(0, HERE)
    from sketchy_amd import synth
    from sketchy_amd.mshio import write_msh
    refs = [synth.make_reference(n, S_CLI, k=16, hash_seed=0, rng_seed=51 + i, device="cuda:0", mode="snp") for i, n in enumerate(SIZES_CLI)]
    for i, r in enumerate(refs):
        names = [f"sp{i}_g{g:05d}.fa" for g in range(r["ref"].shape[0])]
        write_msh(f"{d}/sp{i}.msh", names, r["ref"], r["col_len"], kmer=16, seed=0)
        with open(f"{d}/sp{i}.tsv", "w") as f:
            f.write("id\t" + "\t".join(f"col{j}" for j in range(i + 1)) + "\n")
            f.write("".join(nm + "".join(f"\tv{(g * (j + 3)) % (5 + j)}" for j in range(i + 1)) + "\n" for g, nm in enumerate(names)))
    parts = []
    for sp, n, seed in ((0, N_READS // 4, 7), (3, N_READS - N_READS // 4, 8)):
        src = torch.from_numpy(refs[sp]["truth_genome"]).to("cuda:0")
        b, o = synth.make_reads_torch(src, n, L, err=0.05, rng_seed=seed, lognormal_sigma=0.0, device="cuda:0")
        parts.append(b.cpu().numpy().reshape(n, L))
    reads = np.concatenate(parts)
    rec = np.empty((N_READS, 3 + L + 3 + L + 1), np.uint8)  # "@r\n" + bases + "\n+\n" + quality + "\n"
    rec[:, :3] = np.frombuffer(b"@r\n", np.uint8)
    rec[:, 3:3 + L] = reads
    rec[:, 3 + L:6 + L] = np.frombuffer(b"\n+\n", np.uint8)
    rec[:, 6 + L:6 + 2 * L] = ord("I")
    rec[:, -1] = ord("\n")
    rec.tofile(f"{d}/reads.fq")


def _blocks(path, top):
    with open(path, "rb") as f:
        lines = f.readlines()
    assert len(lines) % top == 0, (path, len(lines), top)
    return [lines[i:i + top] for i in range(0, len(lines), top)]


def agree(d, top, mode):
    n_sp = len(SIZES_CLI)
    lead_files = [f"{d}/lead{i}.out" if mode == "consensus" else f"{d}/single{i}.out" for i in range(n_sp)]
    lead_top = top  # (consensus: the lead files are the same runs' rows)
    lead = np.array([[int(b[0].split(b"\t")[2]) for b in _blocks(p, lead_top)] for p in lead_files])
    called = np.argmax(lead, axis=0)
    per = 1 if mode == "consensus" else top
    single = [_blocks(f"{d}/single{i}.out", per) for i in range(n_sp)]
    multi = _blocks(f"{d}/multi.out", per)
    ok = len(multi) == lead.shape[1]
    for r, b in enumerate(multi):
        if not ok:
            break
        f = [ln.split(b"\t", 2) for ln in b]
        ok = all(x[1] == b"sp%d" % called[r] for x in f) and [x[0] + b"\t" + x[2] for x in f] == single[called[r]][r]
    flips = int((called[1:] != called[:-1]).sum())
    print(f"{len(multi)} reads, called species {sorted(set(called.tolist()))}, {flips} changes of species: every block "
          + ("equals the called species' own run" if ok else "DIFFERS from the called species' own run"))
    sys.exit(0 if ok else 1)


def filter_(plain, changes, top):
    n_plain, n_kept, prev, same = 0, 0, None, True
    with open(changes, "rb") as g:
        for b in _blocks(plain, top):
            n_plain += len(b)
            key = [ln.split(b"\t")[1:3] + ln.split(b"\t")[4:] for ln in b]
            if key != prev:
                n_kept += len(b)
                same = same and all(g.readline() == ln for ln in b)
            prev = key
        same = same and g.readline() == b""
    print(f"lines {n_plain} -> {n_kept} with --changes, filtered text {'matches' if same else 'DIFFERS'}")
    sys.exit(0 if same else 1)


def spread(path, label):
    runs = [(float(ln.split()[0]) / 1e9, float(ln.split()[1])) for ln in open(path) if ln.strip()]
    rate = [n / s for s, n in runs]
    print(f"    {label:30s} wall median {sorted(s for s, _ in runs)[len(runs) // 2]:6.2f} s  "
          f"{sorted(rate)[len(rate) // 2] / 1e6:6.2f} M reads/s  max - min {(max(rate) - min(rate)) / 1e6:5.2f}  runs " + ",".join(f"{v / 1e6:.2f}" for v in rate))


if __name__ == "__main__":
    cmd, a = sys.argv[1], sys.argv[2:]
    {"step": lambda: step(a[0] if a else None), "inputs": lambda: inputs(a[0]), "agree": lambda: agree(a[0], int(a[1]), a[2]),
     "filter": lambda: filter_(a[0], a[1], int(a[2])), "spread": lambda: spread(a[0], a[1])}[cmd]()
