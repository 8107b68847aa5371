"""tools/neighbours_rate.sh's driver: wall time of the leave-one-out neighbours of a WHOLE resident reference, and for comparison what
existed before it --
  line 1  ReferenceSketch.neighbours(top=TOP): query rows rebuilt on the device from the resident matrix, self left out in the selection
  line 2  the same rows pushed through ReferenceSketch.rank_sketches from the host, in the same chunks (256 MiB of rows), with TOP + 1
          rows per genome (room for self).  That line times what existed before; its rows still hold self wherever fewer than TOP + 1
          genomes that share the whole sketch precede it.  Printed, not asserted: for how many genomes "drop self if it is there, else
          the last row" does not give line 1's rows.
A short warm-up of each (the first 256 genomes), then REPS timed runs, alternating; every run ends in a synchronised copy to the host.
usage: neighbours_rate.py SHAPE   (c2: 40 000 genomes x s = 10 000; toy: 600 genomes x s = 1 000)"""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {"c2": (40000, 10000, 2), "toy": (600, 1000, 5)}
TOP = 5
CHUNK_BYTES = 256 << 20


def main():
    shape = sys.argv[1]
    n, s, reps = SHAPES[shape]
    import torch  # first: its bundled HIP runtime must be the one the process ends up with
    import numpy as np
    from sketchy_amd import api, synth
    ref = synth.make_reference(n, s, rng_seed=1, device="cuda:0" if torch.cuda.is_available() else "numpy")
    if api.device_count() < 1:
        raise SystemExit("no HIP device (this measurement has no CPU path)")
    hashes, col_len = ref["ref"], ref["col_len"]
    R = api.ReferenceSketch(hashes, col_len)
    chunk = max(1, CHUNK_BYTES // (s * 8))

    def new(count=None):
        return R.neighbours(count=count, top=TOP)

    def old(count=None):
        m = n if count is None else count
        out = [R.rank_sketches(hashes[a:min(a + chunk, m)], col_len[a:min(a + chunk, m)], top=TOP + 1) for a in range(0, m, chunk)]
        return np.concatenate([o[0][:, 0] for o in out]), np.concatenate([o[1][:, 0] for o in out])

    new(256), old(256)
    t = {"new": [], "old": []}
    for _ in range(reps):
        for name, fn in (("new", new), ("old", old)):
            t0 = time.perf_counter()
            res = fn()
            t[name].append(time.perf_counter() - t0)
            if name == "new":
                got = res
            else:
                host = res
    # self dropped from the TOP + 1 rows on the host where it is among them, cut to TOP: does it differ from the selection that never saw self?
    me = np.arange(n, dtype=np.uint32)[:, None]
    keep = host[0] != me
    pos = np.argsort(~keep, axis=1, kind="stable")[:, :TOP]
    dropped = np.take_along_axis(host[0], pos, axis=1)
    differ = int((dropped != got[0]).any(axis=1).sum())
    mn, mo = statistics.median(t["new"]), statistics.median(t["old"])
    print(f"{shape}: {n} genomes x s={s}, top={TOP}, chunks of {chunk} genomes, {reps} alternating runs after a 256-genome warm-up each")
    print(f"{shape} line 1: neighbours (skx_ref_neighbours), all {n} genomes        median_wall_s={mn:.4f} runs_s={','.join('%.4f' % x for x in t['new'])}")
    print(f"{shape} line 2: rank_sketches from the host, same chunks, top={TOP + 1}          median_wall_s={mo:.4f} runs_s={','.join('%.4f' % x for x in t['old'])}")
    print(f"{shape} genomes whose line-2 rows with self dropped (self dropped where present, else the last row) are not line 1's rows: {differ} of {n}")
    R.close()


if __name__ == "__main__":
    main()
