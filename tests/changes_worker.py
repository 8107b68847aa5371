"""Child process of tests/test_gpu_changes.py: with whatever library and knobs the environment selects (the experiments build).
  chunks IN.npz OUT.npz   api.changes_rows on IN's rows with every cap in IN's caps (SKX_CHANGES_ROWS cuts the rows into chunks)
  passes IN.npz OUT.npz   one batch through push and push_device on a stream whose passes hold 64 distinct hashes, an event list bound;
                          SKX_DEBUG_PASS makes the library name the reads that begin a pass on stderr"""
import sys

import numpy as np

sys.path.insert(0, __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__))))
from sketchy_amd import api  # noqa: E402

SENTINEL = 0xDEADBEEF


def chunks(z):
    out = {}
    for cap in z["caps"].tolist():
        n, ev = api.changes_rows(z["rows"], cap)
        out[f"n{cap}"], out[f"ev{cap}"] = np.uint64(n), ev
    return out


def passes(z):
    ref, col_len, bases, offsets, top, cap = z["ref"], z["col_len"], z["bases"], z["offsets"], int(z["top"]), int(z["cap"])
    n = len(offsets) - 1
    R = api.ReferenceSketch(ref, col_len)
    try:
        api.set_option("stream_query_rows", 64)
        S = api.SumOfSharedHashes(R, top=top, max_batch_reads=n, max_batch_bases=int(offsets[-1]))
    finally:
        api.set_option("stream_query_rows", 0)
    out = {}
    got = S.push(bases, offsets, want_changes=cap)
    out.update(push_passes=np.uint64(S.stats()["last_passes"]), push_idx=got["topk_idx"], push_n=np.uint64(got["changes"]["n"]),
               push_read=got["changes"]["read"], push_ev_idx=got["changes"]["idx"], push_ev_sum=got["changes"]["sum"], push_sum=got["topk_sum"])
    S.reset()
    d_b, d_o = api.DeviceBuffer.from_numpy(bases), api.DeviceBuffer.from_numpy(offsets)
    d_i, d_s = api.DeviceBuffer(n * top * 4), api.DeviceBuffer(n * top * 8)
    ev = [api.DeviceBuffer.from_numpy(np.full(m, SENTINEL, t)) for m, t in ((1, np.uint32), (cap, np.uint32), (cap * top, np.uint32), (cap * top, np.uint64))]
    S.push_device(d_b.ptr, d_o.ptr, n, int(offsets[-1]), d_i.ptr, d_s.ptr, changes=(cap, ev[0].ptr, ev[1].ptr, ev[2].ptr, ev[3].ptr))
    S.sync()
    out.update(dev_passes=np.uint64(S.stats()["last_passes"]), dev_idx=d_i.to_numpy(np.uint32, (n, top)), dev_sum=d_s.to_numpy(np.uint64, (n, top)),
               dev_n=ev[0].to_numpy(np.uint32, 1), dev_read=ev[1].to_numpy(np.uint32, cap), dev_ev_idx=ev[2].to_numpy(np.uint32, (cap, top)),
               dev_ev_sum=ev[3].to_numpy(np.uint64, (cap, top)))
    for d in [d_b, d_o, d_i, d_s] + ev:
        d.free()
    S.close()
    R.close()
    return out


if __name__ == "__main__":
    mode, src, dst = sys.argv[1:4]
    np.savez(dst, **{"chunks": chunks, "passes": passes}[mode](np.load(src)))
