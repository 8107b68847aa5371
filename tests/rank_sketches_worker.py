"""Child process of tests/test_gpu_rank_sketches.py: with whatever library and knobs the environment selects (the experiments build)
runs ReferenceSketch.predict_groups on the .npz file's records -- SKX_PREDICT_GROUPS cuts the groups into chunks -- and the
selection kernel alone (skx_debug_row_topk, experiments build only) on its synthetic counts; writes the results next to it."""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sketchy_amd import _lib, api  # noqa: E402

src, dst = sys.argv[1], sys.argv[2]
z = np.load(src)
out = {}
R = api.ReferenceSketch(z["ref"], z["col_len"])
idx, val, sk, sl, vk = R.predict_groups(z["bases"], z["offsets"], z["first"], top=int(z["top"]), want_sketches=True, want_valid_kmers=True)
out.update(idx=idx, val=val, sk=sk, sl=sl, vk=vk)
R.close()
L = _lib.load()
fn = L.skx_debug_row_topk
fn.restype = C.c_int
fn.argtypes = [C.c_int, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
for i in range(int(z["n_topk"])):
    counts = np.ascontiguousarray(z[f"counts{i}"], np.uint32)
    for top in z["tops"].tolist():
        ti, tv = np.zeros((len(counts), top), np.uint32), np.zeros((len(counts), top), np.uint32)
        _lib.check(fn(0, counts.ctypes.data, counts.shape[0], counts.shape[1], top, int(z[f"bound{i}"]), ti.ctypes.data, tv.ctypes.data))
        out[f"ti{i}_{top}"], out[f"tv{i}_{top}"] = ti, tv
np.savez(dst, **out)
