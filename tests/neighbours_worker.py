"""Child process of tests/test_gpu_neighbours.py: with whatever library and knobs the environment selects (the experiments build;
SKX_NEIGHBOUR_CHUNK cuts a call's genomes into chunks) runs, for every case of the .npz file and every species of the case,
ReferenceSketch.neighbours over the whole species and the row-rebuilding kernels alone (skx_debug_ref_rows, experiments build only);
writes the results next to it."""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sketchy_amd import _lib, api  # noqa: E402

src, dst = sys.argv[1], sys.argv[2]
z = np.load(src)
L = _lib.load()
fn = L.skx_debug_ref_rows
fn.restype = C.c_int
fn.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
out = {}
for i in range(int(z["n_cases"])):
    n_sp = int(z[f"n_species{i}"])
    refs = [z[f"ref{i}_{sp}"] for sp in range(n_sp)]
    R = api.ReferenceSketch(refs if n_sp > 1 else refs[0], [z[f"len{i}_{sp}"] for sp in range(n_sp)] if n_sp > 1 else z[f"len{i}_0"])
    for sp in range(n_sp):
        n, stride = refs[sp].shape
        top = min(int(z[f"top{i}"]), n - 1)
        out[f"idx{i}_{sp}"], out[f"val{i}_{sp}"] = R.neighbours(top=top, species=sp)
        rows, rlen = np.zeros((n, stride), np.uint64), np.zeros(n, np.uint32)
        _lib.check(fn(R._h, sp, 0, n, rows.ctypes.data, rlen.ctypes.data))
        a, c = 1, min(n - 1, 70)   # a range that begins inside a group of 64 genomes: the same rows
        part, plen = np.zeros((c, stride), np.uint64), np.zeros(c, np.uint32)
        _lib.check(fn(R._h, sp, a, c, part.ctypes.data, plen.ctypes.data))
        assert np.array_equal(part, rows[a:a + c]) and np.array_equal(plen, rlen[a:a + c])
        out[f"rows{i}_{sp}"], out[f"rlen{i}_{sp}"] = rows, rlen
    R.close()
np.savez(dst, **out)
