"""skx_call_rows on synthetic rows: the geometry of species_call_kernel without a reference.  Every species count, row width and
code width at which the kernel's lanes fall differently (1 and 64 species; rows of 1, 3, 17 and 64: below, across and at a wave;
row counts around a wave, around a workgroup of four waves, and many workgroups), against call_cases.call_ref in every element, with
canary-filled outputs that must stay untouched past n_rows.  The rows carry planted ties (call_cases.planted_rows)."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from call_cases import call_ref, planted_rows
from helpers import exp_env

pytestmark = pytest.mark.gpu

CANARY32, CANARY64 = 0xDEADBEEF, 0xDEADBEEFCAFEF00D
N_MAX, PAD = 5000, 3
HERE = os.path.dirname(os.path.abspath(__file__))


@functools.lru_cache(maxsize=1)
def _rows(n_sp, top):
    return planted_rows(N_MAX, n_sp, top, n_feat=64, seed=1000 * n_sp + top)


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _raw(idx, sums, codes, n):
    """skx_call_rows on the first n rows into outputs of n + PAD rows filled with canaries"""
    from sketchy_amd import _lib
    n_sp, top = idx.shape[1:]
    nf = 0 if codes is None else codes.shape[2]
    sp = np.full(n + PAD, CANARY32, np.uint32)
    ci = np.full((n + PAD, top), CANARY32, np.uint32)
    cs = np.full((n + PAD, top), CANARY64, np.uint64)
    cc = None if codes is None else np.full((n + PAD, nf), CANARY32, np.uint32)
    _lib.check(_lib.load().skx_call_rows(0, _p(idx), _p(sums), _p(codes), n, n_sp, top, nf, _p(sp), _p(ci), _p(cs), _p(cc)))
    return sp, ci, cs, cc


@pytest.mark.parametrize("top", [1, 3, 17, 64])
@pytest.mark.parametrize("n_sp", [1, 2, 5, 63, 64])
def test_call_rows_equals_call_ref_and_leaves_canaries(gpu, n_sp, top):
    idx, sums, codes64 = _rows(n_sp, top)
    for nf in (0, 1, 64):
        codes = None if nf == 0 else np.ascontiguousarray(codes64[:, :, :nf])
        want = call_ref(idx, sums, codes)
        if nf == 0 and n_sp >= 2:  # (the workload must be one the tie rule decides and one that calls more than one species)
            lead = sums[:, :, 0]
            assert ((lead == lead.max(axis=1, keepdims=True)).sum(axis=1) > 1).any() and len(set(want["call_species"].tolist())) > 1
        for n in (0, 1, 63, 64, 65, 257, N_MAX):
            sp, ci, cs, cc = _raw(idx, sums, codes, n)
            what = f"n_species={n_sp} top={top} n_features={nf} n_rows={n}"
            np.testing.assert_array_equal(sp[:n], want["call_species"][:n], err_msg=what)
            np.testing.assert_array_equal(ci[:n], want["call_idx"][:n], err_msg=what)
            np.testing.assert_array_equal(cs[:n], want["call_sum"][:n], err_msg=what)
            assert (sp[n:] == CANARY32).all() and (ci[n:] == CANARY32).all() and (cs[n:] == CANARY64).all(), what
            if nf:
                np.testing.assert_array_equal(cc[:n], want["call_codes"][:n], err_msg=what)
                assert (cc[n:] == CANARY32).all(), what


def test_call_rows_optional_outputs_and_the_python_wrapper(gpu):
    from sketchy_amd import _lib, api
    idx, sums, codes = planted_rows(300, 5, 3, n_feat=4, seed=7)
    want = call_ref(idx, sums, codes)
    got = api.call_rows(idx, sums, codes)
    for k in ("call_species", "call_idx", "call_sum", "call_codes"):
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    assert api.call_rows(idx, sums)["call_codes"] is None
    sp = np.zeros(300, np.uint32)  # the species alone
    _lib.check(_lib.load().skx_call_rows(0, _p(idx), _p(sums), None, 300, 5, 3, 0, _p(sp), None, None, None))
    np.testing.assert_array_equal(sp, want["call_species"])
    empty = api.call_rows(idx[:0], sums[:0], codes[:0])
    assert empty["call_species"].shape == (0,) and empty["call_idx"].shape == (0, 3) and empty["call_codes"].shape == (0, 4)


@pytest.mark.parametrize("chunk", [7, 64])
def test_call_rows_in_several_chunks(gpu, tmp_path, chunk):
    """SKX_CALL_ROWS (experiments build) cuts the rows into chunks of 7 and of 64: 43 and 5 chunks, the last one short"""
    idx, sums, codes = planted_rows(300, 5, 3, n_feat=4, seed=11)
    src, dst = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    np.savez(src, idx=idx, sums=sums, codes=codes)
    r = subprocess.run([sys.executable, os.path.join(HERE, "call_worker.py"), "chunks", src, dst], env=exp_env(SKX_CALL_ROWS=chunk),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    got, want = np.load(dst), call_ref(idx, sums, codes)
    for k in ("call_species", "call_idx", "call_sum", "call_codes"):
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
