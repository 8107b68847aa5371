"""skx_ref_neighbours and `sketchy-hip neighbours`: what can be checked without a device.

* the entry point is exported, bound and wrapped;
* every argument check that needs no reference handle runs before the device is touched;
* the Python wrapper refuses bad ranges before it calls into the library;
* the host under AddressSanitizer + UndefinedBehaviorSanitizer against tests/stub, which has no skx_ref_neighbours (and whose
  skx_common_hashes counts nothing): the host intersects the file's sketches itself, sorts with self skipped and votes over rows.  Rows,
  -c lines and -S counts of a 40-genome file against the oracle (neighbours_cases.py); the command-line errors end with status 2."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import neighbours_cases as nc
from sketchy_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "stub", "sketchy-hip-asan")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=99", UBSAN_OPTIONS="halt_on_error=1:exitcode=98")


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _call(ref=None, species=0, first=0, count=1, top_k=1, nb_idx="ok", nb_shared="ok", codes=None):
    L = _lib.load()
    idx = np.zeros(64, np.uint32) if isinstance(nb_idx, str) else nb_idx
    val = np.zeros(64, np.uint32) if isinstance(nb_shared, str) else nb_shared
    rc = L.skx_ref_neighbours(ref, species, first, count, top_k, _p(idx), _p(val), _p(codes))
    return rc, L.skx_last_error().decode()


def test_symbols_are_exported_and_bound():
    L = _lib.load()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    assert "skx_ref_neighbours" in {n for n, _, _ in _lib.SYMBOLS}
    assert hasattr(L, "skx_ref_neighbours")
    assert re.search(r"\bT skx_ref_neighbours\b", out)
    from sketchy_amd import api
    assert callable(api.ReferenceSketch.neighbours)


def test_argument_errors_come_before_the_device():
    rc, msg = _call(ref=None)
    assert rc == _lib.ERR_INVALID and "NULL" in msg, (rc, msg)
    for top in (0, _lib.MAX_TOP + 1):
        rc, msg = _call(ref=None, top_k=top)
        assert rc == _lib.ERR_INVALID and re.search(r"\btop_k\b", msg), (top, rc, msg)


def test_checks_that_need_a_reference_handle():
    """species, range, top_k per species, NULL outputs, codes without a table: SKX_ERR_INVALID naming the argument; count == 0: SKX_OK,
    nothing touched -- asserted only where a reference handle can be had (a device is present); without one nothing is asserted."""
    L = _lib.load()
    if L.skx_device_count() <= 0:
        return
    hashes = np.arange(1, 13, dtype=np.uint64).reshape(3, 4)
    h = C.c_void_p()
    _lib.check(L.skx_ref_create(C.byref(h), 0, 16, 0, 4, 4, 3, _p(hashes), _p(np.full(3, 4, np.uint32))))
    try:
        for kw, word in ((dict(species=1), "species"), (dict(first=3, count=1), "count"), (dict(first=1, count=3), "count"),
                         (dict(first=0xFFFFFFFF, count=2), "count"), (dict(top_k=3), "top_k"), (dict(nb_idx=None), "NULL"),
                         (dict(nb_shared=None), "NULL"), (dict(codes=np.zeros(64, np.uint32)), "genotype")):
            rc, msg = _call(ref=h, **kw)
            assert rc == _lib.ERR_INVALID and word in msg, (kw, rc, msg)
        untouched = np.full(64, 77, np.uint32)
        rc, msg = _call(ref=h, count=0, nb_idx=untouched)
        assert rc == _lib.OK and (untouched == 77).all(), (rc, msg)
        rc, msg = _call(ref=h, count=3, top_k=2)
        assert rc == _lib.OK, (rc, msg)
    finally:
        L.skx_ref_destroy(h)


class _FakeRef:
    """ReferenceSketch's fields without a handle: the wrapper must refuse bad ranges before it reaches the library."""
    n_species, species, n_genomes, s, _h, n_features = 2, [5, 3], 8, 4, None, 0


def test_wrapper_refuses_bad_ranges_before_the_library():
    from sketchy_amd import api
    fake = _FakeRef()
    for kw, word in ((dict(species=2), "species"), (dict(species=-1), "species"), (dict(first=6), "first"), (dict(first=2, count=4), "count"),
                     (dict(first=-1, count=1), "first"), (dict(top=0), "top"), (dict(top=5), "top"), (dict(species=1, top=3), "top"),
                     (dict(top=65), "top"), (dict(want_codes=True), "genotype")):
        with pytest.raises(ValueError, match=word):
            api.ReferenceSketch.neighbours(fake, **kw)


# ---- the host's own path under the sanitizers
@pytest.fixture(scope="module")
def asan_bin():
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "stub")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return BIN


def _run(*args):
    p = subprocess.run([BIN, *args], capture_output=True, env=ENV, timeout=120)
    return p.returncode, p.stdout.decode(), p.stderr.decode()


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    return nc.write_cli_files(tmp_path_factory.mktemp("neighbours_cli"))


def test_the_case_holds_what_it_should():
    names, hs, geno = nc.cli_genomes()
    counts = nc.cli_counts()
    assert len(hs) == 40 and len(hs[11]) == 0 and np.array_equal(hs[7], hs[23]) and counts[7, 23] == len(hs[7])
    assert len(hs[13]) < len(hs[2]) and counts[13, 2] == len(hs[13])   # a strict prefix: contained in whole
    idx, val = nc.loo_rows(counts, 5)
    assert idx[7, 0] == 23 and idx[23, 0] == 7 and (val[11] == 0).all() and list(idx[11]) == [0, 1, 2, 3, 4]
    assert (val[:, :-1] == val[:, 1:]).any()                            # ties inside the rows


def test_rows_against_the_oracle(asan_bin, files):
    msh, tsv = files
    for top in (1, 3, 39):
        rc, out, err = _run("neighbours", "-r", msh, "-t", str(top))
        assert rc == 0, err
        assert out == nc.expected_rows(top, False), top
        rc, out, err = _run("neighbours", "-r", msh, "-g", tsv, "-t", str(top), "-H")
        assert rc == 0, err
        assert out == "sketch_id\tneighbour_id\tshared_hashes\tmlst\tres\n" + nc.expected_rows(top, True), top
    rc, out, err = _run("neighbours", "-r", msh)   # TOP = 1
    assert rc == 0 and out == nc.expected_rows(1, False), err
    rc, out, err = _run("neighbours", "-r", msh, "-H")
    assert rc == 0 and out.startswith("sketch_id\tneighbour_id\tshared_hashes\n"), err


def test_consensus_lines_and_summary_against_the_oracle(asan_bin, files):
    msh, tsv = files
    for top in (1, 3, 5, 39):
        rc, out, err = _run("neighbours", "-r", msh, "-g", tsv, "-c", "-t", str(top))
        assert rc == 0, err
        assert out == nc.expected_consensus(top), top
    for top in (1, 2, 3, 8):
        for flag in ("-S", "--summary"):
            rc, out, err = _run("neighbours", "-r", msh, "-g", tsv, flag, "-t", str(top))
            assert rc == 0, err
            assert out == nc.expected_summary(top), top
    assert nc.expected_consensus(3) != nc.expected_consensus(1) and nc.expected_summary(3) != nc.expected_summary(1)


def test_command_line_errors_end_with_status_2(asan_bin, files):
    msh, tsv = files
    for args in (("-g", tsv, "-c", "-t", "2"), ("-c", "-t", "3"), ("-S", "-t", "3"), ("-t", "40"), ("-t", "41"), ("-g", tsv, "-t", "40"),
                 ("-t", "0")):
        rc, out, err = _run("neighbours", "-r", msh, *args)
        assert rc == 2 and out == "" and err.startswith("Error:"), (args, rc, err)
    rc, out, err = _run("neighbours", "-g", tsv)
    assert rc == 2 and out == "", (rc, err)
