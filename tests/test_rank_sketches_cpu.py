"""skx_rank_sketches / skx_predict_groups and offline `predict` over several inputs: what can be checked without a device.

* every argument check runs before the device is touched (include/sketchy_hip.h);
* the Python wrappers refuse malformed queries before they call into the library;
* the host under AddressSanitizer + UndefinedBehaviorSanitizer against tests/stub (which has no skx_rank_sketches: the host's
  fallback -- skx_common_hashes for all samples at once plus a stable sort per sample -- runs): `predict -i a b c` prints the
  three single-input outputs one after the other, `-s` with two inputs ends with exit status 2."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from mshio import write_msh
from sketchy_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "stub", "sketchy-hip-asan")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=99", UBSAN_OPTIONS="halt_on_error=1:exitcode=98")


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _rank(ref=None, query="ok", query_len="ok", n_query=2, q_stride=4, top_k=1, top_idx="ok", top_shared="ok", common=None):
    L = _lib.load()
    d = dict(query=np.array([[1, 2, 3, 4], [5, 6, 7, 8]], np.uint64), query_len=np.array([4, 3], np.uint32),
             top_idx=np.zeros((2, 1, 64), np.uint32), top_shared=np.zeros((2, 1, 64), np.uint32))
    given = dict(query=query, query_len=query_len, top_idx=top_idx, top_shared=top_shared)
    a = {name: (d[name] if isinstance(v, str) else v) for name, v in given.items()}
    rc = L.skx_rank_sketches(ref, _p(a["query"]), _p(a["query_len"]), n_query, q_stride, top_k, _p(a["top_idx"]), _p(a["top_shared"]),
                             _p(common))
    return rc, L.skx_last_error().decode()


def _predict(ref=None, n_records=1, n_groups=1, top_k=1, idx=None):
    L = _lib.load()
    bases = np.frombuffer(b"ACGTACGTACGTACGTACGT", np.uint8).copy()
    offsets, first = np.array([0, 20], np.uint64), np.array([0, n_records], np.uint32)
    idx, val = np.zeros(64, np.uint32) if idx is None else idx, np.zeros(64, np.uint32)
    rc = L.skx_predict_groups(ref, _p(bases), _p(offsets), n_records, _p(first), n_groups, top_k, _p(idx), _p(val), None, None, None)
    return rc, L.skx_last_error().decode()


def test_symbols_are_exported_and_bound():
    L = _lib.load()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    for name in ("skx_rank_sketches", "skx_predict_groups"):
        assert name in {n for n, _, _ in _lib.SYMBOLS}
        assert hasattr(L, name)
        assert re.search(r"\bT %s\b" % name, out)
    from sketchy_amd import api
    assert callable(api.ReferenceSketch.rank_sketches) and callable(api.ReferenceSketch.predict_groups)


def test_argument_errors_come_before_the_device():
    rc, msg = _rank(ref=None)
    assert rc == _lib.ERR_INVALID and "NULL" in msg, (rc, msg)
    for top in (0, _lib.MAX_TOP + 1):
        rc, msg = _rank(ref=None, top_k=top)
        assert rc == _lib.ERR_INVALID and re.search(r"\btop_k\b", msg), (top, rc, msg)
        rc, msg = _predict(ref=None, top_k=top)
        assert rc == _lib.ERR_INVALID and re.search(r"\btop_k\b", msg), (top, rc, msg)
    rc, msg = _predict(ref=None)
    assert rc == _lib.ERR_INVALID and "NULL" in msg, (rc, msg)


def test_checks_that_need_a_reference_handle():
    """An unsorted row is SKX_ERR_UNSORTED, top_k above the smallest species SKX_ERR_INVALID, no queries / no groups SKX_OK --
    asserted only where a reference handle can be had (a device is present); without one nothing is asserted."""
    L = _lib.load()
    if L.skx_device_count() <= 0:
        return
    hashes = np.arange(1, 13, dtype=np.uint64).reshape(3, 4)
    h = C.c_void_p()
    _lib.check(L.skx_ref_create(C.byref(h), 0, 16, 0, 4, 4, 3, _p(hashes), _p(np.full(3, 4, np.uint32))))
    try:
        rc, msg = _rank(ref=h, query=np.array([[1, 2, 3, 4], [5, 7, 6, 8]], np.uint64), query_len=np.array([4, 4], np.uint32))
        assert rc == _lib.ERR_UNSORTED, (rc, msg)
        rc, msg = _rank(ref=h, query=np.array([[1, 2, 3, 4], [5, 6, 8, 7]], np.uint64))  # (query_len 3: the row's first three are ascending)
        assert rc == _lib.OK, (rc, msg)
        rc, msg = _rank(ref=h, top_k=4)
        assert rc == _lib.ERR_INVALID and re.search(r"\btop_k\b", msg), (rc, msg)
        for name in ("query", "query_len", "top_idx", "top_shared"):
            rc, msg = _rank(ref=h, **{name: None})
            assert rc == _lib.ERR_INVALID and "NULL" in msg, (name, rc, msg)
        rc, msg = _rank(ref=h, query_len=np.array([4, 5], np.uint32))
        assert rc == _lib.ERR_INVALID and "q_stride" in msg, (rc, msg)
        untouched = np.full((2, 1, 64), 77, np.uint32)
        rc, msg = _rank(ref=h, n_query=0, top_idx=untouched)
        assert rc == _lib.OK and (untouched == 77).all(), (rc, msg)
        rc, msg = _predict(ref=h, n_groups=0)
        assert rc == _lib.ERR_INVALID and "group_first" in msg, (rc, msg)  # (one record, no group to hold it)
        untouched = np.full(64, 77, np.uint32)
        rc, msg = _predict(ref=h, n_records=0, n_groups=0, idx=untouched)
        assert rc == _lib.OK and (untouched == 77).all(), (rc, msg)
    finally:
        L.skx_ref_destroy(h)


class _FakeRef:
    """ReferenceSketch's fields without a handle: the wrappers must refuse bad shapes before they reach the library."""
    n_species, n_genomes, s, _h = 1, 3, 4, None


def test_wrappers_reject_malformed_queries_before_the_library():
    from sketchy_amd import api
    fake = _FakeRef()
    with pytest.raises(ValueError, match="n_query, stride"):
        api.ReferenceSketch.rank_sketches(fake, np.arange(8, dtype=np.uint64))
    with pytest.raises(ValueError, match="query_len"):
        api.ReferenceSketch.rank_sketches(fake, np.arange(8, dtype=np.uint64).reshape(2, 4), query_len=np.array([4, 4, 4], np.uint32))
    with pytest.raises(ValueError, match="query_len"):
        api.ReferenceSketch.rank_sketches(fake, np.arange(8, dtype=np.uint64).reshape(2, 4), query_len=np.array([[4, 4]], np.uint32))
    with pytest.raises(ValueError, match="group_first"):
        api.ReferenceSketch.predict_groups(fake, np.zeros(4, np.uint8), np.array([0, 4], np.uint64), np.zeros(0, np.uint32))


# ---- the host's fallback under the sanitizers
@pytest.fixture(scope="module")
def asan_bin():
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "stub")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return BIN


def _run(*args):
    p = subprocess.run([BIN, *args], capture_output=True, env=ENV, timeout=120)
    return p.returncode, p.stdout.decode(), p.stderr.decode()


@pytest.fixture(scope="module")
def samples(tmp_path_factory):
    d = tmp_path_factory.mktemp("rank_cli")
    rng = np.random.default_rng(41)
    names = [f"genome{i:02d}.fa" for i in range(9)]
    hs = [np.sort(rng.choice(2 ** 40, size=12, replace=False).astype(np.uint64)) for _ in names]
    msh, tsv = str(d / "ref.msh"), str(d / "geno.tsv")
    write_msh(msh, names, hs, kmer=16, seed=0, lengths=[1000] * len(names))
    with open(tsv, "w") as f:
        f.write("id\tmlst\n" + "".join(f"{nm}\tST{i % 4}\n" for i, nm in enumerate(names)))
    alpha = np.frombuffer(b"ACGT", np.uint8)
    files = []
    for j, n_reads in enumerate((37, 1, 12)):
        path = str(d / f"sample{j}.fq")
        with open(path, "w") as f:
            for i in range(n_reads):
                r = alpha[rng.integers(0, 4, int(rng.integers(20, 200)))].tobytes().decode()
                f.write(f"@s{j}r{i}\n{r}\n+\n{'I' * len(r)}\n")
        files.append(path)
    return msh, tsv, files, names


def test_offline_predict_over_three_inputs_is_the_three_runs_concatenated(asan_bin, samples):
    msh, tsv, files, names = samples
    for extra in (("-t", "3"), ("-t", "3", "-l", "5"), ("-c", "-t", "3"), ("-t", "2", "-b", "8")):
        singles = []
        for f in files:
            rc, out, err = _run("predict", "-r", msh, "-g", tsv, "-i", f, *extra)
            assert rc == 0 and out, err
            singles.append(out)
        rc, out, err = _run("predict", "-r", msh, "-g", tsv, "-i", *files, *extra)
        assert rc == 0, err
        assert out == "".join(singles), (extra, err)
        rc, out_h, err = _run("predict", "-r", msh, "-g", tsv, "-i", *files, *extra, "-H")
        assert rc == 0 and out_h == "reads\tsketch_id\tshared_hashes\tmlst\n" + out, err  # (the header once)
    # the `reads` column counts each file's own reads; the stub's counts are all 0: rows 0 .. top-1
    rc, out, err = _run("predict", "-r", msh, "-g", tsv, "-i", *files, "-t", "2")
    want = "".join(f"{n}\t{names[g]}\t0\tST{g % 4}\n" for n in (37, 1, 12) for g in (0, 1))
    assert rc == 0 and out == want, err


def test_streaming_predict_refuses_several_inputs(asan_bin, samples):
    msh, tsv, files, _ = samples
    for args in (("-s", "-i", files[0], files[1]), ("-i", files[0], files[1], "-s", "-t", "1")):
        rc, out, err = _run("predict", "-r", msh, "-g", tsv, *args)
        assert rc == 2 and out == "", (rc, err)
        assert err.startswith("Error:") and "one input" in err, err
    rc, out, err = _run("predict", "-r", msh, "-g", tsv, "-s", "-i", files[1])  # one input: as before
    assert rc == 0 and out.count("\n") == 1, err
