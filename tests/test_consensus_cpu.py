"""Consensus genotypes on the device (skx_ref_set_genotypes, skx_consensus_rows, skx_stream_bind_consensus): what can be checked
without a device.

* the four symbols are declared, exported and bound;
* argument errors that need no handle come back before the device is touched; those that need a reference handle are asserted only
  where one can be had (a device is present);
* api.encode_genotypes numbers every column's distinct strings in byte-wise sorted order;
* the host under AddressSanitizer + UndefinedBehaviorSanitizer against tests/stub, which has none of the new entry points: the weak
  references stay null and `predict -c` / `predict -s -c` vote over rows on the host, printing what they always printed."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from mshio import write_msh
from sketchy_amd import _lib, api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "stub", "sketchy-hip-asan")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=99", UBSAN_OPTIONS="halt_on_error=1:exitcode=98")
NEW = ("skx_ref_set_genotypes", "skx_ref_n_features", "skx_consensus_rows", "skx_stream_bind_consensus")


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def consensus_ref(idx, codes, species):
    """The issue's semantics, restated: idx [rows, n_species, top] local indices, codes [n_genomes, F] with the species one after
    the other -> [rows, n_species, F]: the most frequent code among a row's genomes per column, ties to the smallest code."""
    base = np.concatenate([[0], np.cumsum(species)])[:-1].astype(np.int64)
    got = np.sort(codes[idx.astype(np.int64) + base[None, :, None]], axis=2)  # [rows, species, top, F], ascending per column
    top = got.shape[2]
    pos = np.arange(top)[None, None, :, None]
    new = np.ones(got.shape, bool)
    new[:, :, 1:] = got[:, :, 1:] != got[:, :, :-1]                        # a run of equal codes begins here ...
    last = np.ones(got.shape, bool)
    last[:, :, :-1] = new[:, :, 1:]                                        # ... and ends here
    first_pos = np.maximum.accumulate(np.where(new, pos, 0), axis=2)
    last_pos = np.flip(np.minimum.accumulate(np.flip(np.where(last, pos, top), 2), axis=2), 2)
    j = np.argmax(last_pos - first_pos, axis=2)                            # the longest run; of several, the first = smallest code
    return np.take_along_axis(got, j[:, :, None, :], axis=2)[:, :, 0, :]


def test_the_restatement_itself():
    codes = np.array([[5, 0], [3, 0], [5, 1], [3, 1], [9, 0xFFFFFFFF]], np.uint32)
    idx = np.array([[[0, 1, 2]], [[0, 1, 4]], [[4, 4, 3]], [[0, 3, 4]]], np.uint32)
    want = np.array([[[5, 0]], [[3, 0]], [[9, 0xFFFFFFFF]], [[3, 0]]], np.uint32)
    got = consensus_ref(idx, codes, [5])
    assert got.dtype == np.uint32 and np.array_equal(got, want)
    # ... and against the definition read out literally, on random rows of two species
    rng = np.random.default_rng(5)
    species, codes = [7, 4], rng.integers(0, 3, (11, 3)).astype(np.uint32)
    for top in (1, 2, 4, 9):
        idx = np.stack([rng.integers(0, n, (50, top)) for n in species], axis=1).astype(np.uint32)
        got = consensus_ref(idx, codes, species)
        for r in range(50):
            for sp, g0 in enumerate((0, 7)):
                for f in range(3):
                    col = codes[g0 + idx[r, sp], f].tolist()
                    assert got[r, sp, f] == min(set(col), key=lambda v: (-col.count(v), v))


def test_symbols_are_declared_exported_and_bound():
    L = _lib.load()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    header = open(os.path.join(ROOT, "include", "sketchy_hip.h")).read()
    for name in NEW:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in {n for n, _, _ in _lib.SYMBOLS}
        assert hasattr(L, name)
        assert re.search(r"\bT %s\b" % name, out)
    assert re.search(r"#define SKX_MAX_FEATURES 64u", header) and _lib.MAX_FEATURES == 64
    for attr in ("set_genotypes", "n_features", "consensus_rows"):
        assert hasattr(api.ReferenceSketch, attr)
    assert callable(api.SumOfSharedHashes.consensus) and callable(api.encode_genotypes)


def test_argument_errors_come_before_the_device():
    L = _lib.load()
    codes, idx, out = np.zeros((3, 2), np.uint32), np.zeros((2, 1, 3), np.uint32), np.zeros((2, 1, 2), np.uint32)
    n = C.c_uint32(7)

    def err():
        return L.skx_last_error().decode()

    assert L.skx_ref_set_genotypes(None, 2, _p(codes)) == _lib.ERR_INVALID and "NULL" in err()
    assert L.skx_ref_n_features(None, C.byref(n)) == _lib.ERR_INVALID and n.value == 7
    assert L.skx_stream_bind_consensus(None, _p(out)) == _lib.ERR_INVALID and "NULL" in err()
    assert L.skx_consensus_rows(None, _p(idx), 2, 3, _p(out)) == _lib.ERR_INVALID and "NULL" in err()
    for top in (0, _lib.MAX_TOP + 1):
        assert L.skx_consensus_rows(None, _p(idx), 2, top, _p(out)) == _lib.ERR_INVALID and re.search(r"\btop_k\b", err()), top


def test_checks_that_need_a_reference_handle():
    """n_features out of range, NULL codes, a second table, no table, an index out of range, n_rows == 0 -- asserted only where a
    reference handle can be had (a device is present); without one nothing is asserted."""
    L = _lib.load()
    if L.skx_device_count() <= 0:
        return
    hashes = np.arange(1, 13, dtype=np.uint64).reshape(3, 4)
    h = C.c_void_p()
    _lib.check(L.skx_ref_create(C.byref(h), 0, 16, 0, 4, 4, 3, _p(hashes), _p(np.full(3, 4, np.uint32))))
    try:
        codes = np.array([[1, 9], [1, 8], [2, 8]], np.uint32)
        idx, out = np.array([[[0, 1, 2]]], np.uint32), np.full((1, 1, 2), 77, np.uint32)
        n = C.c_uint32(7)
        assert L.skx_ref_n_features(h, C.byref(n)) == _lib.OK and n.value == 0
        assert L.skx_consensus_rows(h, _p(idx), 1, 3, _p(out)) == _lib.ERR_INVALID and "genotype table" in L.skx_last_error().decode()
        for bad in (0, _lib.MAX_FEATURES + 1):
            assert L.skx_ref_set_genotypes(h, bad, _p(np.zeros((3, 65), np.uint32))) == _lib.ERR_INVALID
        assert L.skx_ref_set_genotypes(h, 2, None) == _lib.ERR_INVALID
        assert L.skx_ref_n_features(h, C.byref(n)) == _lib.OK and n.value == 0
        assert L.skx_ref_set_genotypes(h, 2, _p(codes)) == _lib.OK
        assert L.skx_ref_n_features(h, C.byref(n)) == _lib.OK and n.value == 2
        assert L.skx_ref_set_genotypes(h, 2, _p(codes)) == _lib.ERR_INVALID and "already" in L.skx_last_error().decode()
        for name in ("idx", "out"):
            a = dict(idx=_p(idx), out=_p(out))
            a[name] = None
            assert L.skx_consensus_rows(h, a["idx"], 1, 3, a["out"]) == _lib.ERR_INVALID
        assert L.skx_consensus_rows(h, _p(np.array([[[0, 3, 1]]], np.uint32)), 1, 3, _p(out)) == _lib.ERR_INVALID
        assert "index 3" in L.skx_last_error().decode()
        assert L.skx_consensus_rows(h, _p(idx), 0, 3, _p(out)) == _lib.OK and (out == 77).all()
        assert L.skx_consensus_rows(h, _p(idx), 1, 3, _p(out)) == _lib.OK and out.tolist() == [[[1, 8]]]
    finally:
        L.skx_ref_destroy(h)


def test_encode_genotypes_numbers_each_column_in_bytewise_sorted_order():
    rows = [["ST8", "b", "x"], ["ST30", "a", "x"], ["ST8", "B", "y"], ["st8", "a", "ST8"], ["ST239", "é", "x"]]
    codes, values = api.encode_genotypes(rows)
    assert codes.dtype == np.uint32 and codes.shape == (5, 3)
    # byte-wise: upper case before lower case, "ST239" < "ST30" < "ST8", a two-byte UTF-8 letter after all ASCII
    assert values[0] == ["ST239", "ST30", "ST8", "st8"]
    assert values[1] == ["B", "a", "b", "é"]
    assert values[2] == ["ST8", "x", "y"]
    assert codes[:, 0].tolist() == [2, 1, 2, 3, 0] and codes[:, 1].tolist() == [2, 1, 0, 1, 3]
    # the same string in different columns has unrelated codes
    assert codes[0, 0] == 2 and codes[3, 2] == 0
    # round trip, and order = sorted(bytes)
    for f in range(3):
        assert [values[f][c] for c in codes[:, f]] == [r[f] for r in rows]
        assert [v.encode() for v in values[f]] == sorted(v.encode() for v in set(r[f] for r in rows))
    with pytest.raises(ValueError, match="same number"):
        api.encode_genotypes([["a", "b"], ["a"]])
    codes, values = api.encode_genotypes([])
    assert codes.shape == (0, 0) and values == []


# ---- the host without the new entry points, under the sanitizers
@pytest.fixture(scope="module")
def asan_bin():
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "stub")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return BIN


def _run(*args):
    p = subprocess.run([BIN, *args], capture_output=True, env=ENV, timeout=120)
    return p.returncode, p.stdout.decode(), p.stderr.decode()


def consensus_of_rows(text, top):
    """`predict` rows (read, name, sum, columns ...) -> the consensus lines: majority per column over every `top` rows, ties to the
    smallest string (byte-wise)."""
    lines = [ln.split("\t") for ln in text.splitlines()]
    assert len(lines) % top == 0
    out = []
    for i in range(0, len(lines), top):
        grp = lines[i:i + top]
        assert len({g[0] for g in grp}) == 1
        call = []
        for j in range(3, len(grp[0])):
            col = [g[j].encode() for g in grp]
            call.append(min(set(col), key=lambda v: (-col.count(v), v)).decode())
        out.append("\t".join([grp[0][0], "-", "-"] + call) + "\n")
    return "".join(out)


def test_the_stub_host_keeps_its_consensus_output(asan_bin, tmp_path):
    nm = subprocess.check_output(["nm", BIN], text=True)
    for name in ("skx_ref_set_genotypes", "skx_consensus_rows", "skx_stream_bind_consensus"):
        assert re.search(r"\bw %s\b" % name, nm), name  # weak and undefined: the host takes its old route
    rng = np.random.default_rng(43)
    names = [f"genome{i:02d}.fa" for i in range(11)]
    hs = [np.sort(rng.choice(2 ** 40, size=12, replace=False).astype(np.uint64)) for _ in names]
    msh, tsv = str(tmp_path / "ref.msh"), str(tmp_path / "geno.tsv")
    write_msh(msh, names, hs, kmer=16, seed=0, lengths=[1000] * len(names))
    with open(tsv, "w") as f:
        f.write("id\tmlst\tmec\tpvl\n" + "".join(f"{n}\tST{i % 3}\t{'+-'[i % 2]}\tv{i}\n" for i, n in enumerate(names)))
    alpha = np.frombuffer(b"ACGT", np.uint8)
    files = []
    for j, n_reads in enumerate((150, 9)):
        path = str(tmp_path / f"sample{j}.fq")
        with open(path, "w") as f:
            for i in range(n_reads):
                r = alpha[rng.integers(0, 4, int(rng.integers(20, 200)))].tobytes().decode()
                f.write(f"@s{j}r{i}\n{r}\n+\n{'I' * len(r)}\n")
        files.append(path)
    for args in (("-s", "-i", files[0], "-b", "32"), ("-i", *files)):
        rc, rows, err = _run("predict", "-r", msh, "-g", tsv, "-t", "3", *args)
        assert rc == 0 and rows, err
        rc, cons, err = _run("predict", "-r", msh, "-g", tsv, "-t", "3", "-c", *args)
        assert rc == 0, err
        assert cons == consensus_of_rows(rows, 3), args
        assert cons.count("\n") == (150 if "-s" in args else 2)
