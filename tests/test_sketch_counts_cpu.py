"""skx_sketch_groups_counts (pooled sketches with the abundance of every hash) and the counts32 list of `.msh` files: what can be
checked without a device -- the symbol is exported and bound, every argument check runs before the device is touched, both `.msh`
writers and readers agree about the list, the host refuses a list of the wrong length, and the host's counted merge
(formats.hpp::merge_counted) holds against a std::map reference under AddressSanitizer + UndefinedBehaviorSanitizer."""
import ctypes as C
import inspect
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import mshio as tests_mshio
from sketchy_amd import _lib
from sketchy_amd import mshio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ASAN_BIN = os.path.join(ROOT, "tests", "stub", "sketchy-hip-asan")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=99", UBSAN_OPTIONS="halt_on_error=1:exitcode=98")


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _call(k=16, seed=0, s=8, bases="ok", offsets="ok", n_records=3, group_first="ok", n_groups=2, sketches="ok", sketch_len="ok",
          valid="ok", counts="ok"):
    """One call with valid defaults (3 records in 2 groups); a keyword replaces one argument (None = NULL)."""
    L = _lib.load()
    d = dict(bases=np.frombuffer(b"ACGTACGTACGTACGTACGTACGTACGTAC", np.uint8).copy(), offsets=np.array([0, 10, 20, 30], np.uint64),
             group_first=np.array([0, 2, 3], np.uint32), sketches=np.zeros((max(n_groups, 1), max(s, 1)), np.uint64),
             sketch_len=np.zeros(max(n_groups, 1), np.uint32), valid=np.zeros(max(n_groups, 1), np.uint64),
             counts=np.full((max(n_groups, 1), max(s, 1)), 77, np.uint32))
    given = dict(bases=bases, offsets=offsets, group_first=group_first, sketches=sketches, sketch_len=sketch_len, valid=valid, counts=counts)
    a = {name: (d[name] if isinstance(v, str) else v) for name, v in given.items()}
    rc = L.skx_sketch_groups_counts(0, k, seed, s, _p(a["bases"]), _p(a["offsets"]), n_records, _p(a["group_first"]), n_groups,
                                    _p(a["sketches"]), _p(a["sketch_len"]), _p(a["valid"]), _p(a["counts"]))
    return rc, L.skx_last_error().decode(), a


def test_symbol_is_exported_and_bound():
    L = _lib.load()
    assert "skx_sketch_groups_counts" in {n for n, _, _ in _lib.SYMBOLS}
    assert hasattr(L, "skx_sketch_groups_counts")
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    assert re.search(r"\bT skx_sketch_groups_counts\b", out)
    assert re.search(r"\bT skx_sketch_groups\b", out)
    from sketchy_amd import api
    p = inspect.signature(api.sketch_groups).parameters
    assert "want_counts" in p and p["want_counts"].default is False


@pytest.mark.parametrize("kw, names", [
    (dict(offsets=None), "offsets"),
    (dict(group_first=None), "group_first"),
    (dict(sketches=None), "sketches"),
    (dict(sketch_len=None), "sketch_len"),
    (dict(counts=None), "counts"),
    (dict(bases=None), "bases"),
    (dict(k=0), "k"),
    (dict(k=_lib.MAX_K + 1), "k"),
    (dict(s=0), "s"),
    (dict(offsets=np.array([0, 20, 10, 30], np.uint64)), "offsets"),
    (dict(group_first=np.array([1, 2, 3], np.uint32)), "group_first"),      # does not start at 0
    (dict(group_first=np.array([0, 2, 2], np.uint32)), "group_first"),      # does not end at n_records
    (dict(group_first=np.array([0, 3, 2], np.uint32)), "group_first"),      # decreases
    (dict(group_first=np.array([0, 4, 3], np.uint32)), "group_first"),      # decreases, ends at n_records
])
def test_argument_errors_come_before_the_device(kw, names):
    rc, msg, _ = _call(**kw)
    assert rc == _lib.ERR_INVALID, (rc, msg)
    assert re.search(r"\b%s\b" % names, msg), msg
    assert "skx_sketch_groups_counts" in msg


def test_no_groups_is_ok_and_touches_nothing():
    rc, msg, a = _call(n_records=0, n_groups=0, offsets=np.array([0], np.uint64), group_first=np.array([0], np.uint32), bases=None)
    assert rc == _lib.OK, msg
    assert (a["counts"] == 77).all()
    rc, msg, _ = _call(n_records=0, n_groups=0, offsets=np.array([7], np.uint64), group_first=np.array([0], np.uint32), valid=None)
    assert rc == _lib.OK, msg


def test_valid_arguments_without_a_device():
    if _lib.load().skx_device_count() > 0:
        pytest.skip("a device is present")
    for kw in (dict(), dict(valid=None), dict(group_first=np.array([0, 0, 3], np.uint32))):
        rc, msg, _ = _call(**kw)
        assert rc == _lib.ERR_NO_DEVICE, (rc, msg)
        assert "no HIP device" in msg
    from sketchy_amd import api
    with pytest.raises(_lib.SketchyHipError) as e:
        api.sketch_groups(np.frombuffer(b"ACGTACGTAC", np.uint8), np.array([0, 10], np.uint64), np.array([0, 1], np.uint32), k=4, s=5,
                          want_counts=True)
    assert e.value.code == _lib.ERR_NO_DEVICE


# ---- counts32 in `.msh` files
def _collection(rng, n=5, s=40):
    names = [f"genome{i}.fa" for i in range(n)]
    lens = rng.integers(0, s + 1, n)
    lens[0], lens[1], lens[2] = s, 7, 0  # full, odd (half a word of counts), empty
    hashes = np.zeros((n, s), np.uint64)
    counts = np.zeros((n, s), np.uint32)
    for g in range(n):
        hashes[g, :lens[g]] = np.sort(rng.choice(2 ** 50, int(lens[g]), replace=False).astype(np.uint64))
        counts[g, :lens[g]] = rng.integers(1, 2 ** 32, int(lens[g]), dtype=np.uint64).astype(np.uint32)
    return names, hashes, counts, lens


def test_python_msh_round_trip(tmp_path):
    rng = np.random.default_rng(8)
    names, hashes, counts, lens = _collection(rng)
    path = str(tmp_path / "c.msh")
    mshio.write_msh(path, names, hashes, col_len=lens, kmer=21, seed=5, lengths=[1000 + g for g in range(len(names))], counts=counts)
    k, seed, recs = mshio.read_msh(path)
    assert (k, seed) == (21, 5) and [r["name"] for r in recs] == names
    for g, r in enumerate(recs):
        np.testing.assert_array_equal(r["hashes"], hashes[g, :lens[g]])
        np.testing.assert_array_equal(r["counts"], counts[g, :lens[g]])
        assert r["counts"].dtype == np.uint32 and r["hashes"].dtype == np.uint64
        assert r["length"] == 1000 + g and r["num_valid_kmers"] == 0
    # the tests' independent reader still finds the hashes of a file that carries counts
    k2, seed2, recs2 = tests_mshio.read_msh(path)
    assert (k2, seed2) == (21, 5)
    for g, r in enumerate(recs2):
        assert r["name"] == names[g]
        np.testing.assert_array_equal(np.asarray(r["hashes"], np.uint64), hashes[g, :lens[g]])
    # without counts: the same bytes as before the list existed in the writer's signature, and empty counts on the way back
    plain = str(tmp_path / "p.msh")
    mshio.write_msh(plain, names, hashes, col_len=lens, kmer=21, seed=5)
    _, _, precs = mshio.read_msh(plain)
    for g, r in enumerate(precs):
        assert len(r["counts"]) == 0 and r["counts"].dtype == np.uint32
        np.testing.assert_array_equal(r["hashes"], hashes[g, :lens[g]])
    # ... and a file of the tests' writer (another word order) reads the same through read_msh
    other = str(tmp_path / "t.msh")
    tests_mshio.write_msh(other, names, [hashes[g, :lens[g]] for g in range(len(names))], kmer=21, seed=5, lengths=[9] * len(names))
    _, _, orecs = mshio.read_msh(other)
    for g, r in enumerate(orecs):
        assert r["name"] == names[g] and r["length"] == 9 and len(r["counts"]) == 0
        np.testing.assert_array_equal(r["hashes"], hashes[g, :lens[g]])
    with pytest.raises(ValueError):
        mshio.write_msh(plain, names, hashes, counts=counts[:, :-1])


@pytest.fixture(scope="module")
def asan_bin():
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "stub")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return ASAN_BIN


def _host(*args):
    p = subprocess.run([ASAN_BIN, *args], capture_output=True, env=ENV, timeout=120)
    return p.returncode, p.stdout.decode(), p.stderr.decode()


def test_host_reader_checks_the_length_of_counts32(asan_bin, tmp_path):
    rng = np.random.default_rng(9)
    names, hashes, counts, lens = _collection(rng)
    good = str(tmp_path / "good.msh")
    mshio.write_msh(good, names, hashes, col_len=lens, kmer=16, seed=0, lengths=[500] * len(names), counts=counts)
    rc, out, err = _host("info", "-i", good)
    assert rc == 0, err
    assert out == "".join(f"{nm} 500 {int(n)}\n" for nm, n in zip(names, lens))
    # reference 1's counts32 one entry short: the list pointer is pointer 6 of element 1 of the reference table (words: root pointer,
    # 3 + 4 of the root struct, 1 of ReferenceList, the tag, then 3 + 7 words per reference)
    raw = bytearray(open(good, "rb").read())
    at = 8 + 8 * (1 + 3 + 4 + 1 + 1 + 1 * 10 + 3 + 6)
    ptr, = struct.unpack_from("<Q", raw, at)
    assert ptr & 3 == 1 and (ptr >> 32) & 7 == 4 and ptr >> 35 == lens[1]
    struct.pack_into("<Q", raw, at, ptr - (1 << 35))
    bad = str(tmp_path / "bad.msh")
    open(bad, "wb").write(bytes(raw))
    rc, out, err = _host("info", "-i", bad)
    assert rc == 1, (rc, err)
    assert "counts32" in err and names[1] in err and "AddressSanitizer" not in err and "runtime error" not in err


def test_host_counts_flag_needs_the_entry_point(asan_bin, tmp_path):
    """The stub library has no skx_sketch_groups_counts: `sketch --counts` must say so, not write a file without counts."""
    fa = str(tmp_path / "g.fa")
    open(fa, "w").write(">c\nACGTACGTACGTACGTACGTAAACCCGGGTTT\n")
    out = str(tmp_path / "o.msh")
    rc, so, err = _host("sketch", "-i", fa, "-o", out, "-s", "10", "--counts")
    assert rc == 1, (rc, err)
    assert "skx_sketch_groups_counts" in err and not os.path.exists(out)
    rc, so, err = _host("sketch", "-i", fa, "-o", out, "-s", "10")
    assert rc == 0, err
    _, _, recs = mshio.read_msh(out)
    assert len(recs) == 1 and recs[0]["name"] == "g.fa" and len(recs[0]["counts"]) == 0  # (the stub's sketcher returns no hashes)


def test_counted_merge_against_a_map_under_sanitizers(tmp_path):
    """tests/stub/merge_counted_check.cpp: a stand-alone program around formats.hpp::merge_counted, built here with
    -fsanitize=address,undefined and run once."""
    exe = str(tmp_path / "merge-counted-check")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "sketchy_amd", "host"), os.path.join(ROOT, "tests", "stub", "merge_counted_check.cpp"),
           "-o", exe, "-lz"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, env=ENV, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert re.search(r"\b0 failures\b", r.stdout), r.stdout
    assert int(r.stdout.split()[0]) > 4000
