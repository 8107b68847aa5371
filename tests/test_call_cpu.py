"""The species call on the CPU: call_cases.call_ref / call_changes_ref (numpy; what the GPU tests hold the device to) pinned against a
literal per-read loop on rows with planted ties; the argument checks of skx_stream_bind_call, skx_stream_bind_call_changes and
skx_call_rows that come before the device is touched, through the real library; and the host's `predict` with several -r against the
stub-linked sanitizer build of tests/test_host_cpu.py, whose library has none of the entry points."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from call_cases import call_changes_loop, call_changes_ref, call_loop, call_ref, planted_rows
from sketchy_amd import _lib, api
from test_host_cpu import _expected, _fastq, _reads, _reference, _run, asan_bin  # noqa: F401  (asan_bin: that module's stub-linked host)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("skx_stream_bind_call", "skx_stream_bind_call_changes", "skx_call_rows")


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


@pytest.mark.parametrize("n_sp,top,nf", [(1, 1, 0), (2, 1, 3), (3, 3, 0), (5, 4, 2), (64, 2, 1), (7, 17, 5)])
def test_call_ref_is_the_per_read_loop(n_sp, top, nf):
    idx, sums, codes = planted_rows(400, n_sp, top, n_feat=nf, seed=n_sp * 100 + top)
    got = call_ref(idx, sums, codes)
    sp, ci, cs, cc = call_loop(idx, sums, codes)
    assert got["call_species"].dtype == np.uint32 and got["call_idx"].dtype == np.uint32 and got["call_sum"].dtype == np.uint64
    assert got["call_species"].tolist() == sp and got["call_idx"].tolist() == ci and got["call_sum"].tolist() == cs
    assert (got["call_codes"] is None) == (nf == 0) and (nf == 0 or got["call_codes"].tolist() == cc)
    for part in ([got["call_idx"]] if nf == 0 else [got["call_idx"], got["call_codes"]]):
        ev = call_changes_ref(got["call_species"], part)
        assert ev.tolist() == call_changes_loop(got["call_species"], part)
        assert ev[0] == 0 and 1 < len(ev) < 400  # (runs of repeated reads: neither every read nor only the first)


def test_planted_rows_hold_the_cases_the_tie_rule_is_about():
    idx, sums, _ = planted_rows(400, 5, 3, seed=3)
    lead = sums[:, :, 0]
    at_max = (lead == lead.max(axis=1, keepdims=True)).sum(axis=1)
    assert {2, 3, 5} <= set(at_max.tolist())                      # equal leads in two, three and all species
    assert (lead.max(axis=1) == 0).any()                          # all-zero leads
    assert (lead.max(axis=1) == (1 << 54) - 1).any() and ((lead > 1 << 32).any(axis=1) & (lead < 1 << 32).any(axis=1)).any()
    sp = call_ref(idx, sums)["call_species"]
    assert (sp[lead.max(axis=1) == 0] == 0).all()                 # a table of zeros calls species 0
    assert (sp[at_max == 5] == 0).all()                           # all equal: the lowest
    assert (sp[lead[:, 4] == (1 << 54) - 1] == 4).all()           # one past 2^54 - 2, told apart in the LAST species
    # leads equal in their low words and different above bit 32: a 32-bit compare would call species 2 or 0 at random
    hi = (lead[:, 0] == (4 << 32)) & (lead[:, 2] == (4 << 32) + 1)
    assert hi.any() and (sp[hi] == 2).all()


def test_call_ref_small_cases_by_hand():
    idx = np.array([[[1, 2], [3, 4]], [[5, 6], [7, 8]], [[5, 6], [7, 8]], [[9, 9], [7, 8]]], np.uint32)
    sums = np.array([[[5, 1], [5, 4]], [[2, 2], [9, 0]], [[3, 2], [9, 0]], [[0, 0], [0, 0]]], np.uint64)
    got = call_ref(idx, sums)
    assert got["call_species"].tolist() == [0, 1, 1, 0]
    assert got["call_idx"].tolist() == [[1, 2], [7, 8], [7, 8], [9, 9]] and got["call_sum"].tolist() == [[5, 1], [9, 0], [9, 0], [0, 0]]
    assert call_changes_ref(got["call_species"], got["call_idx"]).tolist() == [0, 1, 3]
    same_rows = np.zeros((4, 2), np.uint32)  # the species alone changes
    assert call_changes_ref(np.array([0, 0, 1, 1]), same_rows).tolist() == [0, 2]
    assert call_changes_ref(np.zeros(0, np.uint32), np.zeros((0, 2), np.uint32)).tolist() == []


def test_symbols_are_declared_exported_and_bound():
    L = _lib.load()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    header = open(os.path.join(ROOT, "include", "sketchy_hip.h")).read()
    for name in NEW:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in {n for n, _, _ in _lib.SYMBOLS} and hasattr(L, name)
        assert re.search(r"\bT %s\b" % name, out)
    for attr in ("bind_call", "bind_call_changes"):
        assert hasattr(api.SumOfSharedHashes, attr)
    assert callable(api.call_rows)


def test_argument_errors_come_before_the_device():
    L = _lib.load()
    a32, a64 = np.zeros(64, np.uint32), np.zeros(64, np.uint64)
    # what stands for a stream where the check must come first: a zeroed block nobody may write to
    fake = np.zeros(1 << 16, np.uint8)

    def err():
        return L.skx_last_error().decode()

    assert L.skx_stream_bind_call(None, _p(a32), _p(a32), _p(a64), _p(a32)) == _lib.ERR_INVALID and "skx_stream_bind_call" in err()
    assert L.skx_stream_bind_call(_p(fake), None, _p(a32), _p(a64), None) == _lib.ERR_INVALID and "NULL" in err()
    good = [8, _p(a32), _p(a32), _p(a32), _p(a32), _p(a64), None]
    assert L.skx_stream_bind_call_changes(None, *good) == _lib.ERR_INVALID and "skx_stream_bind_call_changes" in err()
    for i in (1, 2, 3):  # n_events, ev_read, ev_species
        bad = list(good)
        bad[i] = None
        assert L.skx_stream_bind_call_changes(_p(fake), *bad) == _lib.ERR_INVALID and "NULL" in err(), i
    assert L.skx_stream_bind_call_changes(_p(fake), 0, *good[1:]) == _lib.ERR_INVALID and "cap" in err()
    assert not fake.any()

    idx, sums, codes = np.zeros((2, 2, 2), np.uint32), np.full((2, 2, 2), 3, np.uint64), np.zeros((2, 2, 2), np.uint32)
    sp, ci, cs, cc = np.full(2, 77, np.uint32), np.full((2, 2), 77, np.uint32), np.full((2, 2), 77, np.uint64), np.full((2, 2), 77, np.uint32)

    def call(idx_=idx, sums_=sums, codes_=None, n=2, n_sp=2, top=2, nf=0, sp_=sp, cc_=None):
        return L.skx_call_rows(0, _p(idx_), _p(sums_), _p(codes_), n, n_sp, top, nf, _p(sp_), _p(ci), _p(cs), _p(cc_))

    assert call(idx_=None) == _lib.ERR_INVALID and "NULL" in err()
    assert call(sums_=None) == _lib.ERR_INVALID and "NULL" in err()
    assert call(sp_=None) == _lib.ERR_INVALID and "NULL" in err()
    for bad in (0, _lib.MAX_SPECIES + 1):
        assert call(n_sp=bad) == _lib.ERR_INVALID and "n_species" in err(), bad
    for bad in (0, _lib.MAX_TOP + 1):
        assert call(top=bad) == _lib.ERR_INVALID and "top_k" in err(), bad
    assert call(codes_=codes, nf=2) == _lib.ERR_INVALID and "call_codes" in err()      # codes without call_codes
    assert call(cc_=cc, nf=2) == _lib.ERR_INVALID and "call_codes" in err()            # call_codes without codes
    for bad in (0, _lib.MAX_FEATURES + 1):
        assert call(codes_=codes, cc_=cc, nf=bad) == _lib.ERR_INVALID and "n_features" in err(), bad
    assert call(n=0) == _lib.OK and call(n=0, codes_=codes, cc_=cc, nf=2) == _lib.OK     # nothing to do: nothing is touched
    for a in (sp, ci, cs, cc):
        assert (a == 77).all()


# ---- the host: several -r
def _two_references(tmp_path):
    a, b = tmp_path / "a", tmp_path / "b"
    a.mkdir()
    b.mkdir()
    return _reference(a), _reference(b, n=11)


def test_cli_several_references_need_the_entry_points(asan_bin, tmp_path):  # noqa: F811
    """the stub library has neither skx_ref_create_multi nor the call: several -r end with a message that names what is missing and
    nothing on stdout, as `sketch --counts` does"""
    nm = subprocess.check_output(["nm", asan_bin], text=True)
    for name in ("skx_ref_create_multi",) + NEW:
        assert re.search(r"\bw %s\b" % name, nm), name  # weak and undefined
    (_, _, msh_a, tsv_a), (_, _, msh_b, tsv_b) = _two_references(tmp_path)
    fq = str(tmp_path / "r.fq")
    _fastq(fq, _reads(20, 30, 90))
    for extra in (("-s",), ("-s", "-c"), ("-s", "--changes"), ()):
        rc, out, err = _run("predict", "-r", msh_a, msh_b, "-g", tsv_a, tsv_b, "-i", fq, "-t", "3", *extra)
        assert rc not in (0, 98, 99) and rc < 128, (extra, rc, err)
        assert out == "" and re.search(r"skx_ref_create_multi|skx_stream_bind_call|skx_call_rows", err), (extra, err)


def test_cli_counts_of_references_and_tables_must_agree(asan_bin, tmp_path):  # noqa: F811
    (_, _, msh_a, tsv_a), (_, _, msh_b, tsv_b) = _two_references(tmp_path)
    fq = str(tmp_path / "r.fq")
    _fastq(fq, _reads(5, 30, 90))
    for args in (("-r", msh_a, msh_b, "-g", tsv_a), ("-r", msh_a, "-g", tsv_a, tsv_b), ("-g", tsv_a, "-r", msh_a, msh_b)):
        rc, out, err = _run("predict", *args, "-i", fq, "-s")
        assert rc == 2 and out == "" and "-g" in err and "-r" in err, (args, err)


def test_cli_one_reference_prints_what_it_printed(asan_bin, tmp_path):  # noqa: F811
    """one -r is the path it was: the text the stub's rows give (tests/test_host_cpu.py's own expectation), no species column, and
    the same bytes from the same command line again"""
    names, geno, msh, tsv = _reference(tmp_path)
    reads = _reads(200, 1, 300)
    fq = str(tmp_path / "r.fq")
    _fastq(fq, reads)
    header = "reads\tsketch_id\tshared_hashes\tmlst\tmeca"
    line = ("predict", "-r", msh, "-g", tsv, "-i", fq, "-s", "-t", "2", "-H", "-b", "16", "-j", "4")
    rc, out, err = _run(*line)
    assert rc == 0, err
    assert out == _expected(reads, names, geno, top=2, header=header)
    assert _run(*line) == (rc, out, err)
    rc, out, err = _run("predict", "-g", tsv, "-r", msh, "-i", fq, "-s")  # (the order of -g and -r does not matter)
    assert rc == 0 and out == _expected(reads, names, geno, top=1)
    rc, cons, err = _run(*[a if a != "2" else "3" for a in line], "-c")
    assert rc == 0 and cons.count("\n") == 201 and all(ln.split("\t")[1:3] == ["-", "-"] for ln in cons.splitlines()[1:])
    rc, off, err = _run("predict", "-r", msh, "-g", tsv, "-i", fq, "-t", "2")  # offline: one pooled sketch, two rows of reads, id, shared hashes, two columns
    assert rc == 0 and [len(ln.split("\t")) for ln in off.splitlines()] == [5, 5], err
