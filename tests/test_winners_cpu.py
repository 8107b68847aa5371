"""Winner-takes-all breadth, the parts that need no device: the expectation builder (tests/winner_cases.py) on hand-made tables, the
conditions that keep the GPU cases from being vacuous, the host's order and rank construction (sketchy_amd/csrc/skx_winner_order.hpp)
under sanitizers, the error paths answered before the device is touched, and `screen -w` against a library without the entry point."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import coverage_cases as cc
import hash_classes as hc
import winner_cases as wc
from mshio import write_msh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _table(cols):
    stride = max(1, max(len(c) for c in cols))
    ref = np.zeros((len(cols), stride), np.uint64)
    for g, c in enumerate(cols):
        ref[g, :len(c)] = sorted(c)
    return [ref], [np.array([len(c) for c in cols], np.uint32)]


def test_two_genomes_sharing_everything():
    """equal columns: equal containment, equal covered -- the lower index takes all"""
    w = wc.Winners(*_table([[3, 5, 9, 11], [3, 5, 9, 11]]), {3, 9, 11, 100})
    assert w.covered.tolist() == [3, 3] and w.won.tolist() == [3, 0] and w.order == [0, 1]
    assert w.winner == {3: 0, 9: 0, 11: 0}


def test_a_subset_against_its_superset_with_equal_containment():
    """genome 0 = {1, 2} seen {1}; genome 1 = {1, 2, 3, 4} seen {1, 3}: 1/2 == 2/4, the larger covered wins the shared hash although
    its index is the higher one"""
    w = wc.Winners(*_table([[1, 2], [1, 2, 3, 4]]), {1, 3})
    assert w.covered.tolist() == [1, 2] and w.order == [1, 0]
    assert w.won.tolist() == [0, 2] and w.winner == {1: 1, 3: 1}
    # ... and with a strictly larger containment the subset wins it
    w = wc.Winners(*_table([[1, 2], [1, 2, 3, 4, 5]]), {1, 3})
    assert w.order == [0, 1] and w.won.tolist() == [1, 1]


def test_disjoint_genomes_keep_everything():
    w = wc.Winners(*_table([[1, 2, 3], [4, 5], [6, 7, 8, 9]]), {1, 3, 4, 5, 9, 77})
    assert w.covered.tolist() == [2, 2, 1] and w.won.tolist() == w.covered.tolist()
    assert w.order == [1, 0, 2]


def test_an_empty_column():
    """col_len = 0 counts as 1: containment 0, behind everything that covers something, and no hash is ever its"""
    w = wc.Winners(*_table([[], [1, 2], []]), {1})
    assert w.covered.tolist() == [0, 1, 0] and w.won.tolist() == [0, 1, 0] and w.order == [1, 0, 2]
    w = wc.Winners(*_table([[], [1, 2]]), set())
    assert w.won.tolist() == [0, 0] and w.order == [0, 1] and w.n_seen == 0


def test_the_single_species_design_is_not_trivial():
    """64 dense, s = 48, 500 reads: 1 218 seen reference hashes, 546 genomes win something, 545 of them less than they cover, one
    everything; most of the order's neighbours are tied on (containment, covered) and decided by the index"""
    d, refs, col_lens, bases, offsets = cc.single(64)
    w = wc.single_expected(64, None)[500]
    np.testing.assert_array_equal(w.covered, cc.single_expected(64, None)[500])
    assert w.n_seen == 1218
    assert int((w.won > 0).sum()) == 546
    assert int(((w.won > 0) & (w.won < w.covered)).sum()) == 545
    assert int(((w.won == w.covered) & (w.covered > 0)).sum()) == 1
    cl = col_lens[0]
    tied = sum(1 for a, b in zip(w.order[:-1], w.order[1:])
               if int(w.covered[a]) == int(w.covered[b]) and int(w.covered[a]) * int(cl[b]) == int(w.covered[b]) * int(cl[a]))
    assert tied >= 1000, tied
    # the ranking by won differs from the ranking by covered
    assert wc.expected_rank(w.won, d.species, 5)[0].tolist() != cc.expected_rank(w.covered, d.species, 5)[0].tolist()


def test_the_species_design_has_hashes_held_by_two_species():
    """(70, 600, 3), 1 200 reads: 627 seen reference hashes, 243 genomes win something; seen hashes held by two species exist for every
    pair of species, and each is credited to exactly one genome"""
    d = hc.species_design()
    refs, col_lens = hc.build_reference(d)
    bases, offsets = hc.reads(d, n_reads=1200)
    w = wc.expected_winners(refs, col_lens, bases, offsets, int(col_lens[0][0]), (1200,))[1200]
    assert w.n_seen == 627 and int((w.won > 0).sum()) == 243
    assert int(((w.won > 0) & (w.won < w.covered)).sum()) == 242
    pairs = {}
    for h, g in w.winner.items():
        sp = sorted(set(int(x) for x in d.species_of(d.members[h])))
        for a in sp:
            for b in sp:
                if a < b:
                    pairs[a, b] = pairs.get((a, b), 0) + 1   # (a hash held by all three counts for every pair)
    assert pairs == {(0, 1): 9, (0, 2): 3, (1, 2): 3}


def test_order_under_sanitizers(tmp_path):
    """tests/stub/winner_order_check.cpp drives the header alone against a 128-bit brute force: built with address and undefined-behaviour
    sanitizers, run once"""
    exe = str(tmp_path / "winner-order-check")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "sketchy_amd", "csrc"), os.path.join(ROOT, "tests", "stub", "winner_order_check.cpp"),
           "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=99", UBSAN_OPTIONS="halt_on_error=1:exitcode=98")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert re.search(r"\b0 failures\b", r.stdout), r.stdout
    assert int(r.stdout.split()[0]) > 10000


def test_error_paths_that_need_no_device():
    """a NULL stream is answered with SKX_ERR_INVALID before any device is looked at"""
    from sketchy_amd import _lib
    L = _lib.load()
    out = np.zeros(4, np.uint32)
    p = out.ctypes.data_as(C.c_void_p)
    assert L.skx_stream_winners(None, p, p) == _lib.ERR_INVALID
    assert L.skx_stream_winners_rows(None, p, 1, p, p) == _lib.ERR_INVALID
    assert L.skx_stream_winners_rank(None, 1, p, p) == _lib.ERR_INVALID
    assert b"NULL" in L.skx_last_error()
    assert not out.any()


def test_screen_against_a_library_without_the_entry_point(tmp_path):
    """the host references skx_stream_winners weakly: against tests/stub `screen -w` is a usage error (status 2) that names it, before
    anything is read; plain `screen` ends as it did (status 1, naming skx_stream_enable_coverage)"""
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "stub")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    msh, fq = str(tmp_path / "ref.msh"), str(tmp_path / "reads.fq")
    write_msh(msh, ["a.fa", "b.fa"], [np.array([3, 9, 27], np.uint64), np.array([4, 9], np.uint64)], kmer=16, seed=0, lengths=[1000, 1000])
    with open(fq, "w") as f:
        f.write("@r0\nACGTACGTACGTACGTACGT\n+\nIIIIIIIIIIIIIIIIIIII\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=99", UBSAN_OPTIONS="halt_on_error=1:exitcode=98")
    exe = os.path.join(ROOT, "tests", "stub", "sketchy-hip-asan")
    for flag in ("-w", "--winner-take-all"):
        p = subprocess.run([exe, "screen", "-r", msh, "-i", fq, flag], capture_output=True, text=True, env=env, timeout=120)
        assert p.returncode == 2, (p.returncode, p.stderr)
        assert "skx_stream_winners" in p.stderr and p.stdout == ""
    p = subprocess.run([exe, "screen", "-r", msh, "-i", fq], capture_output=True, text=True, env=env, timeout=120)
    assert p.returncode == 1, (p.returncode, p.stderr)
    assert "skx_stream_enable_coverage" in p.stderr and "skx_stream_winners" not in p.stderr and p.stdout == ""
    p = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert p.returncode == 2 and "--winner-take-all" in p.stderr
