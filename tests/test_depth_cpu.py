"""Depth of a stream, the parts that need no device: the expectation helper (tests/depth_cases.py) against a literal loop, the
conditions that keep the GPU tests (tests/test_gpu_depth.py) from being vacuous on the designs they use, the error paths answered before
the device is touched, and `screen --depth` against a library without the entry points."""
import ctypes as C
import os
import subprocess

import numpy as np

import coverage_cases as cc
import depth_cases as dc
import hash_classes as hc
from helpers import pack_reads
from mshio import write_msh
from oracle import oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_helper_against_a_literal_loop():
    """three genomes, six reads (one of them twice), s = 6: per column the list of counts, its lower median by hand"""
    rng = np.random.default_rng(11)
    genome = bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), 400))
    reads = [genome[a:a + 60] for a in (0, 50, 100, 220, 330, 50)]
    cols = [orc.py_sketch(genome[a:b], dc.K, dc.SEED, 40) for a, b in ((0, 200), (100, 400), (0, 400))]
    stride = max(len(c) for c in cols)
    ref = np.zeros((3, stride), np.uint64)
    for g, c in enumerate(cols):
        ref[g, :len(c)] = c
    col_len = np.array([len(c) for c in cols], np.uint32)
    bases, offsets = pack_reads(reads)
    got = dc.expected_depth([ref], [col_len], bases, offsets, 6, (0, 3, 6))
    assert all(not a.any() for a in got[0])
    for n in (3, 6):
        sketches = [orc.py_sketch(seq, dc.K, dc.SEED, 6) for seq in reads[:n]]
        for g, c in enumerate(cols):
            counts = sorted(v for v in (sum(h in sk for sk in sketches) for h in c) if v)
            assert got[n][0][g] == len(counts) and got[n][2][g] == sum(counts)
            assert got[n][1][g] == (counts[(len(counts) - 1) // 2] if counts else 0)
    five = dc.expected_depth([ref], [col_len], bases, offsets[:6], 6, (5,))[5]
    assert (got[6][2] >= five[2]).all() and got[6][2].sum() > five[2].sum()   # (the repeated read counts twice for depth ...)
    np.testing.assert_array_equal(got[6][0], cc.expected_coverage([ref], [col_len], bases, offsets, 6, (6,))[6])   # ... and once for breadth
    # the read counted once more through `twice` is the same as pushing it again
    again = dc.expected_depth([ref], [col_len], bases, offsets[:6], 6, (5,), twice=(1, 2))[5]
    for a, b in zip(again, got[6]):
        np.testing.assert_array_equal(a, b)


def test_the_lower_median_of_an_even_count():
    cov, med, tot = dc.summarise(np.array([[0, 7, 1, 0, 3, 9], [5, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0], [2, 2, 8, 8, 0, 0]]))
    assert cov.tolist() == [4, 1, 0, 4] and med.tolist() == [3, 5, 0, 2] and tot.tolist() == [20, 5, 0, 20]


def test_the_single_species_design_is_not_vacuous():
    """cc.single(64), s = 48, after 500 / 501 / 1200 reads: every genome covered, 19 / 19 / 41 distinct medians in 3..21 / 3..21 / 6..46,
    maximum depth 30 / 30 / 66, 642 / 642 / 660 genomes with an even covered (the lower-median rule matters), the median below the
    maximum everywhere; covered is the coverage tests' expectation and total the oracle's table"""
    d, refs, col_lens, bases, offsets = cc.single(64)
    exp, cnt = dc.single_expected(64), dc.single_counters(64)
    want = {500: (19, 3, 21, 30, 642, 171095), 501: (19, 3, 21, 30, 642, 171189), 1200: (41, 6, 46, 66, 660, 381487)}
    for n, (n_med, lo, hi, deepest, even, total) in want.items():
        cov, med, tot = exp[n]
        depth = dc.depth_matrix(refs, col_lens, cnt[n])
        assert (cov > 0).all()
        assert (len(np.unique(med)), int(med.min()), int(med.max())) == (n_med, lo, hi)
        assert int(depth.max()) == deepest and int((cov % 2 == 0).sum()) == even
        assert (med < depth.max(axis=1)).all()
        assert int(tot.sum()) == total
        np.testing.assert_array_equal(cov, cc.single_expected(64, None)[n])
    table = orc.stream(dc.K, dc.SEED, 48, refs[0], col_lens[0], bases, offsets, top_k=1)["cum"]
    np.testing.assert_array_equal(exp[1200][2], table)
    # reads 900..1199 once more: depth grows, breadth does not
    twice = dc.single_expected(64, None, (1200,), (900, 1200))[1200]
    np.testing.assert_array_equal(twice[0], exp[1200][0])
    assert (twice[2] >= exp[1200][2]).all() and int(twice[2].sum()) > 381487 and (twice[1] != exp[1200][1]).any()
    # the variants of the design have their own expectation, none of them flat
    for n_dense in (65, 900):
        assert len(np.unique(dc.single_expected(n_dense)[1200][1])) > 10
    # s = 512: no read is truncated -- 1 277 columns are covered in full (the coverage tests' figure); a genome has 40 to 113 covered
    # values where s = 48 leaves it 28 at the most, so the select's later ranks are asked for
    wide = dc.single_expected(64, 512, (1200,))[1200]
    assert int((wide[0] == col_lens[0]).sum()) == 1277 and int(exp[1200][0].max()) == 28
    assert (int(wide[0].min()), int(wide[0].max())) == (40, 113) and (int(wide[1].min()), int(wide[1].max())) == (40, 44)


def test_the_species_and_lifted_designs_are_not_vacuous():
    d = hc.species_design()
    refs, col_lens = hc.build_reference(d)
    bases, offsets = hc.reads(d, n_reads=600)
    exp = dc.expected_depth(refs, col_lens, bases, offsets, int(col_lens[0][0]), (250, 600))
    assert len(exp[600][1]) == 673
    assert [(len(np.unique(exp[n][1])), int(exp[n][1].max())) for n in (250, 600)] == [(16, 20), (38, 49)]
    d = hc.lifted_design(600, "both")
    refs, col_lens = hc.build_reference(d)
    bases, offsets = hc.reads(d, n_reads=300)
    cnt = dc.read_counters(bases, offsets, int(col_lens[0][0]), (300,))[300]
    depth = dc.depth_matrix(refs, col_lens, cnt)
    cov, med, tot = dc.summarise(depth)
    assert int((cov == 0).sum()) == 243 and not med[cov == 0].any()
    assert (int(med.min()), int(med.max())) == (0, 62) and int((med < depth.max(axis=1)).sum()) == 137
    assert hc.FE not in cnt and hc.FF not in cnt   # (no read hashes to a lifted value: those counters move through import only)
    assert len(d.members[hc.FE]) > 0 and len(d.members[hc.FF]) > 0


def test_error_paths_that_need_no_device():
    """NULL arguments are answered with SKX_ERR_INVALID before any stream or device is looked at"""
    from sketchy_amd import _lib
    L = _lib.load()
    out = np.zeros(4, np.uint64)
    p, n = out.ctypes.data_as(C.c_void_p), C.c_uint64(0)
    assert L.skx_stream_enable_depth(None) == _lib.ERR_INVALID
    assert L.skx_stream_depth(None, p, p, p) == _lib.ERR_INVALID
    assert L.skx_stream_depth_rows(None, p, 1, p, p, p) == _lib.ERR_INVALID
    assert L.skx_stream_depth_count(None, C.byref(n)) == _lib.ERR_INVALID
    assert L.skx_stream_depth_export(None, p, p, 1, C.byref(n)) == _lib.ERR_INVALID
    assert L.skx_stream_depth_import(None, p, p, 1, C.byref(n)) == _lib.ERR_INVALID
    assert b"NULL" in L.skx_last_error()


def test_screen_against_a_library_without_the_entry_points(tmp_path):
    """the host references the depth entry points weakly: against tests/stub `screen --depth` ends with status 2 and a message that
    names what is missing; without the flags `screen` answers what it answered before"""
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "stub")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    msh, fq = str(tmp_path / "ref.msh"), str(tmp_path / "reads.fq")
    write_msh(msh, ["a.fa", "b.fa"], [np.array([3, 9, 27], np.uint64), np.array([4, 9], np.uint64)], kmer=16, seed=0, lengths=[1000, 1000])
    with open(fq, "w") as f:
        f.write("@r0\nACGTACGTACGTACGTACGT\n+\nIIIIIIIIIIIIIIIIIIII\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=99", UBSAN_OPTIONS="halt_on_error=1:exitcode=98")

    def run(*args):
        return subprocess.run([os.path.join(ROOT, "tests", "stub", "sketchy-hip-asan"), "screen", "-r", msh, "-i", fq, *args], capture_output=True,
                              text=True, env=env, timeout=120)
    for flags in (("-d",), ("--depth",), ("-I", "-d", "-H")):
        p = run(*flags)
        assert p.returncode == 2, (flags, p.returncode, p.stderr)
        assert "skx_stream_enable_depth" in p.stderr and p.stdout == ""
    for flags in ((), ("-I",)):
        p = run(*flags)
        assert p.returncode == 1, (flags, p.returncode, p.stderr)
        assert "skx_stream_enable_coverage" in p.stderr and "depth" not in p.stderr and p.stdout == ""
