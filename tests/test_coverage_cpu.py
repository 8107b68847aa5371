"""Breadth of a stream, the parts that need no device: the expectation helper (tests/coverage_cases.py) against a literal loop, the
invariants covered <= col_len and covered <= table on the designs the GPU tests use, the conditions that keep those tests from being
vacuous, the error paths that are answered before the device is touched, and `screen` against a library without the entry points."""
import ctypes as C
import os
import subprocess

import numpy as np

import coverage_cases as cc
import hash_classes as hc
from helpers import pack_reads, unpack_reads
from mshio import write_msh
from oracle import oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_helper_against_a_literal_loop():
    """three genomes, five reads, s = 4: read by read the first four distinct hashes, a set, an intersection per column"""
    rng = np.random.default_rng(11)
    genome = bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), 400))
    reads = [genome[a:a + 60] for a in (0, 50, 100, 220, 330)]
    cols = [orc.py_sketch(genome[a:b], cc.K, cc.SEED, 40) for a, b in ((0, 200), (100, 400), (0, 400))]
    stride = max(len(c) for c in cols)
    ref = np.zeros((3, stride), np.uint64)
    for g, c in enumerate(cols):
        ref[g, :len(c)] = c
    col_len = np.array([len(c) for c in cols], np.uint32)
    bases, offsets = pack_reads(reads)
    got = cc.expected_coverage([ref], [col_len], bases, offsets, 4, (0, 1, 3, 5))
    seen = set()
    for r, seq in enumerate(reads):
        if r in got:
            assert got[r].tolist() == [len(set(c) & seen) for c in cols], r
        seen |= set(orc.py_sketch(seq, cc.K, cc.SEED, 4))
    assert got[5].tolist() == [len(set(c) & seen) for c in cols]
    assert got[0].tolist() == [0, 0, 0] and got[5].max() > 0
    # ... and truncation matters on the toy too: every 16-mer of the reads would cover more
    every = set()
    for seq in reads:
        every |= set(orc.py_sketch(seq, cc.K, cc.SEED, 10 ** 6))
    assert [len(set(c) & every) for c in cols] != got[5].tolist()


def test_expected_rank_breaks_ties_by_index():
    idx, val = cc.expected_rank(np.array([3, 5, 5, 0, 7, 7, 7], np.uint32), (4, 3), 3)
    assert idx.tolist() == [[1, 2, 0], [0, 1, 2]] and val.tolist() == [[5, 5, 3], [7, 7, 7]]


def test_truncated_expectation_on_the_single_species_design():
    """s = col_len[0] = 48: every read (285 k-mers) is truncated, and the expectation differs from the union of all k-mer hashes for
    every one of the 1 300 genomes; 23 distinct values, at most 28, ties at the fifth place.  covered <= col_len, covered <= table."""
    d, refs, col_lens, bases, offsets = cc.single(64)
    assert int(col_lens[0][0]) == 48 and d.n_genomes == 1300 and len(offsets) - 1 == 1200
    exp = cc.single_expected(64, None)
    cov = exp[1200]
    every = np.unique(np.concatenate([orc.kmer_hashes(seq, cc.K, cc.SEED)[0] for seq in unpack_reads(bases, offsets)]))
    valid = np.arange(refs[0].shape[1])[None, :] < col_lens[0][:, None]
    untruncated = (np.isin(refs[0], every) & valid).sum(axis=1)
    assert (untruncated != cov).all()
    assert len(np.unique(cov)) == 23 and int(cov.max()) == 28
    fifth = np.sort(cov)[::-1][4]
    assert (cov == fifth).sum() >= 2
    table = orc.stream(cc.K, cc.SEED, 48, refs[0], col_lens[0], bases, offsets, top_k=1)["cum"]
    for n in (500, 501, 1200):
        assert (exp[n] <= col_lens[0]).all()
    assert (cov <= table).all()
    assert (exp[500] <= exp[501]).all() and (exp[501] <= cov).all()
    # the variants of the design differ in their dense hashes only: each has its own expectation, same invariants
    for n_dense in (65, 900):
        e = cc.single_expected(n_dense, None)[1200]
        assert (e <= cc.single(n_dense)[2][0]).all() and e.max() > 0


def test_saturation_on_the_single_species_design():
    """s = 512 (no read has that many k-mers): full columns for 689 / 1 053 / 1 277 genomes after 100 / 500 / 1 200 reads"""
    d, refs, col_lens, bases, offsets = cc.single(64)
    exp = cc.single_expected(64, 512, (100, 500, 1200))
    assert [int((exp[n] == col_lens[0]).sum()) for n in (100, 500, 1200)] == [689, 1053, 1277]
    assert all((exp[n] <= col_lens[0]).all() for n in exp)


def test_ties_at_the_top_of_the_species_design():
    d = hc.species_design()
    refs, col_lens = hc.build_reference(d)
    bases, offsets = hc.reads(d, n_reads=600)
    s = int(col_lens[0][0])
    cov = cc.expected_coverage(refs, col_lens, bases, offsets, s, (600,))[600]
    assert (cov <= np.concatenate(col_lens)).all()
    table = np.concatenate([orc.stream(cc.K, cc.SEED, s, r, c, bases, offsets, top_k=1)["cum"] for r, c in zip(refs, col_lens)])
    assert (cov <= table).all()
    for sp, (a, n) in enumerate(zip((0, 70), (70, 600))):
        c = np.sort(cov[a:a + n])[::-1]
        assert c[2] == c[3], (sp, c[:6])   # top = 3 cuts through a tie in species 0 and 1: the lower index has to win
    assert np.sort(cov[:70])[::-1][0] == np.sort(cov[:70])[::-1][1]   # ... and so does top = 1 in species 0
    ff = d.members[hc.FF]
    assert len(ff) == 1 and cov[ff[0]] < np.concatenate(col_lens)[ff[0]]


def test_error_paths_that_need_no_device():
    """NULL arguments are answered with SKX_ERR_INVALID before any stream or device is looked at"""
    from sketchy_amd import _lib
    L = _lib.load()
    out = np.zeros(4, np.uint32)
    p = out.ctypes.data_as(C.c_void_p)
    assert L.skx_stream_enable_coverage(None) == _lib.ERR_INVALID
    assert L.skx_stream_coverage(None, p) == _lib.ERR_INVALID
    assert L.skx_stream_coverage_rows(None, p, 1, p) == _lib.ERR_INVALID
    assert L.skx_stream_coverage_rank(None, 1, p, p) == _lib.ERR_INVALID
    assert b"NULL" in L.skx_last_error()


def test_screen_against_a_library_without_the_entry_points(tmp_path):
    """the host references the coverage entry points weakly: against tests/stub `screen` ends with a message that names what is missing"""
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "stub")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    msh, fq = str(tmp_path / "ref.msh"), str(tmp_path / "reads.fq")
    write_msh(msh, ["a.fa", "b.fa"], [np.array([3, 9, 27], np.uint64), np.array([4, 9], np.uint64)], kmer=16, seed=0, lengths=[1000, 1000])
    with open(fq, "w") as f:
        f.write("@r0\nACGTACGTACGTACGTACGT\n+\nIIIIIIIIIIIIIIIIIIII\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=99", UBSAN_OPTIONS="halt_on_error=1:exitcode=98")
    p = subprocess.run([os.path.join(ROOT, "tests", "stub", "sketchy-hip-asan"), "screen", "-r", msh, "-i", fq], capture_output=True, text=True,
                       env=env, timeout=120)
    assert p.returncode == 1, (p.returncode, p.stderr)
    assert "skx_stream_enable_coverage" in p.stderr and p.stdout == ""
