"""Composition of a stream, the parts that need no device: the conditions that keep the GPU cases (tests/test_gpu_composition.py) from
being vacuous, the expectation's own arithmetic on a hand-made case, the error paths that are answered before a device is looked at,
and the host's `composition` against a library without the entry points."""
import ctypes as C
import os
import subprocess

import numpy as np

import composition_cases as pc
import hash_classes as hc
from mshio import write_msh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_balanced_design_is_not_vacuous():
    """at the reference's own s = 507 every class holds at least 10 of the design's 600 reads at min_hits 1 and 3, the two values give
    different counts, and hc.species_design()'s reads would all have been species 1's; the 50 unrelated reads and the 5 reads without a
    k-mer are unclassified; the classes add up to the reads"""
    d, refs, col_lens, bases, offsets, hits = pc.balanced()
    n = len(offsets) - 1
    assert refs[0].shape[1] == 507 and n == pc.N_DESIGN + pc.N_OTHER + pc.N_SHORT
    one, three = pc.composition(hits, 1, 0, pc.N_DESIGN), pc.composition(hits, 3, 0, pc.N_DESIGN)
    assert one[0].tolist() == [146, 305, 49, 88, 12] and three[0].tolist() == [139, 299, 47, 74, 41]
    for reads, pairs in (one, three):
        assert int(reads.min()) >= 10 and int(reads.sum()) == pc.N_DESIGN and int(pairs.min()) > 0
    assert (one[0] != three[0]).all() and (one[1] == three[1]).all()
    for m in (1, 3):
        rest = pc.composition(hits, m, pc.N_DESIGN, n)
        assert rest[0].tolist() == [0, 0, 0, 0, pc.N_OTHER + pc.N_SHORT] and not rest[1].any()
        assert int(pc.composition(hits, m)[0].sum()) == n
    for a, b in zip(pc.CUTS, (*pc.CUTS[1:], n)):   # (the cuts of the GPU case add up too)
        assert int(pc.composition(hits, 1, a, b)[0].sum()) == b - a
    # the boundary set of the GPU case: reads of one hash each, held by genomes 64..127 -- species 0, species 1 and ties, nobody else
    wanted = {h for h, m in d.members.items() if ((m >= 64) & (m < 128)).any()}
    b, o = pc.reads_from_hashes(d.genome, wanted)
    edge = pc.composition(pc.read_hits(pc.species_masks(refs, col_lens), 3, b, o, 507), 1)[0]
    assert min(int(edge[0]), int(edge[1]), int(edge[3])) >= 20 and int(edge[2]) == 0 and int(edge[4]) == 0


def test_species_design_would_be_vacuous():
    d = hc.species_design()
    refs, col_lens = hc.build_reference(d)
    bases, offsets = hc.reads(d, n_reads=600)
    hits = pc.read_hits(pc.species_masks(refs, col_lens), 3, bases, offsets, refs[0].shape[1])
    for m in (1, 12):
        assert pc.composition(hits, m)[0].tolist() == [0, 600, 0, 0, 0]


def test_a_hand_made_case():
    """three species over six hashes: 10 and 20 are species 0's, 30 species 1's, 40 is held by species 0 AND 1, 50 by species 2, 60 by
    nobody (it lies behind its genome's col_len); 0xFF..FE is in a column and counts for nobody"""
    refs = [np.array([[10, 20, 40], [10, 40, 60]], np.uint64), np.array([[30, 40, hc.FE]], np.uint64), np.array([[50, 0, 0]], np.uint64)]
    col_lens = [np.array([3, 2], np.uint32), np.array([3], np.uint32), np.array([1], np.uint32)]
    masks = pc.species_masks(refs, col_lens)
    assert masks == {10: 1, 20: 1, 30: 2, 40: 3, 50: 4}
    hits = pc.sketch_hits(masks, 3, [[10, 40, 50], [20, 30], [50, 60, hc.FE]])
    assert hits.tolist() == [[2, 1, 1], [1, 1, 0], [0, 0, 1]]
    reads, pairs = pc.composition(hits, 1)
    assert reads.tolist() == [1, 0, 1, 1, 0] and pairs.tolist() == [3, 2, 2]   # (read 1: a two-way tie, nobody's)
    reads, pairs = pc.composition(hits, 2)
    assert reads.tolist() == [1, 0, 0, 0, 2] and pairs.tolist() == [3, 2, 2]   # (the tie at one hit is below min_hits: unclassified)
    assert pc.composition(pc.sketch_hits(masks, 3, [[]]), 1)[0].tolist() == [0, 0, 0, 0, 1]
    assert pc.cli_lines(("a", "b", "c"), pc.composition(hits, 1)) == \
        ["a\t1\t0.333333\t3", "b\t0\t0.000000\t2", "c\t1\t0.333333\t2", "ambiguous\t1\t0.333333\t-", "unclassified\t0\t0.000000\t-"]


def test_error_paths_that_need_no_device():
    """a NULL stream is answered with SKX_ERR_INVALID before any device is looked at"""
    from sketchy_amd import _lib
    L = _lib.load()
    out = np.zeros(4, np.uint64)
    p = out.ctypes.data_as(C.c_void_p)
    assert L.skx_stream_enable_composition(None, 1) == _lib.ERR_INVALID
    assert L.skx_stream_enable_composition(None, 0) == _lib.ERR_INVALID
    assert L.skx_stream_composition(None, p, p) == _lib.ERR_INVALID
    assert b"NULL" in L.skx_last_error()
    assert not out.any()


def test_composition_against_a_library_without_the_entry_points(tmp_path):
    """the host references both entry points weakly: against tests/stub `composition` is a usage error (status 2) that names the
    missing one, before anything is read"""
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "stub")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    a, b, fq = str(tmp_path / "a.msh"), str(tmp_path / "b.msh"), str(tmp_path / "reads.fq")
    write_msh(a, ["a.fa"], [np.array([3, 9, 27], np.uint64)], kmer=16, seed=0, lengths=[1000])
    write_msh(b, ["b.fa"], [np.array([4, 9], np.uint64)], kmer=16, seed=0, lengths=[1000])
    with open(fq, "w") as f:
        f.write("@r0\nACGTACGTACGTACGTACGT\n+\nIIIIIIIIIIIIIIIIIIII\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=99", UBSAN_OPTIONS="halt_on_error=1:exitcode=98")
    exe = os.path.join(ROOT, "tests", "stub", "sketchy-hip-asan")
    for args in (["-r", a, b, "-i", fq], ["-r", a, "-i", fq, "-m", "3", "-H"]):
        p = subprocess.run([exe, "composition", *args], capture_output=True, text=True, env=env, timeout=120)
        assert p.returncode == 2, (p.returncode, p.stderr)
        assert "skx_stream_enable_composition" in p.stderr and p.stdout == ""
    p = subprocess.run([exe, "composition", "-r", a, "-i", fq, "-m", "0"], capture_output=True, text=True, env=env, timeout=120)
    assert p.returncode == 2 and "-m" in p.stderr and p.stdout == ""
    p = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert p.returncode == 2 and "sketchy-hip composition" in p.stderr
