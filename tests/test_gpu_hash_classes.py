"""Every storage class of a reference hash, at its edges, against the oracle -- on references built from a designed membership
(tests/hash_classes.py; its invariants and the agreement of the design's counts with orc.common_hashes: tests/test_hash_classes_cpu.py).

skx_ref_create files a reference hash by the number of genomes that hold it and by the look of its list: postings (<= 8 genomes),
a bit row (9 .. R, R = policy rare_hash_genomes), a (pattern, <= 14 exceptions) record, a row of the static dense dictionary (> R), a
forced list (> R over several species), an exception (>= 0xFFFFFFFFFFFFFFFE).  Each class reaches the bit matrix, the gains and the
compact candidate ranking through kernels of its own; natural workloads of at most 1 024 genomes hold postings only.  Here one
reference of 1 300 genomes holds all of them -- lists of 8 | 9, R | R + 1, 63 | 64 | 65 genomes, lineages across a tile (256) and a
rank group (512) with 1 .. 16 exceptions of both kinds, 64 | 65 dense hashes (the static dictionary's tail from row 64 | 128) and more
dense hashes than a static dictionary takes -- and what the index reports is asserted against the design's own counts, so a
construction that missed a class fails.  Everything is integer and compared exactly."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import hash_classes as hc
from helpers import exp_env

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R_ = hc.R_TEST
VARIANTS = [(64, R_), (65, R_), (900, R_), (64, 0), (64, 1024)]   # (dense hashes of the design, rare_hash_genomes)


@functools.lru_cache(maxsize=None)
def _design(n_dense):
    d = hc.single_species(n_dense)
    names, q, qlen = hc.class_queries(d)
    counts = hc.design_counts(d, q, qlen)
    for a in (q, qlen, counts):
        a.setflags(write=False)
    return d, names, q, qlen, counts


@functools.lru_cache(maxsize=None)
def _reads(n_dense):
    return hc.reads(_design(n_dense)[0])


@functools.lru_cache(maxsize=None)
def _stream_oracle(n_dense, top):
    refs, col_lens = hc.build_reference(_design(n_dense)[0])
    return hc.oracle_stream(refs, col_lens, *_reads(n_dense), top)


@pytest.mark.parametrize("n_dense,rare", VARIANTS)
def test_whole_sketch_operators(gpu, n_dense, rare):
    """common_hashes and rank_sketches (top 1, 5, 64; rows and counts) for one query per class, the lineages' hashes, mixed queries,
    genomes' own columns, hashes nobody holds and an empty query -- with 64 and 65 dense hashes, with more than the static dictionary
    takes (per-pass dictionaries, index kept), without the index, and under the default policy (only the hashes of N - 1 and N genomes
    dense).  The index figures are the design's."""
    d, names, q, qlen, counts = _design(n_dense)
    R, _, _ = hc.create_reference(d, rare)
    try:
        hc.assert_index(R, d, rare)
        hc.check_operators(R, d.species, q, qlen, counts, (1, 5, 64), what=f"dense={n_dense} rare={rare}")
    finally:
        R.close()


def test_whole_sketch_operators_with_a_row_policy(gpu):
    """stream_query_rows small: the policy bounds the passes of a stream (test_a_push_cut_into_several_passes); the whole-sketch
    operators size their matrices from the queries themselves and must give the same counts with it set.  (Their queries are really
    cut into several passes by the experiments build's SKX_PASS_READS: test_forced_variants.)"""
    from sketchy_amd import api
    d, names, q, qlen, counts = _design(65)
    R, _, _ = hc.create_reference(d, R_)
    try:
        api.set_option("stream_query_rows", 64)
        try:
            hc.check_operators(R, d.species, q, qlen, counts, (5,), what="stream_query_rows=64")
        finally:
            api.set_option("stream_query_rows", 0)
    finally:
        R.close()


@pytest.mark.parametrize("n_dense,rare,top", [(64, R_, 1), (64, R_, 3), (65, R_, 3), (900, R_, 1), (64, 0, 3), (64, 1024, 1)])
def test_stream_pushes(gpu, n_dense, rare, top):
    """1 200 reads of 300 bases from the design's genome through synchronous pushes: rows, per-read counts for every genome and the table"""
    d = _design(n_dense)[0]
    bases, offsets = _reads(n_dense)
    n = len(offsets) - 1
    R, _, _ = hc.create_reference(d, rare)
    try:
        st = hc.check_pushes(R, _stream_oracle(n_dense, top), bases, offsets, top, [0, 500, 501, n], what=f"dense={n_dense} rare={rare}")
        print("stats:", st)
    finally:
        R.close()


@pytest.mark.parametrize("n_dense,rare,top", [(64, R_, 1), (64, R_, 3), (65, R_, 1), (900, R_, 3), (64, 0, 1), (64, 1024, 3)])
def test_stream_batches_that_share_passes(gpu, n_dense, rare, top):
    """the same reads as twelve device batches through enqueue_device: groups of batches share a pass.  The first pass of a stream
    ranks on every genome (on a table of zeros all 1 300 are candidates); on the 64-dense reference the batches of the later passes are
    ranked on their candidates (compact problems with pattern rows)"""
    d = _design(n_dense)[0]
    bases, offsets = _reads(n_dense)
    n = len(offsets) - 1
    R, _, _ = hc.create_reference(d, rare)
    try:
        st = hc.check_enqueued(R, _stream_oracle(n_dense, top), bases, offsets, top, list(range(0, n + 1, 100)), what=f"dense={n_dense} rare={rare}")
        print("stats:", st)
        assert st["passes_shared"] >= 1, st
        if (n_dense, rare) == (64, R_):
            assert R.patterns["pattern_lists"] > 0 and st["batches_compact"] >= 1, st
    finally:
        R.close()


def test_a_push_cut_into_several_passes(gpu):
    """stream_query_rows = 512: a push of 1 200 reads holds more distinct hashes than a pass has rows beside the static dictionary's"""
    from sketchy_amd import api
    d = _design(65)[0]
    bases, offsets = _reads(65)
    n = len(offsets) - 1
    R, _, _ = hc.create_reference(d, R_)
    try:
        api.set_option("stream_query_rows", 512)
        try:
            st = hc.check_pushes(R, _stream_oracle(65, 3), bases, offsets, 3, [0, n], what="stream_query_rows=512")
        finally:
            api.set_option("stream_query_rows", 0)
        assert st["last_passes"] > 1, st
    finally:
        R.close()


@pytest.mark.parametrize("rare", (R_, 0))
def test_several_species(gpu, rare):
    """(70, 600, 3) genomes: hashes of 30 + 71 genomes of two species (more than R in all: a list anyway) and of every genome of every
    species, hashes of 200 genomes of species 1 alone (dense, in that species' segment of the static dictionary), lists inside each
    species and 0xFF..FF in the last genome of the last species, whose padded index (1 538) is far from its real one (672)."""
    d = hc.species_design()
    R, refs, col_lens = hc.create_reference(d, rare)
    try:
        fig = hc.assert_index(R, d, rare)
        assert fig["static_dense"][0] == (rare != 0)
        names, q, qlen = hc.class_queries(d)
        counts = hc.oracle_counts(refs, col_lens, q, qlen)
        assert counts[names.index("lifted_ff")].tolist() == [0] * 672 + [1]
        hc.check_operators(R, d.species, q, qlen, counts, (1, 3), what=f"species rare={rare}")
        bases, offsets = hc.reads(d, n_reads=600)
        exp = hc.oracle_stream(refs, col_lens, bases, offsets, 2)
        assert all(e["shared"].max() > 0 for e in exp)
        hc.check_pushes(R, exp, bases, offsets, 2, [0, 250, 600], what=f"species rare={rare}")
        st = hc.check_enqueued(R, exp, bases, offsets, 2, [0, 150, 300, 450, 600], what=f"species rare={rare} enqueued")
        assert st["passes_shared"] >= 1, st
    finally:
        R.close()


@pytest.mark.parametrize("rare", (R_, 0))
@pytest.mark.parametrize("n_genomes", (600, 20))
@pytest.mark.parametrize("which", ("ff", "fe", "both"))
def test_lifted_hashes(gpu, which, n_genomes, rare):
    """References that hold only 0xFF..FF, only 0xFF..FE, or both (different genomes and a common one) -- 600 genomes (a dense segment
    in front of the static dictionary's tail; holders in three tiles and two rank groups) and 20 -- against queries that end in [FE],
    [FF], [FE, FF], [FD] and those values alone.  A lifted query hash that no genome holds counts for nobody.

    Before classify_a_kernel looked lifted query hashes up in the tail, reference "ff" with the default index mapped a query's FE onto
    the row of FF (lower_bound without the equality test): every holder of FF got 1 for the queries [.., FE] and [FE] (the oracle: 0)
    and 2 for [.., FE, FF] and [FE, FF] (the oracle: 1)."""
    d = hc.lifted_design(n_genomes, which)
    R, refs, col_lens = hc.create_reference(d, rare)
    try:
        hc.assert_index(R, d, rare)
        names, q, qlen = hc.lifted_queries(d)
        counts = hc.oracle_counts(refs, col_lens, q, qlen)
        assert counts[names.index("FE+FF")].max() == (2 if which == "both" else 1)
        hc.check_operators(R, d.species, q, qlen, counts, (1, 5, 20), what=f"lifted {which} n={n_genomes} rare={rare}")
    finally:
        R.close()


def _worker(**knobs):
    return subprocess.run([sys.executable, os.path.join(ROOT, "tests", "hash_classes_worker.py")], env=exp_env(**knobs),
                          capture_output=True, text=True)


@pytest.mark.parametrize("knobs", [{"SKX_STATIC_DENSE": 0}, {"SKX_PATTERNS": 0}, {"SKX_LONG_ROWS": 0}, {"SKX_LONG_ROWS_T": 0},
                                   {"SKX_LONG_ROWS_T": 2}, {"SKX_RARE_DIRECT": 0}, {"SKX_CAND": 0}, {"SKX_PASS_READS": 64}],
                         ids=lambda k: "-".join(f"{a}={b}" for a, b in k.items()))
def test_forced_variants(gpu, knobs):
    """The operators and the stream on the 64-dense reference in a fresh child with the experiments build: per-pass dictionaries, no
    patterns, no bit rows, no / always transposed bit rows, rare rows through M, no compact ranking, and passes of 64 reads / queries."""
    out = _worker(**knobs)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert out.stdout.rstrip().endswith("hash classes ok")


def test_an_ablated_scan_is_noticed(gpu):
    """negative control: SKX_SCAN_ABLATE=1 (the scan writes no results back) must make the worker fail -- the dense classes of this
    reference really go through the scan, although nearly every hash of it has a list"""
    out = _worker(SKX_SCAN_ABLATE=1)
    assert out.returncode != 0, "the dense hashes never reached the scan:\n" + out.stdout[-2000:]
    assert "hash classes ok" not in out.stdout
    assert "AssertionError" in out.stderr, out.stderr[-3000:]     # (wrong numbers, not a fault)
