"""Composition of a stream on the device: every read pushed falls into one class -- a species, ambiguous, unclassified -- by its own
sketch's hits per species, against the oracle's expectation (tests/composition_cases.py; the conditions that keep these cases from
being vacuous: tests/test_composition_cpu.py).  Everything is integer and compared exactly.

The counts ride behind a pass's pair -> query index step, one thread per read of every batch of the pass, so every route by which a
stream's pass gets there and every forced variant of the pass has to leave the same counters, and a read without a pair -- a pass
without a dictionary -- must still be counted; the species masks are walked out of the tiled matrix once per reference."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import composition_cases as pc
import coverage_cases as cc
import hash_classes as hc
from helpers import exp_env, unpack_reads
from mshio import write_msh

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "sketchy_amd", "sketchy-hip")
R_ = hc.R_TEST


@pytest.fixture(scope="module")
def balanced_ref(gpu):
    d, refs, col_lens, bases, offsets, hits = pc.balanced()
    R, _, _ = cc.create_reference(d, R_, s=refs[0].shape[1])   # (the reference's own s)
    yield R
    R.close()


@functools.lru_cache(maxsize=None)
def _single_hits():
    d, refs, col_lens, bases, offsets = cc.single(64)
    hits = pc.read_hits(pc.species_masks(refs, col_lens), 1, bases, offsets, cc.S_SINGLE)
    hits.setflags(write=False)
    return hits


@pytest.mark.parametrize("min_hits", (1, 3))
def test_pushes(balanced_ref, min_hits):
    """the balanced design under rare_hash_genomes = R_TEST, synchronous pushes cut at (0, 250, 251, n), the query after every cut;
    rows and table are those of a stream that never enabled composition"""
    d, refs, col_lens, bases, offsets, hits = pc.balanced()
    cuts = (*pc.CUTS, len(offsets) - 1)
    assert balanced_ref.s == 507
    parts, table = pc.check_pushes(balanced_ref, bases, offsets, hits, min_hits, cuts)
    plain, plain_table = cc.plain_pushes(balanced_ref, bases, offsets, cuts)
    for a, b in zip(parts, plain):
        np.testing.assert_array_equal(a["topk_idx"], b["topk_idx"])
        np.testing.assert_array_equal(a["topk_sum"], b["topk_sum"])
    np.testing.assert_array_equal(table, plain_table)


def test_batches_that_share_passes(balanced_ref):
    """the same reads as twelve enqueue_device batches, queried after every fourth (the query flushes) and at the end"""
    d, refs, col_lens, bases, offsets, hits = pc.balanced()
    n = len(offsets) - 1
    S = pc.stream(balanced_ref, bases, 2 * n)
    try:
        S.enable_composition(1)
        edges = [int(x) for x in np.linspace(0, n, 13)]
        cc.enqueue_batches(S, bases, offsets, edges, query_after=(4, 8, 12),
                           on_query=lambda b: pc.check(S, pc.composition(hits, 1, 0, b), what=f"enqueued, {b} reads"))
        pc.check(S, pc.composition(hits, 1), what="enqueued, end")
        st = S.stats()
        assert st["passes_shared"] >= 1, st
    finally:
        S.close()


@pytest.mark.parametrize("packed", (False, True), ids=("ascii", "packed"))
def test_submit_and_packed_input(balanced_ref, packed):
    """page-locked batches through submit / drain, as ASCII and as 4-bit packed input"""
    from sketchy_amd import api
    d, refs, col_lens, bases, offsets, hits = pc.balanced()
    n = len(offsets) - 1
    data, off = api.pack_reads(bases, offsets, first_nibble=1) if packed else (np.ascontiguousarray(bases), np.ascontiguousarray(offsets))
    S = api.SumOfSharedHashes(balanced_ref, top=0, max_batch_reads=n, max_batch_bases=len(bases) + 2)
    keep = []
    try:
        S.enable_composition(3)
        if packed:
            S.set_packed_input(True)
        hb = api.HostBuffer(len(data))
        hb.view(np.uint8)[:] = data
        keep.append(hb)
        for a, b in ((0, 350), (350, 351), (351, 600), (600, n)):
            ho = api.HostBuffer((b - a + 1) * 8)
            ho.view(np.uint64)[:] = off[a:b + 1]
            keep.append(ho)
            S.submit(hb.ptr, ho.ptr, b - a)
        S.drain()
        pc.check(S, pc.composition(hits, 3), what=f"submit packed={packed}")
    finally:
        S.close()
        for h in keep:
            h.free()


@pytest.mark.parametrize("knobs", [{"SKX_STATIC_DENSE": 0}, {"SKX_PATTERNS": 0}, {"SKX_LONG_ROWS": 0}, {"SKX_RARE_DIRECT": 0}, {"SKX_PASS_READS": 64}],
                         ids=lambda k: "-".join(f"{a}={b}" for a, b in k.items()))
def test_forced_variants(gpu, knobs):
    """pushes and enqueued batches in a fresh child with the experiments build: per-pass dictionaries, no patterns, no bit rows, rare
    rows through M, passes of 64 reads"""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "composition_worker.py")], env=exp_env(**knobs), capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert out.stdout.rstrip().endswith("composition ok")


def test_edge_batches(balanced_ref):
    """only 15-base reads (no k-mer: a pass without a dictionary), a single read, a batch of reads that hit nothing"""
    d, refs, col_lens, bases, offsets, hits = pc.balanced()
    n = len(offsets) - 1
    n0, n1 = pc.N_DESIGN, pc.N_DESIGN + pc.N_OTHER
    S = pc.stream(balanced_ref, bases, n)
    try:
        S.enable_composition(1)
        zero = (np.zeros(5, np.uint64), np.zeros(3, np.uint64))
        pc.check(S, zero, what="before any read")
        S.push(bases, offsets[n1:n + 1])
        only_short = pc.composition(hits, 1, n1, n)
        assert int(only_short[0][-1]) == pc.N_SHORT == int(only_short[0].sum()) and not only_short[1].any()
        pc.check(S, only_short, what="reads without a k-mer")
        S.reset()
        S.push(bases, offsets[7:9])
        pc.check(S, pc.composition(hits, 1, 7, 8), what="a single read")
        S.reset()
        S.push(bases, offsets[n0:n1 + 1])
        nothing = pc.composition(hits, 1, n0, n1)
        assert int(nothing[0][-1]) == pc.N_OTHER and not nothing[1].any()
        pc.check(S, nothing, what="reads that hit nothing")
    finally:
        S.close()


@pytest.mark.parametrize("min_hits", (1, 36))
def test_single_species(gpu, min_hits):
    """one species needs no mask table: reads[0] = reads whose sketch holds at least min_hits reference hashes (the on-target reads),
    nobody is ambiguous"""
    d, refs, col_lens, bases, offsets = cc.single(64)
    hits = _single_hits()
    exp = pc.composition(hits, min_hits)
    assert int(exp[0][0]) == int((hits[:, 0] >= min_hits).sum()) and (min_hits == 1 or 200 < int(exp[0][0]) < 1000)
    R, _, _ = cc.create_reference(d, R_, s=cc.S_SINGLE)
    try:
        S = pc.stream(R, bases, 1200)
        try:
            S.enable_composition(min_hits)
            S.push(bases, offsets[:501])
            S.push(bases, offsets[500:])
            reads, pairs = S.composition()
            assert int(reads[1]) == 0 and int(reads[0] + reads[2]) == 1200
            pc.check(S, exp, what=f"single species min_hits={min_hits}")
        finally:
            S.close()
    finally:
        R.close()


def test_forty_species(gpu):
    """40 species of two genomes (the per-thread counters of more than 31 species take more of the LDS than a kernel gets unasked):
    the last species included, ties between neighbours"""
    from sketchy_amd import synth
    d = pc.many_species_design(40)
    refs, col_lens = hc.build_reference(d)
    bases, offsets = synth.make_reads(d.genome, 300, 40, err=0.02, rng_seed=21)
    s = refs[0].shape[1]
    hits = pc.read_hits(pc.species_masks(refs, col_lens), 40, bases, offsets, s)
    exp = pc.composition(hits, 1)
    assert int((exp[0][:40] > 0).sum()) >= 30 and int(exp[0][39]) > 0 and int(exp[0][40]) >= 5 and int(exp[0].sum()) == 300
    R, _, _ = cc.create_reference(d, R_, s=s)
    try:
        S = pc.stream(R, bases, 300)
        try:
            S.enable_composition(1)
            S.push(bases, offsets[:257])
            S.push(bases, offsets[256:])
            pc.check(S, exp, what="forty species")
        finally:
            S.close()
    finally:
        R.close()


def test_reads_of_genomes_64_to_127(balanced_ref):
    """a mask-dependent check on the real genomes 64..127 (64..69 are species 0, 70..127 species 1): reads made only of hashes those
    genomes hold, one 16-mer each.  No 64-genome group of the WALK straddles two species: a species is padded to whole 512-genome
    rank groups, species 1 starts at padded genome 512"""
    d, refs, col_lens, bases, offsets, _ = pc.balanced()
    wanted = {h for h, m in d.members.items() if ((m >= 64) & (m < 128)).any()}
    b, o = pc.reads_from_hashes(d.genome, wanted)
    hits = pc.read_hits(pc.species_masks(refs, col_lens), 3, b, o, balanced_ref.s)
    exp = pc.composition(hits, 1)
    assert min(int(exp[0][0]), int(exp[0][1]), int(exp[0][3])) >= 20 and int(exp[0][4]) == 0
    S = pc.stream(balanced_ref, b, len(o) - 1)
    try:
        S.enable_composition(1)
        S.push(b, o)
        pc.check(S, exp, what="boundary")
    finally:
        S.close()


def test_state(balanced_ref):
    """enable after the first read and a second enable with another min_hits are SKX_ERR_INVALID, min_hits = 0 too; the query without
    composition is SKX_ERR_INVALID; reset zeroes the counters and keeps composition enabled; table_add leaves them alone; two streams
    on one reference are independent"""
    from sketchy_amd import _lib
    d, refs, col_lens, bases, offsets, hits = pc.balanced()
    n = len(offsets) - 1
    A, B = pc.stream(balanced_ref, bases, n, top=1), pc.stream(balanced_ref, bases, n, top=1)
    try:
        for bad in (B.composition, lambda: B.enable_composition(0)):
            with pytest.raises(_lib.SketchyHipError) as e:
                bad()
            assert e.value.code == _lib.ERR_INVALID
        B.push(bases, offsets[:11])
        with pytest.raises(_lib.SketchyHipError) as e:
            B.enable_composition(1)
        assert e.value.code == _lib.ERR_INVALID
        B.reset()
        B.enable_composition(3)   # (after a reset the stream has taken no reads)
        with pytest.raises(_lib.SketchyHipError) as e:
            B.enable_composition(1)
        assert e.value.code == _lib.ERR_INVALID
        A.enable_composition(1)
        A.push(bases, offsets[:301])
        B.push(bases, offsets[300:302])
        pc.check(A, pc.composition(hits, 1, 0, 300), what="A")
        pc.check(B, pc.composition(hits, 3, 300, 301), what="B")
        table = A.table()
        A.table_add(np.ones(sum(pc.SIZES), np.uint64))
        pc.check(A, pc.composition(hits, 1, 0, 300), what="A after table_add")
        np.testing.assert_array_equal(A.table(), table + np.uint64(1))
        A.reset()
        pc.check(A, (np.zeros(5, np.uint64), np.zeros(3, np.uint64)), what="A after reset")
        A.push(bases, offsets[:n + 1])   # (composition is still enabled)
        pc.check(A, pc.composition(hits, 1), what="A after reset and a push")
        pc.check(B, pc.composition(hits, 3, 300, 301), what="B at the end")
    finally:
        A.close(); B.close()


def test_a_reference_without_the_index(gpu):
    """rare_hash_genomes = 0: enable_composition is SKX_ERR_UNSUPPORTED and the stream goes on working"""
    from sketchy_amd import _lib
    d, refs, col_lens, bases, offsets, hits = pc.balanced()
    n = len(offsets) - 1
    R, _, _ = cc.create_reference(d, 0, s=refs[0].shape[1])
    try:
        S = pc.stream(R, bases, n, top=1)
        try:
            with pytest.raises(_lib.SketchyHipError) as e:
                S.enable_composition(1)
            assert e.value.code == _lib.ERR_UNSUPPORTED
            got = S.push(bases, offsets)
            exp = hc.oracle_stream(refs, col_lens, bases, offsets, 1)
            np.testing.assert_array_equal(S.table(), np.concatenate([e_["cum"] for e_ in exp]))
            np.testing.assert_array_equal(got["topk_idx"].reshape(n, 3), np.concatenate([e_["topk_idx"] for e_ in exp], axis=1))
            with pytest.raises(_lib.SketchyHipError) as e:
                S.composition()
            assert e.value.code == _lib.ERR_INVALID
        finally:
            S.close()
    finally:
        R.close()


def test_beside_coverage_and_depth(balanced_ref):
    """coverage and depth enabled beside composition give what they give alone, and composition what it gives alone"""
    d, refs, col_lens, bases, offsets, hits = pc.balanced()
    n = len(offsets) - 1
    A, B = pc.stream(balanced_ref, bases, n), pc.stream(balanced_ref, bases, n)
    try:
        A.enable_depth()
        B.enable_composition(1)
        B.enable_depth()
        for S in (A, B):
            S.push(bases, offsets[:401])
            S.push(bases, offsets[400:])
        pc.check(B, pc.composition(hits, 1), what="beside depth")
        np.testing.assert_array_equal(A.coverage(), B.coverage())
        assert A.coverage().any()
        for a, b in zip(A.depth(), B.depth()):
            np.testing.assert_array_equal(a, b)
        np.testing.assert_array_equal(A.table(), B.table())
    finally:
        A.close(); B.close()


def test_cli(gpu, tmp_path):
    """`sketchy-hip composition` on the three species written as .msh files and the reads as FASTQ: the lines formatted from the
    oracle's expectation, with -m 3, with -l and with -H"""
    d, refs, col_lens, bases, offsets, hits = pc.balanced()
    n = len(offsets) - 1
    names, files = ("alpha", "beta", "gamma"), []
    for nm, ref, cl in zip(names, refs, col_lens):
        files.append(str(tmp_path / (nm + ".msh")))
        write_msh(files[-1], [f"{nm}{g:04d}.fa" for g in range(len(ref))], [ref[g, :cl[g]] for g in range(len(ref))], kmer=pc.K, seed=pc.SEED,
                  lengths=[3000] * len(ref))
    fq = str(tmp_path / "reads.fq")
    with open(fq, "w") as f:
        for i, r in enumerate(unpack_reads(bases, offsets)):
            f.write(f"@read{i}\n{r.decode()}\n+\n{'I' * len(r)}\n")

    def run(*args):
        p = subprocess.run([BIN, "composition", "-r", *files, "-i", fq, *args], capture_output=True, text=True)
        assert p.returncode == 0, p.stderr
        return p.stdout.split("\n")[:-1]
    assert int(col_lens[0][0]) >= 25   # (the host sketches the reads with the first sketch's size: no read of the design is truncated)
    h = hits
    one, three = pc.cli_lines(names, pc.composition(h, 1)), pc.cli_lines(names, pc.composition(h, 3))
    assert one != three
    assert run() == one
    assert run("-m", "3") == three
    assert run("-l", "300", "-H") == ["species\treads\tfraction\tpairs"] + pc.cli_lines(names, pc.composition(h, 1, 0, 300))
