"""Depth of a stream on the device: depth[h] = reads so far whose bottom-s sketch holds reference hash h, and per genome covered, the
lower median of its covered hashes' depths and their total, against the oracle's expectation (tests/depth_cases.py; the conditions that
keep these cases from being vacuous: tests/test_depth_cpu.py).  Everything is integer and compared exactly.

The counts ride behind a pass's pair -> query index step (one lane per (read, hash) pair), so every route by which a stream's pass gets
there and every forced variant of the pass has to leave the same counters; the walk reads the tiled matrix like the coverage walk, the
select behind it has to find the right rank whatever the counters' width; export / import carry the counters by hash, which is the only
way to reach wide and saturated counters and the lifted ones."""
import functools
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

import coverage_cases as cc
import depth_cases as dc
import hash_classes as hc
from helpers import exp_env, unpack_reads
from mshio import write_msh

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "sketchy_amd", "sketchy-hip")
R_ = hc.R_TEST
NAMES = ("covered", "median", "total")


@functools.lru_cache(maxsize=None)
def _oracle_table(n_dense, s, n_reads):
    from oracle import oracle as orc
    d, refs, col_lens, bases, offsets = cc.single(n_dense)
    return orc.stream(cc.K, cc.SEED, s, refs[0], col_lens[0], bases, offsets[:n_reads + 1], top_k=1)


def _stream(R, bases, n=1200, top=1):
    from sketchy_amd import api
    return api.SumOfSharedHashes(R, top=top, max_batch_reads=n, max_batch_bases=max(1, len(bases)))


def _assert_depth(got, exp, what=""):
    for name, g, e in zip(NAMES, got, exp):
        np.testing.assert_array_equal(g, e, err_msg=f"{what} {name}")


@pytest.mark.parametrize("n_dense,rare", [(64, R_), (65, R_), (900, R_), (64, 1024)])
def test_storage_classes(gpu, n_dense, rare):
    """hc.single_species under four policies / dictionary shapes, s = 48, synchronous pushes cut at [0, 500, 501, n]: after every cut
    the whole table and a scattered list (tile and rank-group edges, the last genome, the lineage starts, one index twice); covered
    equals coverage(), total equals table().  Rows and table equal those of a stream that never enabled depth -- and the oracle's."""
    d, refs, col_lens, bases, offsets = cc.single(n_dense)
    exp = dc.single_expected(n_dense)
    R, _, _ = cc.create_reference(d, rare, s=cc.S_SINGLE)
    try:
        assert R.s == 48 and R.rare_index["keys"] > 0
        parts, table = dc.check_pushes(R, bases, offsets, cc.CUTS_1300, exp, cc.ROWS_1300, what=f"dense={n_dense} rare={rare}")
        plain, plain_table = cc.plain_pushes(R, bases, offsets, cc.CUTS_1300)
        for a, b in zip(parts, plain):
            np.testing.assert_array_equal(a["topk_idx"], b["topk_idx"])
            np.testing.assert_array_equal(a["topk_sum"], b["topk_sum"])
        np.testing.assert_array_equal(table, plain_table)
        o = _oracle_table(n_dense, 48, 1200)
        np.testing.assert_array_equal(table, o["cum"])
        np.testing.assert_array_equal(np.concatenate([p["topk_idx"] for p in parts]), o["topk_idx"])
    finally:
        R.close()


def test_batches_that_share_passes(gpu):
    """the reads as twelve enqueue_device batches; depth is queried after every fourth (the query flushes) and at the end"""
    d, refs, col_lens, bases, offsets = cc.single(64)
    exp = dc.single_expected(64, None, (400, 800, 1200))
    R, _, _ = cc.create_reference(d, R_, s=cc.S_SINGLE)
    try:
        S = _stream(R, bases, n=2400, top=0)
        try:
            S.enable_depth()
            cc.enqueue_batches(S, bases, offsets, list(range(0, 1201, 100)), query_after=(4, 8, 12),
                               on_query=lambda b: dc.check_queries(S, exp[b], cc.ROWS_1300, what=f"enqueued, {b} reads"))
            dc.check_queries(S, exp[1200], cc.ROWS_1300, what="enqueued, end")
            st = S.stats()
            assert st["passes_shared"] >= 1, st
            np.testing.assert_array_equal(S.table(), _oracle_table(64, 48, 1200)["cum"])
        finally:
            S.close()
    finally:
        R.close()


def test_a_push_cut_into_several_passes(gpu):
    """stream_query_rows = 512: one push of 1 200 reads takes several passes, every one of them counts; reads 900..1199 pushed once
    more count twice for depth and once for breadth"""
    from sketchy_amd import api
    d, refs, col_lens, bases, offsets = cc.single(65)
    exp = dc.single_expected(65)
    twice = dc.single_expected(65, None, (1200,), (900, 1200))[1200]
    R, _, _ = cc.create_reference(d, R_, s=cc.S_SINGLE)
    try:
        api.set_option("stream_query_rows", 512)
        try:
            S = _stream(R, bases)
        finally:
            api.set_option("stream_query_rows", 0)
        try:
            S.enable_depth()
            S.push(bases, offsets)
            assert S.stats()["last_passes"] > 1
            dc.check_queries(S, exp[1200], cc.ROWS_1300, what="stream_query_rows=512")
            S.push(bases, offsets[900:1201])
            dc.check_queries(S, twice, cc.ROWS_1300, what="reads 900..1199 twice")
            np.testing.assert_array_equal(twice[0], exp[1200][0])
        finally:
            S.close()
    finally:
        R.close()


@pytest.mark.parametrize("packed", (False, True), ids=("ascii", "packed"))
def test_submit_and_packed_input(gpu, packed):
    """page-locked batches through submit / drain, as ASCII and as 4-bit packed input; then a synchronous push of reads 900..1199"""
    from sketchy_amd import api
    d, refs, col_lens, bases, offsets = cc.single(64)
    exp = dc.single_expected(64)
    twice = dc.single_expected(64, None, (1200,), (900, 1200))[1200]
    data, off = api.pack_reads(bases, offsets, first_nibble=1) if packed else (np.ascontiguousarray(bases), np.ascontiguousarray(offsets))
    R, _, _ = cc.create_reference(d, R_, s=cc.S_SINGLE)
    try:
        S = api.SumOfSharedHashes(R, top=0, max_batch_reads=1200, max_batch_bases=len(bases) + 2)
        keep = []
        try:
            S.enable_depth()
            if packed:
                S.set_packed_input(True)
            hb = api.HostBuffer(len(data))
            hb.view(np.uint8)[:] = data
            keep.append(hb)
            for a, b in ((0, 350), (350, 351), (351, 900), (900, 1200)):
                ho = api.HostBuffer((b - a + 1) * 8)
                ho.view(np.uint64)[:] = off[a:b + 1]
                keep.append(ho)
                S.submit(hb.ptr, ho.ptr, b - a)
            S.drain()
            dc.check_queries(S, exp[1200], cc.ROWS_1300, what=f"submit packed={packed}")
            np.testing.assert_array_equal(S.table(), _oracle_table(64, 48, 1200)["cum"])
            S.push(data, off[900:1201])
            dc.check_queries(S, twice, cc.ROWS_1300, what=f"submit packed={packed}, reads 900..1199 twice")
        finally:
            S.close()
            for h in keep:
                h.free()
    finally:
        R.close()


@pytest.mark.parametrize("knobs", [{"SKX_STATIC_DENSE": 0}, {"SKX_PATTERNS": 0}, {"SKX_LONG_ROWS": 0}, {"SKX_RARE_DIRECT": 0}, {"SKX_PASS_READS": 64},
                                   {"SKX_DEPTH_SCRATCH": 3 * 50 * 256}],
                         ids=lambda k: "-".join(f"{a}={b}" for a, b in k.items()))
def test_forced_variants(gpu, knobs):
    """the 64-dense case, pushes, enqueued batches and a repeated push, in a fresh child with the experiments build: per-pass
    dictionaries, no patterns, no bit rows, rare rows through M, passes of 64 reads -- and a select scratch of three groups per launch
    (24 groups: eight chunks)"""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "depth_worker.py")], env=exp_env(**knobs), capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert out.stdout.rstrip().endswith("depth ok")


def test_several_species(gpu):
    """(70, 600, 3) genomes: the table in species order, scattered rows across the species' edges"""
    from sketchy_amd import _lib
    d = hc.species_design()
    R, refs, col_lens = cc.create_reference(d, R_)
    try:
        bases, offsets = hc.reads(d, n_reads=600)
        exp = dc.expected_depth(refs, col_lens, bases, offsets, R.s, (250, 600))
        S = _stream(R, bases, n=600, top=2)
        try:
            S.enable_depth()
            rows = np.array([0, 69, 70, 669, 670, 672, 71, 670], np.uint32)
            for a, b in ((0, 250), (250, 600)):
                S.push(bases, offsets[a:b + 1])
                dc.check_queries(S, exp[b], rows, what=f"species, {b} reads")
            with pytest.raises(_lib.SketchyHipError) as e:
                S.depth_rows([673])
            assert e.value.code == _lib.ERR_INVALID
            assert [len(a) for a in S.depth_rows([])] == [0, 0, 0]
        finally:
            S.close()
    finally:
        R.close()


@pytest.mark.parametrize("n_genomes,which", [(600, "both"), (20, "ff")])
def test_lifted_references(gpu, n_genomes, which):
    """references that hold 0xFF..FE / 0xFF..FF in some columns, 300 reads: the zero-covered genomes (243 of 600) report median 0, the
    walk never probes the padding"""
    d = hc.lifted_design(n_genomes, which)
    R, refs, col_lens = cc.create_reference(d, R_)
    try:
        bases, offsets = hc.reads(d, n_reads=300)
        exp = dc.expected_depth(refs, col_lens, bases, offsets, R.s, (300,))[300]
        if n_genomes == 600:
            assert int((exp[0] == 0).sum()) == 243 and not exp[1][exp[0] == 0].any()
        S = _stream(R, bases, n=300)
        try:
            S.enable_depth()
            S.push(bases, offsets)
            rows = np.array([0, 3, n_genomes // 2, n_genomes // 3, n_genomes - 2, n_genomes - 1, 3], np.uint32)
            dc.check_queries(S, exp, rows, what=f"lifted {which} n={n_genomes}")
        finally:
            S.close()
    finally:
        R.close()


def test_no_truncation(gpu):
    """s = 512 (the matrices widened to 512 columns): no read is truncated, a genome has 40 to 113 covered values"""
    d, refs, col_lens, bases, offsets = cc.single(64)
    at = (100, 500, 1200)
    exp = dc.single_expected(64, 512, at)
    R, _, _ = cc.create_reference(d, R_, s=512, pad_to=512)
    try:
        S = _stream(R, bases)
        try:
            S.enable_depth()
            for a, b in zip((0,) + at[:-1], at):
                S.push(bases, offsets[a:b + 1])
                dc.check_queries(S, exp[b], cc.ROWS_1300, what=f"s=512 after {b} reads")
        finally:
            S.close()
    finally:
        R.close()


def test_export_and_import(gpu):
    """export after 1 200 reads = the oracle's (hash, count) pairs of reference hashes; imported into a fresh stream on a SECOND
    reference built from the same arrays (its slot layout may differ) it gives the same depth(); the export of reads 0..499 plus reads
    500..1199 gives the 1 200-read numbers; an unknown hash is counted and changes nothing; duplicates add up"""
    d, refs, col_lens, bases, offsets = cc.single(64)
    exp, cnt = dc.single_expected(64), dc.single_counters(64)
    R, _, _ = cc.create_reference(d, R_, s=cc.S_SINGLE)
    R2, _, _ = cc.create_reference(d, R_, s=cc.S_SINGLE)
    try:
        A, B, C_, D = (_stream(r, bases) for r in (R, R2, R2, R))
        try:
            for s_ in (A, B, C_, D):
                s_.enable_depth()
            assert A.depth_count() == 0 and [len(a) for a in A.depth_export()] == [0, 0]
            A.push(bases, offsets[:501])
            h500, c500 = A.depth_export()
            order = np.argsort(h500)
            eh, ec = dc.reference_pairs(refs, col_lens, cnt[500])
            np.testing.assert_array_equal(h500[order], eh)
            np.testing.assert_array_equal(c500[order], ec)
            A.push(bases, offsets[500:1201])
            h, c = A.depth_export()
            assert h.dtype == np.uint64 and c.dtype == np.uint32
            order = np.argsort(h)
            eh, ec = dc.reference_pairs(refs, col_lens, cnt[1200])
            np.testing.assert_array_equal(h[order], eh)
            np.testing.assert_array_equal(c[order], ec)
            assert A.depth_count() == len(eh) > 0
            # a fresh stream on the second reference
            assert B.depth_import(h, c) == 0
            _assert_depth(B.depth(), exp[1200], "imported")
            np.testing.assert_array_equal(B.coverage(), exp[1200][0])
            assert not B.table().any()   # (the sums travel with table_add, not with the counters)
            # resume: the export of 500 reads, then the other 700
            assert C_.depth_import(h500, c500) == 0
            C_.push(bases, offsets[500:1201])
            dc.check_queries(C_, exp[1200], cc.ROWS_1300, what="resumed")
            # a hash no genome holds; then every entry split in two, one half listed twice, in one list
            held = set(int(x) for x in eh)
            stranger = next(x for x in range(12345, 20000) if x not in held)
            assert D.depth_import(np.array([stranger], np.uint64), np.array([9], np.uint32)) == 1
            assert D.depth_count() == 0 and not any(a.any() for a in D.depth())
            lo, hi = c // 3, c - 2 * (c // 3)
            n_unknown = D.depth_import(np.concatenate([h, h[::-1], np.array([stranger], np.uint64), h]),
                                       np.concatenate([lo, lo[::-1], np.array([1], np.uint32), hi]))
            assert n_unknown == 1
            _assert_depth(D.depth(), exp[1200], "duplicates")
            assert D.depth_count() == len(eh)
        finally:
            for s_ in (A, B, C_, D):
                s_.close()
    finally:
        R.close(); R2.close()


def test_wide_counters_and_saturation(gpu):
    """the exported counts scaled by 70 000 and by 40 000 000 (values past 2^16, 2^24 and 2^31: every byte round of the select), the
    latter imported twice (min(2 v, 2^32 - 1)), and a push on top that leaves the saturated counters where they are"""
    d, refs, col_lens, bases, offsets = cc.single(64)
    cnt = dc.single_counters(64)
    D1200, D500 = dc.depth_matrix(refs, col_lens, cnt[1200]), dc.depth_matrix(refs, col_lens, cnt[500])
    eh, ec = dc.reference_pairs(refs, col_lens, cnt[1200])
    assert int(ec.max()) == 66 and 2 ** 16 < 66 * 70_000 < 2 ** 24 < 40_000_000 and 2 ** 31 < 66 * 40_000_000 < 2 ** 32
    R, _, _ = cc.create_reference(d, R_, s=cc.S_SINGLE)
    try:
        for scale in (70_000, 40_000_000):
            S = _stream(R, bases)
            try:
                S.enable_depth()
                scaled = (ec.astype(np.uint64) * scale).astype(np.uint32)
                assert S.depth_import(eh, scaled) == 0
                exp = dc.summarise(D1200 * scale)
                assert int(exp[1].max()) == 46 * scale
                dc.check_queries(S, exp, cc.ROWS_1300, what=f"x{scale}")
                if scale == 40_000_000:
                    assert S.depth_import(eh, scaled) == 0
                    twice = np.minimum(2 * D1200 * scale, dc.U32_MAX)
                    assert (twice == dc.U32_MAX).any() and ((twice > 0) & (twice < dc.U32_MAX)).any()
                    dc.check_queries(S, dc.summarise(twice), cc.ROWS_1300, what="imported twice")
                    S.push(bases, offsets[:501])
                    dc.check_queries(S, dc.summarise(np.minimum(twice + D500, dc.U32_MAX)), cc.ROWS_1300, what="a push on saturated counters")
                    h, c = S.depth_export()
                    assert int(c.max()) == dc.U32_MAX
            finally:
                S.close()
    finally:
        R.close()


def test_lifted_counters(gpu):
    """hc.lifted_design(600, "both"), 300 reads, then (0xFF..FE, 5) and (0xFF..FF, 7) imported: exactly the holders of each value gain
    one in covered -- in depth() and in coverage() --, medians and totals follow the expectation with those values added"""
    d = hc.lifted_design(600, "both")
    R, refs, col_lens = cc.create_reference(d, R_)
    try:
        bases, offsets = hc.reads(d, n_reads=300)
        cnt = dc.read_counters(bases, offsets, R.s, (300,))[300]
        before = dc.summarise(dc.depth_matrix(refs, col_lens, cnt))
        cnt[hc.FE], cnt[hc.FF] = 5, 7
        after = dc.summarise(dc.depth_matrix(refs, col_lens, cnt))
        gain = np.zeros(600, np.uint32)
        for h in (hc.FE, hc.FF):
            gain[np.asarray(d.members[h], np.int64)] += 1
        assert gain.any() and (after[0] == before[0] + gain).all()
        assert (after[1] != before[1]).any() and int(after[2].sum() - before[2].sum()) == 5 * len(d.members[hc.FE]) + 7 * len(d.members[hc.FF])
        S = _stream(R, bases, n=300)
        try:
            S.enable_depth()
            S.push(bases, offsets)
            rows = np.array([0, 3, 300, 200, 598, 599, *d.members[hc.FE][:3], *d.members[hc.FF][:3]], np.uint32)
            dc.check_queries(S, before, rows, what="lifted, before the import")
            assert S.depth_import(np.array([hc.FE, hc.FF], np.uint64), np.array([5, 7], np.uint32)) == 0
            dc.check_queries(S, after, rows, what="lifted, after the import")
            h, c = S.depth_export()
            assert dict(zip(h.tolist(), c.tolist()))[hc.FE] == 5 and dict(zip(h.tolist(), c.tolist()))[hc.FF] == 7
        finally:
            S.close()
    finally:
        R.close()


def test_a_reference_without_the_index(gpu):
    """rare_hash_genomes = 0: enable_depth is SKX_ERR_UNSUPPORTED, the stream goes on working, everything else is SKX_ERR_INVALID"""
    from sketchy_amd import _lib
    d, refs, col_lens, bases, offsets = cc.single(64)
    R, _, _ = cc.create_reference(d, 0, s=cc.S_SINGLE)
    try:
        S = _stream(R, bases)
        try:
            with pytest.raises(_lib.SketchyHipError) as e:
                S.enable_depth()
            assert e.value.code == _lib.ERR_UNSUPPORTED
            got = S.push(bases, offsets)
            o = _oracle_table(64, 48, 1200)
            np.testing.assert_array_equal(got["topk_idx"], o["topk_idx"])
            np.testing.assert_array_equal(S.table(), o["cum"])
            one = (np.array([1], np.uint64), np.array([1], np.uint32))
            for q in (S.depth, lambda: S.depth_rows([0, 1]), S.depth_count, S.depth_export, lambda: S.depth_import(*one), S.coverage):
                with pytest.raises(_lib.SketchyHipError) as e:
                    q()
                assert e.value.code == _lib.ERR_INVALID
        finally:
            S.close()
    finally:
        R.close()


def test_state(gpu):
    """enable after reads is SKX_ERR_INVALID; queries, export and import without depth are SKX_ERR_INVALID (with coverage alone too);
    reset zeroes the counters and keeps depth enabled; two streams on one reference are independent; table_add moves neither the
    counters nor total"""
    from sketchy_amd import _lib
    d, refs, col_lens, bases, offsets = cc.single(64)
    exp = dc.single_expected(64)
    R, _, _ = cc.create_reference(d, R_, s=cc.S_SINGLE)
    try:
        A, B, C_ = (_stream(R, bases) for _ in range(3))
        try:
            C_.enable_coverage()
            one = (np.array([1], np.uint64), np.array([1], np.uint32))
            for q in (C_.depth, lambda: C_.depth_rows([0]), C_.depth_count, C_.depth_export, lambda: C_.depth_import(*one)):
                with pytest.raises(_lib.SketchyHipError) as e:
                    q()
                assert e.value.code == _lib.ERR_INVALID
            C_.push(bases, offsets[:11])
            with pytest.raises(_lib.SketchyHipError) as e:
                C_.enable_depth()
            assert e.value.code == _lib.ERR_INVALID
            C_.reset()
            C_.enable_depth()   # (after a reset the stream has taken no reads; coverage was on already)
            A.enable_depth()
            B.enable_depth()
            assert not any(a.any() for a in A.depth()) and not A.coverage().any()
            A.push(bases, offsets[:501])
            B.push(bases, offsets[500:502])
            _assert_depth(A.depth(), exp[500], "A")
            only = dc.expected_depth(refs, col_lens, bases[int(offsets[500]):int(offsets[501])], offsets[500:502] - offsets[500], 48, (1,))[1]
            _assert_depth(B.depth(), only, "B")
            assert not any(a.any() for a in C_.depth())
            A.table_add(np.ones(1300, np.uint64))
            _assert_depth(A.depth(), exp[500], "A after table_add")
            np.testing.assert_array_equal(A.table(), exp[500][2] + np.uint64(1))
            A.reset()
            assert not any(a.any() for a in A.depth()) and A.depth_count() == 0 and A.reads == 0
            A.push(bases, offsets[:502])   # (depth is still enabled)
            dc.check_queries(A, exp[501], cc.ROWS_1300, what="A after reset")
            _assert_depth(B.depth(), only, "B at the end")
        finally:
            A.close(); B.close(); C_.close()
    finally:
        R.close()


def test_interleaved_queries_on_one_stream(gpu):
    """the breadth and depth queries and the two rankings share their list and ranking scratch: long and short lists, whole tables and
    rankings of one and five rows alternate on ONE stream after the 1 200 reads, every answer against the oracle's"""
    d, refs, col_lens, bases, offsets = cc.single(64)
    exp = dc.single_expected(64)[1200]
    cov = cc.single_expected(64, None)[1200]
    cum = _oracle_table(64, 48, 1200)["cum"]
    by_sum = np.lexsort((np.arange(1300), -cum.astype(np.int64)))
    long_list = np.concatenate([np.arange(1300, dtype=np.uint32)[::-1], np.arange(0, 1300, 130, dtype=np.uint32)])
    perm = ((np.arange(1300, dtype=np.int64) * 577 + 13) % 1300).astype(np.uint32)   # (577 and 1300 are coprime)
    assert len(long_list) == 1310 and len(set(perm.tolist())) == 1300
    R, _, _ = cc.create_reference(d, R_, s=cc.S_SINGLE)
    try:
        S = _stream(R, bases, top=1)
        try:
            S.enable_depth()
            S.push(bases, offsets)

            def check_rank(top):
                idx, sm = S.rank(top)
                np.testing.assert_array_equal(idx, by_sum[:top], err_msg=f"rank({top}) idx")
                np.testing.assert_array_equal(sm, cum[by_sum[:top]], err_msg=f"rank({top}) sum")

            def check_coverage_rank(top):
                idx, val = cc.expected_rank(cov, [1300], top)
                gi, gv = S.coverage_rank(top)
                np.testing.assert_array_equal(gi, idx, err_msg=f"coverage_rank({top}) idx")
                np.testing.assert_array_equal(gv, val, err_msg=f"coverage_rank({top}) covered")
            np.testing.assert_array_equal(S.coverage_rows(long_list), cov[long_list], err_msg="1 coverage_rows, 1310 entries")
            _assert_depth(S.depth_rows([1299]), [e[[1299]] for e in exp], "2 depth_rows([1299])")
            np.testing.assert_array_equal(S.coverage_rows(cc.ROWS_1300), cov[cc.ROWS_1300], err_msg="3 coverage_rows(ROWS_1300)")
            _assert_depth(S.depth_rows(perm), [e[perm] for e in exp], "4 depth_rows, a permutation of all")
            check_coverage_rank(1)
            check_rank(5)
            check_coverage_rank(5)
            check_rank(1)
            _assert_depth(S.depth(), exp, "9 depth()")
            np.testing.assert_array_equal(S.coverage(), cov, err_msg="10 coverage()")
            np.testing.assert_array_equal(exp[0], cov)
        finally:
            S.close()
    finally:
        R.close()


def _screen_lines(names, col_len, exp, table, top, depth=False, identity=False, geno=None):
    cov, med = exp[0], exp[1]
    size = col_len.astype(np.int64)
    order = sorted(range(len(names)), key=lambda g: (-Fraction(int(cov[g]), int(size[g])), g))[:top]   # (exact, as the host compares)
    lines = []
    for g in order:
        line = f"{names[g]}\t{int(cov[g])}\t{int(size[g])}\t{int(cov[g]) / int(size[g]):.6f}\t{int(table[g])}"
        if depth:
            line += f"\t{int(med[g])}"
        if identity:
            line += "\t%.6f" % ((int(cov[g]) / int(size[g])) ** (1 / cc.K))
        lines.append(line + ("\t" + "\t".join(geno[names[g]]) if geno else ""))
    return lines


def test_screen(gpu, tmp_path):
    """`sketchy-hip screen` on the single-species design written as .msh and its reads as FASTQ: the lines built from the expectation
    and the oracle's table with -d, with -I, with both, and with -H, -g and -l 500; without the flags the lines are what they were"""
    d, refs, col_lens, bases, offsets = cc.single(64)
    exp = dc.single_expected(64)
    names = [f"genome{i:04d}.fa" for i in range(1300)]
    msh, tsv, fq = str(tmp_path / "ref.msh"), str(tmp_path / "geno.tsv"), str(tmp_path / "reads.fq")
    write_msh(msh, names, [refs[0][g, :col_lens[0][g]] for g in range(1300)], kmer=cc.K, seed=cc.SEED, lengths=[6000] * 1300)
    geno = {nm: [f"ST{i % 7}", "R" if i % 3 else "S"] for i, nm in enumerate(names)}
    with open(tsv, "w") as f:
        f.write("id\tmlst\tmeca\n")
        for nm in names:
            f.write(nm + "\t" + "\t".join(geno[nm]) + "\n")
    with open(fq, "w") as f:
        for i, r in enumerate(unpack_reads(bases, offsets)):
            f.write(f"@read{i}\n{r.decode()}\n+\n{'I' * len(r)}\n")

    def run(*args):
        p = subprocess.run([BIN, "screen", "-r", msh, "-i", fq, *args], capture_output=True, text=True)
        assert p.returncode == 0, p.stderr
        return p.stdout.split("\n")[:-1]
    t1200, t500 = _oracle_table(64, 48, 1200)["cum"], _oracle_table(64, 48, 500)["cum"]
    cl = col_lens[0]
    head = "sketch_id\tcovered\tsketch_size\tcontainment\tshared_hashes"
    assert run() == _screen_lines(names, cl, exp[1200], t1200, 10)
    assert run("-l", "500", "-t", "3", "-H") == [head] + _screen_lines(names, cl, exp[500], t500, 3)
    assert run("-d") == _screen_lines(names, cl, exp[1200], t1200, 10, depth=True)
    assert run("--identity", "-t", "25") == _screen_lines(names, cl, exp[1200], t1200, 25, identity=True)
    assert run("-I", "--depth", "-t", "25", "-g", tsv, "-b", "256") == _screen_lines(names, cl, exp[1200], t1200, 25, True, True, geno)
    assert run("-d", "-l", "500", "-t", "3", "-H") == [head + "\tmedian_multiplicity"] + _screen_lines(names, cl, exp[500], t500, 3, depth=True)
    assert run("-l", "500", "-g", tsv, "-H", "-t", "1300", "-d", "-I") == \
        [head + "\tmedian_multiplicity\tidentity\tmlst\tmeca"] + _screen_lines(names, cl, exp[500], t500, 1300, True, True, geno)
    assert run("-I", "-H", "-t", "1") == [head + "\tidentity"] + _screen_lines(names, cl, exp[1200], t1200, 1, identity=True)
