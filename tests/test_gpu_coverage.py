"""Breadth of a stream on the device: covered[g] = hashes of genome g's column that some read so far has shared (its bottom-s sketch:
truncation first), against the oracle's expectation (tests/coverage_cases.py; its invariants and the conditions that keep these cases
from being vacuous: tests/test_coverage_cpu.py).  Everything is integer and compared exactly.

The marks ride on a pass's classify (one bit per key-table slot), so every storage class of a reference hash, every route by which a
stream's pass reaches the classify -- pushes cut into several passes, groups of enqueued batches, submit, packed input -- and every
forced variant of the pass has to leave the same bits; the walk reads the tiled matrix, so tile and rank-group edges, the padding behind
short columns and behind a species, and the lifted hashes (not in the matrix) are what it can get wrong."""
import functools
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

import coverage_cases as cc
import hash_classes as hc
from helpers import exp_env, unpack_reads
from mshio import write_msh

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "sketchy_amd", "sketchy-hip")
R_ = hc.R_TEST
TOPS = (1, 5, 64)


@functools.lru_cache(maxsize=None)
def _oracle_table(n_dense, s, n_reads):
    from oracle import oracle as orc
    d, refs, col_lens, bases, offsets = cc.single(n_dense)
    return orc.stream(cc.K, cc.SEED, s, refs[0], col_lens[0], bases, offsets[:n_reads + 1], top_k=1)


@pytest.mark.parametrize("n_dense,rare", [(64, R_), (65, R_), (900, R_), (64, 1024)])
def test_storage_classes(gpu, n_dense, rare):
    """hc.single_species under four policies / dictionary shapes, s = 48 (every read is truncated), synchronous pushes cut at
    [0, 500, 501, n]: after every cut the whole table, a scattered list (tile and rank-group edges, the last genome, the lineage starts,
    one index twice) and the ranking for top 1, 5, 64.  Rows and table equal those of a stream that never enabled coverage -- and the
    oracle's."""
    d, refs, col_lens, bases, offsets = cc.single(n_dense)
    exp = cc.single_expected(n_dense, None)
    R, _, _ = cc.create_reference(d, rare, s=cc.S_SINGLE)
    try:
        assert R.s == 48 and R.rare_index["keys"] > 0
        parts, table = cc.check_pushes(R, d.species, bases, offsets, cc.CUTS_1300, exp, cc.ROWS_1300, TOPS, what=f"dense={n_dense} rare={rare}")
        plain, plain_table = cc.plain_pushes(R, bases, offsets, cc.CUTS_1300)
        for a, b in zip(parts, plain):
            np.testing.assert_array_equal(a["topk_idx"], b["topk_idx"])
            np.testing.assert_array_equal(a["topk_sum"], b["topk_sum"])
        np.testing.assert_array_equal(table, plain_table)
        o = _oracle_table(n_dense, 48, 1200)
        np.testing.assert_array_equal(table, o["cum"])
        np.testing.assert_array_equal(np.concatenate([p["topk_idx"] for p in parts]), o["topk_idx"])
        assert (exp[1200] <= table).all()
    finally:
        R.close()


def test_a_reference_without_the_index(gpu):
    """rare_hash_genomes = 0: enable_coverage is SKX_ERR_UNSUPPORTED, the stream goes on working (rows and table the oracle's), the
    queries are SKX_ERR_INVALID"""
    from sketchy_amd import _lib, api
    d, refs, col_lens, bases, offsets = cc.single(64)
    R, _, _ = cc.create_reference(d, 0, s=cc.S_SINGLE)
    try:
        assert R.rare_index["keys"] == 0
        S = api.SumOfSharedHashes(R, top=1, max_batch_reads=1200, max_batch_bases=len(bases))
        try:
            with pytest.raises(_lib.SketchyHipError) as e:
                S.enable_coverage()
            assert e.value.code == _lib.ERR_UNSUPPORTED
            got = S.push(bases, offsets)
            o = _oracle_table(64, 48, 1200)
            np.testing.assert_array_equal(got["topk_idx"], o["topk_idx"])
            np.testing.assert_array_equal(got["topk_sum"], o["topk_sum"])
            np.testing.assert_array_equal(S.table(), o["cum"])
            for q in (S.coverage, lambda: S.coverage_rows([0, 1]), lambda: S.coverage_rank(1)):
                with pytest.raises(_lib.SketchyHipError) as e:
                    q()
                assert e.value.code == _lib.ERR_INVALID
        finally:
            S.close()
    finally:
        R.close()


def test_saturation(gpu):
    """s = 512: no read is truncated, and the columns fill up -- 689 / 1 053 / 1 277 full columns after 100 / 500 / 1 200 reads, nobody
    above its col_len.  (The matrices are widened to 512 columns, col_len unchanged: s does not exceed the stride.)"""
    from sketchy_amd import api
    d, refs, col_lens, bases, offsets = cc.single(64)
    at = (100, 500, 1200)
    exp = cc.single_expected(64, 512, at)
    R, _, _ = cc.create_reference(d, R_, s=512, pad_to=512)
    try:
        S = api.SumOfSharedHashes(R, top=1, max_batch_reads=1200, max_batch_bases=len(bases))
        try:
            S.enable_coverage()
            full = []
            for a, b in zip((0,) + at[:-1], at):
                S.push(bases, offsets[a:b + 1])
                cov = S.coverage()
                np.testing.assert_array_equal(cov, exp[b], err_msg=f"after {b} reads")
                assert (cov <= col_lens[0]).all()
                full.append(int((cov == col_lens[0]).sum()))
            assert full == [689, 1053, 1277]
            cc.check_queries(S, exp[1200], d.species, cc.ROWS_1300, TOPS, what="saturated")
        finally:
            S.close()
    finally:
        R.close()


def test_batches_that_share_passes(gpu):
    """the reads as twelve enqueue_device batches; coverage is queried after every fourth (the query flushes) and at the end"""
    from sketchy_amd import api
    d, refs, col_lens, bases, offsets = cc.single(64)
    cuts = list(range(0, 1201, 100))
    exp = cc.single_expected(64, None, (400, 800, 1200))
    R, _, _ = cc.create_reference(d, R_, s=cc.S_SINGLE)
    try:
        S = api.SumOfSharedHashes(R, top=0, max_batch_reads=2400, max_batch_bases=len(bases))
        try:
            S.enable_coverage()
            cc.enqueue_batches(S, bases, offsets, cuts, query_after=(4, 8, 12),
                               on_query=lambda b: cc.check_queries(S, exp[b], d.species, cc.ROWS_1300, (5,), what=f"enqueued, {b} reads"))
            cc.check_queries(S, exp[1200], d.species, cc.ROWS_1300, TOPS, what="enqueued, end")
            st = S.stats()
            assert st["passes_shared"] >= 1, st
            np.testing.assert_array_equal(S.table(), _oracle_table(64, 48, 1200)["cum"])
        finally:
            S.close()
    finally:
        R.close()


def test_a_push_cut_into_several_passes(gpu):
    """stream_query_rows = 512: one push of 1 200 reads takes several passes, every one of them marks"""
    from sketchy_amd import api
    d, refs, col_lens, bases, offsets = cc.single(65)
    exp = cc.single_expected(65, None)
    R, _, _ = cc.create_reference(d, R_, s=cc.S_SINGLE)
    try:
        api.set_option("stream_query_rows", 512)
        try:
            S = api.SumOfSharedHashes(R, top=1, max_batch_reads=1200, max_batch_bases=len(bases))
        finally:
            api.set_option("stream_query_rows", 0)
        try:
            S.enable_coverage()
            S.push(bases, offsets)
            assert S.stats()["last_passes"] > 1
            cc.check_queries(S, exp[1200], d.species, cc.ROWS_1300, TOPS, what="stream_query_rows=512")
        finally:
            S.close()
    finally:
        R.close()


@pytest.mark.parametrize("packed", (False, True), ids=("ascii", "packed"))
def test_submit_and_packed_input(gpu, packed):
    """page-locked batches through submit / drain, as ASCII and as 4-bit packed input"""
    from sketchy_amd import api
    d, refs, col_lens, bases, offsets = cc.single(64)
    exp = cc.single_expected(64, None)
    data, off = api.pack_reads(bases, offsets, first_nibble=1) if packed else (np.ascontiguousarray(bases), np.ascontiguousarray(offsets))
    R, _, _ = cc.create_reference(d, R_, s=cc.S_SINGLE)
    try:
        S = api.SumOfSharedHashes(R, top=0, max_batch_reads=1200, max_batch_bases=len(bases) + 2)
        keep = []
        try:
            S.enable_coverage()
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
            cc.check_queries(S, exp[1200], d.species, cc.ROWS_1300, (1, 5), what=f"submit packed={packed}")
            np.testing.assert_array_equal(S.table(), _oracle_table(64, 48, 1200)["cum"])
            # ... and a synchronous push of packed input on top changes nothing: every hash of these reads has been seen
            S.push(data, off[900:1201])
            np.testing.assert_array_equal(S.coverage(), exp[1200])
        finally:
            S.close()
            for h in keep:
                h.free()
    finally:
        R.close()


def test_several_species(gpu):
    """(70, 600, 3) genomes: the table in species order, the ranking per species for top 1 and 3 (3 = the whole smallest species; ties
    cut by both, the lower index wins), and the genome that holds 0xFF..FF (padded index far from its real one) gets no credit for it"""
    from sketchy_amd import _lib, api
    d = hc.species_design()
    R, refs, col_lens = cc.create_reference(d, R_)
    try:
        bases, offsets = hc.reads(d, n_reads=600)
        exp = cc.expected_coverage(refs, col_lens, bases, offsets, R.s, (250, 600))
        S = api.SumOfSharedHashes(R, top=2, max_batch_reads=600, max_batch_bases=len(bases))
        try:
            S.enable_coverage()
            rows = np.array([0, 69, 70, 669, 670, 672, 71, 670], np.uint32)
            for a, b in ((0, 250), (250, 600)):
                S.push(bases, offsets[a:b + 1])
                cc.check_queries(S, exp[b], d.species, rows, (1, 3), what=f"species, {b} reads")
            cov = S.coverage()
            holder = int(d.members[hc.FF][0])
            ordinary = sum(1 for h, m in d.members.items() if h < hc.FE and holder in m)
            assert holder == 672 and cov[holder] <= ordinary == int(np.concatenate(col_lens)[holder]) - 1
            with pytest.raises(_lib.SketchyHipError) as e:
                S.coverage_rank(4)
            assert e.value.code == _lib.ERR_INVALID
            with pytest.raises(_lib.SketchyHipError) as e:
                S.coverage_rows([673])
            assert e.value.code == _lib.ERR_INVALID
            assert len(S.coverage_rows([])) == 0
        finally:
            S.close()
    finally:
        R.close()


@pytest.mark.parametrize("n_genomes,which", [(600, "both"), (20, "ff")])
def test_lifted_references(gpu, n_genomes, which):
    """references that hold 0xFF..FE / 0xFF..FF in some columns, 300 reads: the expectation as it is -- the holders get no credit for a
    value no read hashes to, the walk never probes the padding; at 600 genomes 243 stay at zero"""
    from sketchy_amd import api
    d = hc.lifted_design(n_genomes, which)
    R, refs, col_lens = cc.create_reference(d, R_)
    try:
        bases, offsets = hc.reads(d, n_reads=300)
        exp = cc.expected_coverage(refs, col_lens, bases, offsets, R.s, (300,))[300]
        if n_genomes == 600:
            assert int((exp == 0).sum()) == 243
        S = api.SumOfSharedHashes(R, top=1, max_batch_reads=300, max_batch_bases=len(bases))
        try:
            S.enable_coverage()
            S.push(bases, offsets)
            rows = np.array([0, 3, n_genomes // 2, n_genomes // 3, n_genomes - 2, n_genomes - 1, 3], np.uint32)
            cc.check_queries(S, exp, d.species, rows, (1, 5, min(20, n_genomes)), what=f"lifted {which} n={n_genomes}")
        finally:
            S.close()
    finally:
        R.close()


def test_state(gpu):
    """enable after reads is SKX_ERR_INVALID; reset clears the bits and keeps coverage enabled; the same reads give the same numbers
    again; two streams on one reference do not see each other; table_add does not touch the set"""
    from sketchy_amd import _lib, api
    d, refs, col_lens, bases, offsets = cc.single(64)
    exp = cc.single_expected(64, None)
    R, _, _ = cc.create_reference(d, R_, s=cc.S_SINGLE)
    try:
        A = api.SumOfSharedHashes(R, top=1, max_batch_reads=1200, max_batch_bases=len(bases))
        B = api.SumOfSharedHashes(R, top=1, max_batch_reads=1200, max_batch_bases=len(bases))
        C_ = api.SumOfSharedHashes(R, top=1, max_batch_reads=1200, max_batch_bases=len(bases))
        try:
            C_.push(bases, offsets[:11])
            with pytest.raises(_lib.SketchyHipError) as e:
                C_.enable_coverage()
            assert e.value.code == _lib.ERR_INVALID
            C_.reset()
            C_.enable_coverage()   # (after a reset the stream has taken no reads)
            A.enable_coverage()
            B.enable_coverage()
            assert not A.coverage().any()
            A.push(bases, offsets[:501])
            B.push(bases, offsets[500:502])
            np.testing.assert_array_equal(A.coverage(), exp[500])
            only = cc.expected_coverage(refs, col_lens, bases[int(offsets[500]):int(offsets[501])], offsets[500:502] - offsets[500], 48, (1,))[1]
            np.testing.assert_array_equal(B.coverage(), only)
            assert not C_.coverage().any()
            A.table_add(np.ones(1300, np.uint64))
            np.testing.assert_array_equal(A.coverage(), exp[500])
            A.reset()
            assert not A.coverage().any() and A.reads == 0
            A.enable_coverage()
            A.push(bases, offsets[:502])
            np.testing.assert_array_equal(A.coverage(), exp[501])
            np.testing.assert_array_equal(B.coverage(), only)
        finally:
            A.close(); B.close(); C_.close()
    finally:
        R.close()


@pytest.mark.parametrize("knobs", [{"SKX_STATIC_DENSE": 0}, {"SKX_PATTERNS": 0}, {"SKX_LONG_ROWS": 0}, {"SKX_RARE_DIRECT": 0}, {"SKX_PASS_READS": 64}],
                         ids=lambda k: "-".join(f"{a}={b}" for a, b in k.items()))
def test_forced_variants(gpu, knobs):
    """the 64-dense case, pushes and enqueued batches, in a fresh child with the experiments build: per-pass dictionaries, no patterns,
    no bit rows, rare rows through M, passes of 64 reads"""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "coverage_worker.py")], env=exp_env(**knobs), capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert out.stdout.rstrip().endswith("coverage ok")


def _screen_lines(names, col_len, cov, table, top, geno=None):
    size = col_len.astype(np.int64)
    order = sorted(range(len(names)), key=lambda g: (-Fraction(int(cov[g]), int(size[g])), g))[:top]   # (exact, as the host compares)
    lines = []
    for g in order:
        line = f"{names[g]}\t{int(cov[g])}\t{int(size[g])}\t{int(cov[g]) / int(size[g]):.6f}\t{int(table[g])}"
        lines.append(line + ("\t" + "\t".join(geno[names[g]]) if geno else ""))
    return lines


def test_screen(gpu, tmp_path):
    """`sketchy-hip screen` on the single-species design written as .msh and its reads as FASTQ: the lines built from the expectation
    and the oracle's table -- default top, -t, -l, -H, with and without -g"""
    d, refs, col_lens, bases, offsets = cc.single(64)
    exp = cc.single_expected(64, None)
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
    assert run() == _screen_lines(names, col_lens[0], exp[1200], t1200, 10)
    assert run("-t", "25", "-g", tsv, "-b", "256") == _screen_lines(names, col_lens[0], exp[1200], t1200, 25, geno)
    head = "sketch_id\tcovered\tsketch_size\tcontainment\tshared_hashes"
    assert run("-l", "500", "-t", "3", "-H") == [head] + _screen_lines(names, col_lens[0], exp[500], t500, 3)
    assert run("-l", "500", "-g", tsv, "-H", "-t", "1300") == [head + "\tmlst\tmeca"] + _screen_lines(names, col_lens[0], exp[500], t500, 1300, geno)
    p = subprocess.run([BIN, "screen", "-r", msh, "-i", fq, "-t", "1301"], capture_output=True, text=True)
    assert p.returncode == 2 and "--top" in p.stderr
