"""Winner-takes-all breadth on the device: won[g] = seen hashes of genome g's column credited to g alone -- every seen hash goes to the
first of its holders in the global order (containment as an exact fraction, then covered, then the index) -- against the oracle's
expectation (tests/winner_cases.py; its invariants and the conditions that keep these cases from being vacuous:
tests/test_winners_cpu.py).  Everything is integer and compared exactly.

The queries recompute from the seen set: a whole-table count, the host's sort, a marking walk (an atomic minimum per seen hash over the
ranks of its holders, merged per wave) and a counting walk.  What they can get wrong: the order's tie rules (the saturated case leaves
15 distinct containments among 1 300 genomes), holders in different tiles, rank groups and species, the lifted hashes (not in the
matrix), the padding behind short columns and behind a species, and a list whose groups are a subset of the marked table."""
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
import winner_cases as wc
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


def _stream(R, bases, n=1200, top=1):
    from sketchy_amd import api
    return api.SumOfSharedHashes(R, top=top, max_batch_reads=n, max_batch_bases=max(1, len(bases)))


@pytest.mark.parametrize("n_dense,rare", [(64, R_), (65, R_), (900, R_), (64, 1024)])
def test_storage_classes(gpu, n_dense, rare):
    """hc.single_species under four policies / dictionary shapes, s = 48, synchronous pushes cut at [0, 500, 501, n]: after every cut the
    whole table, a scattered list (tile and rank-group edges, the last genome, the lineage starts, one index twice) and the ranking by
    won for top 1, 5, 64; covered of winners() is coverage().  Rows and table equal those of a stream that never asked."""
    d, refs, col_lens, bases, offsets = cc.single(n_dense)
    exp = wc.single_expected(n_dense, None)
    R, _, _ = cc.create_reference(d, rare, s=cc.S_SINGLE)
    try:
        parts, table = wc.check_pushes(R, d.species, bases, offsets, cc.CUTS_1300, exp, cc.ROWS_1300, TOPS, what=f"dense={n_dense} rare={rare}")
        plain, plain_table = cc.plain_pushes(R, bases, offsets, cc.CUTS_1300)
        for a, b in zip(parts, plain):
            np.testing.assert_array_equal(a["topk_idx"], b["topk_idx"])
            np.testing.assert_array_equal(a["topk_sum"], b["topk_sum"])
        np.testing.assert_array_equal(table, plain_table)
        np.testing.assert_array_equal(table, _oracle_table(n_dense, 48, 1200)["cum"])
    finally:
        R.close()


def test_saturated_columns(gpu):
    """s = 512: the columns fill up, after 1 200 reads 15 distinct containments remain among 1 300 genomes -- almost every place of the
    order is decided by the second and third rule"""
    d, refs, col_lens, bases, offsets = cc.single(64)
    at = (100, 1200)
    exp = wc.single_expected(64, 512, at)
    w = exp[1200]
    assert len(set(Fraction(int(c), int(n)) for c, n in zip(w.covered, col_lens[0]))) == 15
    R, _, _ = cc.create_reference(d, R_, s=512, pad_to=512)
    try:
        S = _stream(R, bases)
        try:
            S.enable_coverage()
            for a, b in zip((0,) + at[:-1], at):
                S.push(bases, offsets[a:b + 1])
                wc.check_queries(S, exp[b], d.species, cc.ROWS_1300, TOPS, what=f"saturated, {b} reads")
        finally:
            S.close()
    finally:
        R.close()


def test_several_species(gpu):
    """(70, 600, 3) genomes, 1 200 reads: ONE order over all species; the table in species order, the ranking per species for top 1 and 3;
    a seen hash held by two species is credited to exactly one genome of one of them"""
    from sketchy_amd import _lib
    d = hc.species_design()
    R, refs, col_lens = cc.create_reference(d, R_)
    try:
        bases, offsets = hc.reads(d, n_reads=1200)
        exp = wc.expected_winners(refs, col_lens, bases, offsets, R.s, (500, 1200))
        S = _stream(R, bases, top=2)
        try:
            S.enable_coverage()
            rows = np.array([0, 69, 70, 669, 670, 672, 71, 670], np.uint32)
            for a, b in ((0, 500), (500, 1200)):
                S.push(bases, offsets[a:b + 1])
                wc.check_queries(S, exp[b], d.species, rows, (1, 3), what=f"species, {b} reads")
            cov, won = S.winners()
            w = exp[1200]
            shared = [h for h in w.winner if len(set(int(x) for x in d.species_of(d.members[h]))) >= 2]
            assert shared
            credited = 0
            for h in shared:   # the winner's species gets it, no genome of the other species does: their won is what the expectation says
                holders = np.asarray(d.members[h], np.int64)
                losers = holders[holders != w.winner[h]]
                assert (won[losers] == w.won[losers]).all() and won[w.winner[h]] == w.won[w.winner[h]] >= 1
                credited += 1
            assert credited == len(shared) and int(won.sum()) == w.n_seen
            with pytest.raises(_lib.SketchyHipError) as e:
                S.winners_rank(4)
            assert e.value.code == _lib.ERR_INVALID
        finally:
            S.close()
    finally:
        R.close()


def test_lifted_hashes(gpu):
    """hc.lifted_design(600, "both") with depth: after (0xFF..FE, 5) and (0xFF..FF, 7) are imported both values are seen, and of the
    holders of each exactly one wins it; the sum of won is depth_count()"""
    d = hc.lifted_design(600, "both")
    R, refs, col_lens = cc.create_reference(d, R_)
    try:
        bases, offsets = hc.reads(d, n_reads=300)
        before = wc.expected_winners(refs, col_lens, bases, offsets, R.s, (300,))[300]
        after = wc.expected_winners(refs, col_lens, bases, offsets, R.s, (300,), extra=(hc.FE, hc.FF))[300]
        for h in (hc.FE, hc.FF):
            assert len(d.members[h]) == 3 and h not in before.winner and after.winner[h] in d.members[h]
        assert after.n_seen == before.n_seen + 2
        S = _stream(R, bases, n=300)
        try:
            S.enable_depth()
            S.push(bases, offsets)
            rows = np.array([0, 3, 300, 200, 598, 599, *d.members[hc.FE], *d.members[hc.FF]], np.uint32)
            wc.check_queries(S, before, d.species, rows, (1, 5, 20), what="lifted, before the import")
            assert int(S.winners()[1].sum()) == S.depth_count() == before.n_seen
            assert S.depth_import(np.array([hc.FE, hc.FF], np.uint64), np.array([5, 7], np.uint32)) == 0
            wc.check_queries(S, after, d.species, rows, (1, 5, 20), what="lifted, after the import")
            cov, won = S.winners()
            assert int(won.sum()) == S.depth_count() == after.n_seen
            for h in (hc.FE, hc.FF):   # (won == the expectation's, checked above: its winner of the value is one of the three holders)
                holders = np.asarray(d.members[h], np.int64)
                assert sum(1 for g in holders if after.winner[h] == g) == 1 and won[after.winner[h]] >= 1
        finally:
            S.close()
    finally:
        R.close()


def test_batches_that_share_passes(gpu):
    """the reads as twelve enqueue_device batches; the winners are queried after every fourth (the query flushes) and at the end"""
    from sketchy_amd import api
    d, refs, col_lens, bases, offsets = cc.single(64)
    cuts = list(range(0, 1201, 100))
    exp = wc.single_expected(64, None, (400, 800, 1200))
    R, _, _ = cc.create_reference(d, R_, s=cc.S_SINGLE)
    try:
        S = api.SumOfSharedHashes(R, top=0, max_batch_reads=2400, max_batch_bases=len(bases))
        try:
            S.enable_coverage()
            cc.enqueue_batches(S, bases, offsets, cuts, query_after=(4, 8, 12),
                               on_query=lambda b: wc.check_queries(S, exp[b], d.species, cc.ROWS_1300, (5,), what=f"enqueued, {b} reads"))
            wc.check_queries(S, exp[1200], d.species, cc.ROWS_1300, TOPS, what="enqueued, end")
            assert S.stats()["passes_shared"] >= 1
            np.testing.assert_array_equal(S.table(), _oracle_table(64, 48, 1200)["cum"])
        finally:
            S.close()
    finally:
        R.close()


def test_a_push_cut_into_several_passes(gpu):
    """stream_query_rows = 512: one push of 1 200 reads takes several passes"""
    from sketchy_amd import api
    d, refs, col_lens, bases, offsets = cc.single(65)
    exp = wc.single_expected(65, None)
    R, _, _ = cc.create_reference(d, R_, s=cc.S_SINGLE)
    try:
        api.set_option("stream_query_rows", 512)
        try:
            S = _stream(R, bases)
        finally:
            api.set_option("stream_query_rows", 0)
        try:
            S.enable_coverage()
            S.push(bases, offsets)
            assert S.stats()["last_passes"] > 1
            wc.check_queries(S, exp[1200], d.species, cc.ROWS_1300, TOPS, what="stream_query_rows=512")
        finally:
            S.close()
    finally:
        R.close()


def test_state_and_errors(gpu):
    """a query before coverage is enabled is SKX_ERR_INVALID; after reset() everything is zero; the same reads again give the same
    numbers; two streams on one reference do not see each other; table_add changes nothing; an index >= n_genomes is SKX_ERR_INVALID
    and leaves the outputs untouched; n == 0 is SKX_OK; NULL outputs are accepted one at a time"""
    import ctypes as C
    from sketchy_amd import _lib
    L = _lib.load()
    d, refs, col_lens, bases, offsets = cc.single(64)
    exp = wc.single_expected(64, None)
    R, _, _ = cc.create_reference(d, R_, s=cc.S_SINGLE)
    try:
        A, B, N = _stream(R, bases), _stream(R, bases), _stream(R, bases)
        try:
            for q in (N.winners, lambda: N.winners_rows([0, 1]), lambda: N.winners_rank(1)):
                with pytest.raises(_lib.SketchyHipError) as e:
                    q()
                assert e.value.code == _lib.ERR_INVALID
            A.enable_coverage()
            B.enable_coverage()
            cov, won = A.winners()
            assert not cov.any() and not won.any()
            A.push(bases, offsets[:501])
            B.push(bases, offsets[500:502])
            wc.check_queries(A, exp[500], d.species, cc.ROWS_1300, (5,), what="A, 500 reads")
            only = wc.expected_winners(refs, col_lens, bases[int(offsets[500]):int(offsets[501])], offsets[500:502] - offsets[500], 48, (1,))[1]
            wc.check_queries(B, only, d.species, cc.ROWS_1300, (5,), what="B, one read")
            A.table_add(np.ones(1300, np.uint64))
            wc.check_queries(A, exp[500], d.species, cc.ROWS_1300, (1,), what="A after table_add")
            # the raw entry points: an index out of range, n == 0, NULL outputs
            h = A._h
            out_c, out_w = np.full(3, 77, np.uint32), np.full(3, 88, np.uint32)
            pc, pw = out_c.ctypes.data_as(C.c_void_p), out_w.ctypes.data_as(C.c_void_p)
            for bad in ([0, 1300, 5], [1300, 0, 5], [0, 5, 0xFFFFFFFF]):
                g = np.array(bad, np.uint32)
                assert L.skx_stream_winners_rows(h, g.ctypes.data_as(C.c_void_p), 3, pc, pw) == _lib.ERR_INVALID
                assert b"genomes[" in L.skx_last_error()
                assert (out_c == 77).all() and (out_w == 88).all()
            assert L.skx_stream_winners_rows(h, None, 0, None, None) == _lib.OK
            assert L.skx_stream_winners_rows(h, None, 1, pc, pw) == _lib.ERR_INVALID
            assert (out_c == 77).all() and (out_w == 88).all()
            g = np.array([0, 1299, 256], np.uint32)
            pg = g.ctypes.data_as(C.c_void_p)
            assert L.skx_stream_winners_rows(h, pg, 3, pc, None) == _lib.OK
            assert out_c.tolist() == exp[500].covered[g].tolist() and (out_w == 88).all()
            assert L.skx_stream_winners_rows(h, pg, 3, None, pw) == _lib.OK
            assert out_w.tolist() == exp[500].won[g].tolist()
            assert L.skx_stream_winners_rows(h, pg, 3, None, None) == _lib.OK
            full_c, full_w = np.zeros(1300, np.uint32), np.zeros(1300, np.uint32)
            assert L.skx_stream_winners(h, full_c.ctypes.data_as(C.c_void_p), None) == _lib.OK
            assert L.skx_stream_winners(h, None, full_w.ctypes.data_as(C.c_void_p)) == _lib.OK
            assert L.skx_stream_winners(h, None, None) == _lib.OK
            np.testing.assert_array_equal(full_c, exp[500].covered)
            np.testing.assert_array_equal(full_w, exp[500].won)
            assert L.skx_stream_winners_rank(h, 0, pc, pw) == _lib.ERR_INVALID
            assert L.skx_stream_winners_rank(h, 1301, pc, pw) == _lib.ERR_INVALID
            assert L.skx_stream_winners_rank(h, 1, None, pw) == _lib.ERR_INVALID
            # reset, and the same reads again
            A.reset()
            cov, won = A.winners()
            assert not cov.any() and not won.any() and A.reads == 0
            assert not A.winners_rank(5)[1].any()
            A.enable_coverage()
            A.push(bases, offsets[:502])
            wc.check_queries(A, exp[501], d.species, cc.ROWS_1300, (5,), what="A again, 501 reads")
            wc.check_queries(B, only, d.species, cc.ROWS_1300, (1,), what="B afterwards")
        finally:
            A.close(); B.close(); N.close()
    finally:
        R.close()


@pytest.mark.parametrize("knobs", [{"SKX_STATIC_DENSE": 0}, {"SKX_PATTERNS": 0}, {"SKX_RARE_DIRECT": 0}, {"SKX_PASS_READS": 64}],
                         ids=lambda k: "-".join(f"{a}={b}" for a, b in k.items()))
def test_forced_variants(gpu, knobs):
    """the 64-dense case, pushes and enqueued batches, in a fresh child with the experiments build: per-pass dictionaries, no patterns,
    rare rows through M, passes of 64 reads"""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "winners_worker.py")], env=exp_env(**knobs), capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert out.stdout.rstrip().endswith("winners ok")


def _plain_lines(names, col_len, cov, table, top, geno=None):
    """as tests/test_gpu_coverage.py::test_screen builds them"""
    size = col_len.astype(np.int64)
    order = sorted(range(len(names)), key=lambda g: (-Fraction(int(cov[g]), int(size[g])), g))[:top]
    lines = []
    for g in order:
        line = f"{names[g]}\t{int(cov[g])}\t{int(size[g])}\t{int(cov[g]) / int(size[g]):.6f}\t{int(table[g])}"
        lines.append(line + ("\t" + "\t".join(geno[names[g]]) if geno else ""))
    return lines


def _winner_lines(names, col_len, w, table, top, med=None, identity=False, geno=None):
    """by won / size exactly, then the larger plain containment, then the sketch earlier in the file"""
    size = col_len.astype(np.int64)
    cov, won = w.covered, w.won
    order = sorted(range(len(names)), key=lambda g: (-Fraction(int(won[g]), int(size[g])), -Fraction(int(cov[g]), int(size[g])), g))[:top]
    lines = []
    for g in order:
        line = (f"{names[g]}\t{int(cov[g])}\t{int(size[g])}\t{int(cov[g]) / int(size[g]):.6f}\t{int(table[g])}"
                f"\t{int(won[g])}\t{int(won[g]) / int(size[g]):.6f}")
        if med is not None:
            line += f"\t{int(med[g])}"
        if identity:
            line += "\t%.6f" % ((int(won[g]) / int(size[g])) ** (1 / cc.K))
        lines.append(line + ("\t" + "\t".join(geno[names[g]]) if geno else ""))
    return lines


def test_screen(gpu, tmp_path):
    """`sketchy-hip screen -w` on the single-species design written as .msh and its reads as FASTQ: the lines built from the expectation
    and the oracle's table -- default top, -t, -H, with -g, with -d -I (the identity from the winner containment); without -w the bytes
    are what they were"""
    d, refs, col_lens, bases, offsets = cc.single(64)
    exp = wc.single_expected(64, None)
    med = dc.single_expected(64)
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
    whead = head + "\twon\twinner_containment"
    assert run("-w") == _winner_lines(names, cl, exp[1200], t1200, 10)
    assert run("--winner-take-all", "-t", "25", "-b", "256") == _winner_lines(names, cl, exp[1200], t1200, 25)
    assert run("-w", "-l", "500", "-t", "3", "-H") == [whead] + _winner_lines(names, cl, exp[500], t500, 3)
    assert run("-w", "-l", "500", "-g", tsv, "-H", "-t", "1300") == [whead + "\tmlst\tmeca"] + _winner_lines(names, cl, exp[500], t500, 1300, geno=geno)
    assert run("-w", "-d", "-I", "-t", "25", "-H", "-g", tsv) == \
        [whead + "\tmedian_multiplicity\tidentity\tmlst\tmeca"] + _winner_lines(names, cl, exp[1200], t1200, 25, med[1200][1], True, geno)
    # the top of the two orders differs on this design -- and without -w nothing has changed
    assert [ln.split("\t")[0] for ln in run("-w")] != [ln.split("\t")[0] for ln in run()]
    assert run() == _plain_lines(names, cl, exp[1200].covered, t1200, 10)
    assert run("-l", "500", "-g", tsv, "-H", "-t", "1300") == [head + "\tmlst\tmeca"] + _plain_lines(names, cl, exp[500].covered, t500, 1300, geno)
