"""Expectations for winner-takes-all breadth (skx_stream_winners), from the oracle alone, and what the winners tests share
(tests/test_winners_cpu.py, tests/test_gpu_winners.py, tests/winners_worker.py).

    covered[g] = |{h in column g : some read pushed so far has h in its bottom-s sketch}|          (as tests/coverage_cases.py)
    order      = all genomes, species together: the larger covered / max(col_len, 1) as an exact fraction first, then the larger
                 covered, then the lower global index
    winner(x)  = the first genome of the order among those that hold the seen hash x
    won[g]     = seen hashes of column g whose winner is g

read by read orc.sketch(seq, k, seed, s) -- truncation to s first --, a running set of seen hashes; the order with fractions.Fraction.
Nothing of the library is involved.  Every expectation asserts the invariants on itself: won <= covered, the sum of won = distinct seen
reference hashes, the first genome of the order keeps everything it covers."""
import functools
from fractions import Fraction

import numpy as np

import coverage_cases as cc
from helpers import unpack_reads

K, SEED = cc.K, cc.SEED


def order_of(covered, col_len):
    """the global order: list of genome indices, first to last"""
    return sorted(range(len(covered)), key=lambda g: (-Fraction(int(covered[g]), max(int(col_len[g]), 1)), -int(covered[g]), g))


class Winners:
    """covered, won uint32 [n_genomes]; order (list of genomes); winner {hash: genome} for every seen hash some genome holds"""

    def __init__(self, refs, col_lens, seen):
        ref, col_len = np.concatenate(refs), np.concatenate(col_lens)
        valid = np.arange(ref.shape[1])[None, :] < col_len[:, None]
        have = np.isin(ref, np.fromiter(seen, np.uint64, len(seen))) & valid
        self.covered = have.sum(axis=1).astype(np.uint32)
        self.order = order_of(self.covered, col_len)
        rank = np.zeros(len(col_len), np.int64)
        rank[self.order] = np.arange(len(col_len))
        g, _ = np.nonzero(have)
        x = ref[have]
        first = np.lexsort((rank[g], x))           # by hash, the holders of one hash by their place in the order
        g, x = g[first], x[first]
        lead = np.concatenate([[True], x[1:] != x[:-1]]) if len(x) else np.zeros(0, bool)
        self.winner = dict(zip((int(v) for v in x[lead]), (int(v) for v in g[lead])))
        self.won = np.bincount(g[lead], minlength=len(col_len)).astype(np.uint32)
        self.n_seen = int(lead.sum())
        # the invariants of the definition
        assert (self.won <= self.covered).all()
        assert int(self.won.sum()) == self.n_seen == len(np.unique(ref[have]))
        if len(self.order):
            assert self.won[self.order[0]] == self.covered[self.order[0]]
        for a in (self.covered, self.won):
            a.setflags(write=False)

    @property
    def pair(self):
        return self.covered, self.won


def expected_winners(refs, col_lens, bases, offsets, s, at, extra=()):
    """{n_reads: Winners} for every read count in `at`; extra: hashes seen from the start (an import)"""
    from oracle import oracle as orc
    reads = unpack_reads(bases, offsets)
    at = sorted(set(int(a) for a in at))
    assert at and at[-1] <= len(reads)
    seen, out = set(int(h) for h in extra), {}
    if at[0] == 0:
        out[0] = Winners(refs, col_lens, seen)
    for r, seq in enumerate(reads[:at[-1]]):
        seen.update(int(h) for h in orc.sketch(seq, K, SEED, s))
        if r + 1 in at:
            out[r + 1] = Winners(refs, col_lens, seen)
    return out


@functools.lru_cache(maxsize=None)
def single_expected(n_dense, s=None, at=cc.CUTS_1300[1:]):
    d, refs, col_lens, bases, offsets = cc.single(n_dense)
    return expected_winners(refs, col_lens, bases, offsets, cc.S_SINGLE if s is None else s, at)


def expected_rank(won, species, top):
    """(idx, won) [n_species, top]: (won desc, index asc) per species, indices local to the species"""
    return cc.expected_rank(won, species, top)


def check_queries(S, exp, species, rows, tops, what=""):
    """winners(), winners_rows(rows) and winners_rank(top) of stream S against the expectation `exp` (a Winners, or (covered, won))"""
    e_cov, e_won = exp.pair if isinstance(exp, Winners) else exp
    cov, won = S.winners()
    assert cov.dtype == np.uint32 and won.dtype == np.uint32
    np.testing.assert_array_equal(cov, e_cov, err_msg=f"{what} winners covered")
    np.testing.assert_array_equal(won, e_won, err_msg=f"{what} winners won")
    rows = np.asarray(rows, np.uint32)
    cov, won = S.winners_rows(rows)
    np.testing.assert_array_equal(cov, e_cov[rows], err_msg=f"{what} winners_rows covered")
    np.testing.assert_array_equal(won, e_won[rows], err_msg=f"{what} winners_rows won")
    for top in tops:
        idx, val = expected_rank(e_won, species, top)
        gi, gv = S.winners_rank(top)
        np.testing.assert_array_equal(gv, val, err_msg=f"{what} winners_rank top={top} won")
        np.testing.assert_array_equal(gi, idx, err_msg=f"{what} winners_rank top={top} idx")


def check_pushes(R, species, bases, offsets, cuts, exp, rows, tops, what="", top=1):
    """synchronous pushes cut at `cuts`, the three queries after every cut, covered against coverage() too; returns (rows of the
    pushes, table)"""
    from sketchy_amd import api
    n = len(offsets) - 1
    S = api.SumOfSharedHashes(R, top=top, max_batch_reads=n, max_batch_bases=max(1, len(bases)))
    try:
        S.enable_coverage()
        parts = []
        for a, b in zip(cuts[:-1], cuts[1:]):
            parts.append(S.push(bases, offsets[a:b + 1]))
            check_queries(S, exp[b], species, rows, tops, what=f"{what} after {b} reads")
            np.testing.assert_array_equal(S.winners()[0], S.coverage(), err_msg=f"{what} after {b} reads: covered of winners() and coverage()")
        return parts, S.table()
    finally:
        S.close()
