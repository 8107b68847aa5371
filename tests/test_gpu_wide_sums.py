"""GPU parity of every ranking path with running sums past 32 bits.

The running table is u64 through the whole ABI (Vec<u64> in the reference, src/sketchy.rs:326) and a real run passes 2^32 within a
million reads, yet no stream of a test can: the other files' sums stay in the millions, so the upper word of every 64-bit quantity of
the ranking was zero in every comparison.  Here the table is SEEDED (skx_stream_table_add) so that chosen genomes -- the contenders --
cross 2^32, 2^33 + 2^32 or 2^54 in the middle of a 320-read stream while everybody else sits where a compare on the low word, or on a
truncated difference, orders them wrongly.  The number of contenders and their placement select the branch of the pruned rankings
(1 candidate in a rank group, at most 8, at most 64, replay; everyone tied) and the compact / full ranking of the shared passes.
Every check is exact equality with the oracle (oracle/oracle.c: stable sort of the u64 sums) started from the same table.

Also here: the table's stated bound (SKX_MAX_TABLE_SUM = 2^54 - 1, enforced by skx_stream_table_add: the top-k key of 2 <= top <= 16
holds sum + 1 in 55 bits) and the table's plumbing (read back, add in parts, resume from a checkpoint) at that width."""
import functools

import numpy as np
import pytest

from helpers import workload, workload_species
from oracle import oracle as orc
from test_gpu_enqueue import _enqueue_stream

pytestmark = pytest.mark.gpu

N, S_LEN, N_READS, K_MER, SEED = 1100, 160, 320, 16, 0   # three rank groups of 512 genomes, more than the 1024 candidate slots
BOUNDARY = {"m32": 1 << 32, "m33": (1 << 33) + (1 << 32), "m54": 1 << 54}
OFFSET = 120   # every genome gains 239..303 over the 320 reads: a contender seeded this far below the boundary crosses it mid-stream
# (contenders, spread over the reference or not): a seeded table is ranked on the genomes that reach the top-th value, packed into rank
# groups of 512 -- with top <= K those are the K contenders in ONE group: 1, at most 8, at most 64 candidates, more (the replay) are the
# branches of the pruned top-k kernel; 1100: everyone tied, more than the 1024 candidate slots, ranked on everything
CONTENDERS = [(1, 0), (8, 0), (9, 1), (64, 0), (65, 0), (130, 1), (1100, 0)]
TOPS = (1, 2, 16, 17)                    # the top-1 kernel, the pruned top-k kernel (twice), the generic kernel
ALONE_SLOT = 512                         # first slot of the second rank group of a ranking on candidates
PUSH_CUTS = [0, 131, 200, 320]           # the crossing (reads 138..163) lies inside the second call, off the 64-read segment borders
ENQUEUE_CUTS = [0, 1, 130, 131, 200, 320]


@functools.lru_cache(maxsize=None)
def _workload():
    return workload(N, S_LEN, N_READS, read_len=700, rng_seed=91)


@functools.lru_cache(maxsize=None)
def _gains():
    """[n_reads + 1, n_genomes]: what the first r reads add to every genome (the oracle's per-read shared counts, summed)"""
    ref, bases, offsets = _workload()
    shared = orc.stream(K_MER, SEED, S_LEN, ref["ref"], ref["col_len"], bases, offsets, top_k=1, want_shared=True)["shared"]
    out = np.zeros((N_READS + 1, N), np.uint64)
    np.cumsum(shared, axis=0, dtype=np.uint64, out=out[1:])
    out.setflags(write=False)
    return out


@pytest.fixture(scope="module")
def wide(gpu):
    """the workload and ONE resident reference for the whole file"""
    from sketchy_amd import api
    ref, bases, offsets = _workload()
    R = api.ReferenceSketch(ref["ref"], ref["col_len"], k=K_MER, seed=SEED, device=0)
    yield R, ref, bases, offsets
    R.close()


def _positions(K, spread):
    return (np.arange(K) * (N // K if spread else 1) + 7) % N


def _seed_table(mag, K, spread):
    """contenders at B (every third one at B + 1: exact ties and near ties), everyone else where a narrow compare goes wrong"""
    g = np.arange(N, dtype=np.uint64)
    B = np.uint64(BOUNDARY[mag] - OFFSET)
    if mag == "m32":     # after the crossing the others' LOW word is larger than the contenders'
        seed = np.uint64(1000) + g % np.uint64(7)
    elif mag == "m33":   # even g: same low word, smaller high word; odd g: smaller high word, larger low word
        seed = np.where(g % np.uint64(2) == 0, B - np.uint64(1 << 32), B - np.uint64(1 << 33) + np.uint64(1000))
    else:
        seed = B - np.uint64(1 << 40) - g % np.uint64(5)
    seed = seed.astype(np.uint64)
    pos = _positions(K, spread)
    if K == 1:
        # One contender: the rows past the first are taken by the others, and a table that is not fresh is ranked on the genomes that
        # reach the top-th value, packed in reference order into rank groups of 512.  Only 512 of the others stay within reach of
        # the runner-up -- the first 511 and the last one of those on the highest level -- and the rest start 400 lower, more than the
        # stream adds to anyone (303): 513 candidates, the last of them ALONE in the second rank group -- the one-candidate branch
        # of the pruned top-k kernel at top 2 and 16, with a wide sum at every magnitude (_expected checks the count)
        level = seed.max() if mag != "m33" else B - np.uint64(1 << 32)
        near = np.flatnonzero((seed >= level - np.uint64(6)) & (g != np.uint64(pos[0])))
        alone = near[seed[near] == level][-1]
        keep = np.append(near[near != alone][:ALONE_SLOT - 1], alone)
        seed[np.setdiff1d(near, keep)] -= np.uint64(400)
    seed[pos] = B + (np.arange(K) % 3 == 2).astype(np.uint64)
    return seed, pos


@functools.lru_cache(maxsize=None)
def _expected(mag, K, spread, top):
    """the oracle's run from the seeded table -- computed once per case, shared by the push and the enqueue tests, never written to --
    with the conditions that keep the case sharp asserted on the oracle's own output"""
    ref, bases, offsets = _workload()
    seed, pos = _seed_table(mag, K, spread)
    exp = orc.stream(K_MER, SEED, S_LEN, ref["ref"], ref["col_len"], bases, offsets, top_k=top, cum=seed)
    X, kk = BOUNDARY[mag], min(K, top)
    first, last = int(exp["topk_sum"][0, 0]), int(exp["topk_sum"][-1, kk - 1])
    assert first < X <= last, (mag, K, spread, top, first, last)     # the crossing happens inside the stream, in the leading and the last contended row
    assert np.isin(exp["topk_idx"][:, :kk], pos).all()                # only contenders rank
    if K >= 8:
        assert (np.diff(exp["topk_idx"][:, 0].astype(np.int64)) != 0).any()   # the lead changes hands
    if K == 1 and top >= 2:
        # the first long batch of either test has 513 candidates (value as the batch ends >= the top-th value as it begins), and the
        # last of them holds the top-th value or more as the batch begins: a candidate of its rank group from the first segment on
        table = seed + _gains()
        for a, b in ((PUSH_CUTS[0], PUSH_CUTS[1]), (ENQUEUE_CUTS[1], ENQUEUE_CUTS[2])):
            theta = np.sort(table[a])[-top]
            cand = np.flatnonzero(table[b] >= theta)
            assert len(cand) == ALONE_SLOT + 1 and table[a][cand[-1]] >= theta, (mag, top, a, b, len(cand))
    for a in exp.values():
        if a is not None:
            a.setflags(write=False)
    seed.setflags(write=False)
    return seed, exp


def _stream(R, top, seed, bases):
    from sketchy_amd import api
    S = api.SumOfSharedHashes(R, top=top, max_batch_reads=N_READS, max_batch_bases=len(bases))
    S.table_add(seed)
    return S


def _push_in_parts(S, bases, offsets, cuts):
    parts = [S.push(bases, offsets[a:b + 1]) for a, b in zip(cuts[:-1], cuts[1:])]
    return np.concatenate([p["topk_idx"] for p in parts]), np.concatenate([p["topk_sum"] for p in parts])


@pytest.mark.parametrize("top", TOPS)
@pytest.mark.parametrize("K,spread", CONTENDERS)
@pytest.mark.parametrize("mag", ["m32", "m33", "m54"])
def test_pushes_rank_wide_sums_like_the_oracle(wide, mag, K, spread, top):
    """synchronous pushes, cut so that the crossing lies inside the second one (top 1: relative keys; 2 and 16: 64-bit keys; 17: the
    generic kernel); then the ranking of the table itself"""
    R, ref, bases, offsets = wide
    seed, exp = _expected(mag, K, spread, top)
    S = _stream(R, top, seed, bases)
    try:
        idx, val = _push_in_parts(S, bases, offsets, PUSH_CUTS)
        np.testing.assert_array_equal(val, exp["topk_sum"])
        np.testing.assert_array_equal(idx, exp["topk_idx"])
        np.testing.assert_array_equal(S.table(), exp["cum"])
        r_idx, r_sum = S.rank(64)
        order = orc.stable_rank(exp["cum"])[:64]
        np.testing.assert_array_equal(r_idx, order)
        np.testing.assert_array_equal(r_sum, exp["cum"][order])
    finally:
        S.close()


@pytest.mark.parametrize("top", [1, 2, 17])
@pytest.mark.parametrize("K,spread", [(1, 0), (9, 1), (65, 0), (1100, 0)])
@pytest.mark.parametrize("mag", ["m32", "m33", "m54"])
def test_enqueued_batches_rank_wide_sums_like_the_oracle(wide, mag, K, spread, top):
    """the shared passes (tables without the ranking, candidate selection, compact problems): a seeded table with at most 1024 genomes
    reaching the top-th value is ranked compactly, one with more (everyone tied) fully -- both asserted, so that neither path can leave
    this file unnoticed"""
    R, ref, bases, offsets = wide
    seed, exp = _expected(mag, K, spread, top)
    S = _stream(R, top, seed, bases)
    try:
        idx, val = _enqueue_stream(S, bases, offsets, ENQUEUE_CUTS, top)
        np.testing.assert_array_equal(val, exp["topk_sum"])
        np.testing.assert_array_equal(idx, exp["topk_idx"])
        np.testing.assert_array_equal(S.table(), exp["cum"])
        st = S.stats()
        if top <= K <= 130:
            assert st["batches_compact"] > 0, st
        if K == N:
            assert st["batches_full"] > 0, st
    finally:
        S.close()


SPECIES = (300, 70, 600)


@functools.lru_cache(maxsize=None)
def _species_workload():
    return workload_species(SPECIES, 200, 240, read_len=500, rng_seed=131)


@functools.lru_cache(maxsize=None)
def _species_expected(top):
    refs, bases, offsets = _species_workload()
    cums = [np.full(SPECIES[0], (1 << 32) - 60, np.uint64),                                       # crosses 2^32 in the stream
            np.uint64(1 << 40) + np.arange(SPECIES[1], dtype=np.uint64) % np.uint64(3),          # far above it, exact ties
            np.zeros(SPECIES[2], np.uint64)]                                                      # far below it
    exp = orc.stream_fast_species(K_MER, SEED, 200, [r["ref"] for r in refs], bases, offsets, top_k=top, cums=cums)
    first, last = int(exp["topk_sum"][0, 0, 0]), int(exp["topk_sum"][-1, 0, min(top, SPECIES[0]) - 1])
    assert first < (1 << 32) <= last, (top, first, last)
    return np.concatenate(cums), exp


@pytest.mark.parametrize("entry", ["push", "enqueue"])
@pytest.mark.parametrize("top", [1, 3, 17])
def test_three_species_below_across_and_above_32_bits(gpu, entry, top):
    from sketchy_amd import api
    refs, bases, offsets = _species_workload()
    seed, exp = _species_expected(top)
    n = len(offsets) - 1
    R = api.ReferenceSketch([r["ref"] for r in refs], [r["col_len"] for r in refs], k=K_MER, seed=SEED, device=0)
    S = api.SumOfSharedHashes(R, top=top, max_batch_reads=n, max_batch_bases=len(bases))
    try:
        S.table_add(seed)
        if entry == "push":
            idx, val = _push_in_parts(S, bases, offsets, [0, 97, 150, n])
        else:   # (rows are [n_reads][n_species][top]: the helper only sizes and shapes them)
            idx, val = _enqueue_stream(S, bases, offsets, [0, 1, 97, 150, n], len(SPECIES) * top)
            idx, val = idx.reshape(n, len(SPECIES), top), val.reshape(n, len(SPECIES), top)
        np.testing.assert_array_equal(val, exp["topk_sum"])
        np.testing.assert_array_equal(idx, exp["topk_idx"])
        np.testing.assert_array_equal(S.table(), exp["cum"])
        r_idx, r_sum = S.rank(top)
        for i, cum in enumerate(exp["cums"]):
            order = orc.stable_rank(cum)[:top]
            np.testing.assert_array_equal(r_idx[i], order)
            np.testing.assert_array_equal(r_sum[i], cum[order])
    finally:
        S.close()
        R.close()


def test_table_plumbing_at_width(wide):
    """read back bit for bit and added in two wide parts"""
    R, ref, bases, offsets = wide
    seed, _ = _expected("m54", 9, 1, 2)
    S = _stream(R, 2, seed, bases)
    try:
        np.testing.assert_array_equal(S.table(), seed)
        S.reset()
        assert not S.table().any()
        a = seed >> np.uint64(1)
        b = seed - a
        assert a.min() >= 1 << 32 and b.min() >= 1 << 32
        S.table_add(a)
        S.table_add(b)
        np.testing.assert_array_equal(S.table(), seed)
    finally:
        S.close()


@pytest.mark.parametrize("mag,cut", [("m33", 160), ("m54", 100)])
def test_a_stream_resumed_from_a_checkpoint_of_wide_sums(wide, mag, cut):
    """reads [0, cut) on one stream, its table handed to a second one that takes the rest: rows and final table of the uninterrupted
    run.  m33 is cut after its contenders crossed 2^33 + 2^32; a table whose contenders have crossed 2^54 is above what
    skx_stream_table_add accepts (SKX_MAX_TABLE_SUM), so m54 is cut before that and crosses on the resumed stream."""
    from sketchy_amd import api, _lib
    R, ref, bases, offsets = wide
    seed, exp = _expected(mag, 9, 1, 2)
    S = _stream(R, 2, seed, bases)
    S2 = api.SumOfSharedHashes(R, top=2, max_batch_reads=N_READS, max_batch_bases=len(bases))
    try:
        first = S.push(bases, offsets[:cut + 1])
        t = S.table()
        assert (1 << 32) <= int(t.max()) <= _lib.MAX_TABLE_SUM
        assert (int(t.max()) >= BOUNDARY[mag]) == (mag == "m33")
        S2.table_add(t)
        second = S2.push(bases, offsets[cut:])
        np.testing.assert_array_equal(np.concatenate([first["topk_sum"], second["topk_sum"]]), exp["topk_sum"])
        np.testing.assert_array_equal(np.concatenate([first["topk_idx"], second["topk_idx"]]), exp["topk_idx"])
        np.testing.assert_array_equal(S2.table(), exp["cum"])
    finally:
        S.close()
        S2.close()


def test_table_add_refuses_what_exceeds_the_bound(wide):
    """skx_stream_table_add takes an entry up to SKX_MAX_TABLE_SUM and no further (u64 wrap-around included); a refused add leaves the
    table as it was and the stream working: the 320 reads pushed next rank like the oracle's from that table"""
    from sketchy_amd import api, _lib
    R, ref, bases, offsets = wide
    M = _lib.MAX_TABLE_SUM
    assert M == (1 << 54) - 1
    S = api.SumOfSharedHashes(R, top=2, max_batch_reads=N_READS, max_batch_bases=len(bases))

    def one(g, v, rest=0):
        t = np.full(N, rest, np.uint64)
        t[g] = v
        return t

    def refused(add):
        before = S.table()
        with pytest.raises(_lib.SketchyHipError) as e:
            S.table_add(add)
        assert e.value.code == _lib.ERR_INVALID
        np.testing.assert_array_equal(S.table(), before)
        exp = orc.stream(K_MER, SEED, S_LEN, ref["ref"], ref["col_len"], bases, offsets, top_k=2, cum=before)
        got = S.push(bases, offsets)
        np.testing.assert_array_equal(got["topk_sum"], exp["topk_sum"])
        np.testing.assert_array_equal(got["topk_idx"], exp["topk_idx"])
        np.testing.assert_array_equal(S.table(), exp["cum"])
        S.reset()

    try:
        S.table_add(one(700, M))                       # exactly the bound, on a zero table: accepted and read back
        np.testing.assert_array_equal(S.table(), one(700, M))
        refused(one(700, 1))                           # ... and not one more on top of it
        refused(one(3, M + 1))                         # one more than the bound on a zero table (which stays fresh)
        S.table_add(np.full(N, (1 << 53) + 1, np.uint64))
        refused(np.full(N, (1 << 53) + 1, np.uint64))  # two adds of 2^53 + 1: the second is refused
        S.table_add(one(9, 5, rest=1000))
        refused(one(9, (1 << 64) - 1))                 # 5 + (2^64 - 1) is refused, not wrapped to 4
    finally:
        S.close()
