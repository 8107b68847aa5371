"""skx_ref_neighbours on the device: for every genome of the resident reference the first `top` OTHER genomes of its species in
(shared hashes desc, index asc) order -- what offline `predict` of the genome's own sketch would print against a reference without it.

Expected values come from the oracle alone (neighbours_cases.py): counts from orc.common_hashes over all pairs of a species, computed
once per case; rows from orc.stable_rank of a genome's counts with its own entry deleted and the indices above it shifted back.
Everything is integer: compared exactly.  References are clone trees (helpers.workload), so ties are the rule."""
import ctypes as C
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import neighbours_cases as nc
from helpers import exp_env, workload, workload_species

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "sketchy_amd", "sketchy-hip")
S = 200
TOPS = (1, 2, 5, 16, 17, 64)
FE, FF = np.uint64(0xFFFFFFFFFFFFFFFE), np.uint64(0xFFFFFFFFFFFFFFFF)


def _tops(n):
    return sorted({t for t in TOPS + (n - 1,) if 1 <= t <= min(n - 1, 64)})


def _mixed_lengths(n, stride):
    """column lengths 0, 1, stride - 123 and stride, mixed: every genome with index % 7 == 5 takes the next of the first three"""
    col_len = np.full(n, stride, np.uint32)
    short = np.flatnonzero(np.arange(n) % 7 == 5)
    col_len[short] = np.array([0, 1, max(stride - 123, 0)], np.uint32)[np.arange(len(short)) % 3]
    return col_len


def _cols(ref, col_len):
    return [ref[g, :col_len[g]] for g in range(len(ref))]


@functools.lru_cache(maxsize=None)
def _case(n, stride=S):
    ref, _, _ = workload(n, stride, 1, read_len=400, genome_len=40000, rng_seed=700 + n + stride)
    col_len = _mixed_lengths(n, stride)
    counts = nc.pair_counts(_cols(ref["ref"], col_len))
    for a in (ref["ref"], col_len, counts):
        a.setflags(write=False)
    return ref["ref"], col_len, counts


def _check(got, counts, top, first=0, count=None, what=""):
    idx, val = nc.loo_rows(counts, top, first, count)
    np.testing.assert_array_equal(got[1], val, err_msg=f"{what} top={top} shared")
    np.testing.assert_array_equal(got[0], idx, err_msg=f"{what} top={top} idx")


@pytest.mark.gpu
@pytest.mark.parametrize("n", (2, 3, 65, 257, 600))
def test_sizes(gpu, n):
    """One word, the tile boundary at 256, the rank-group boundary at 512; self as the first genome, as the last, as the only other
    genome's neighbour (n = 2); every `top`.  A genome with an empty column: neighbours 0, 1, ... skipping itself, all with 0."""
    from sketchy_amd import api
    ref, col_len, counts = _case(n)
    R = api.ReferenceSketch(ref, col_len)
    try:
        for top in _tops(n):
            got = R.neighbours(top=top)
            assert got[0].shape == (n, top) and not (got[0] == np.arange(n)[:, None]).any()
            _check(got, counts, top, what=f"n={n}")
        for g in np.flatnonzero(col_len == 0)[:3]:
            top = _tops(n)[-1]
            idx, val = R.neighbours(first=int(g), count=1, top=top)
            np.testing.assert_array_equal(idx[0], [h for h in range(top + 1) if h != g][:top])
            assert not val.any()
        if n == 600:   # subranges: the matching slice of the full result
            for first, count in ((0, n), (1, 1), (n - 1, 1), (250, 20)):
                _check(R.neighbours(first=first, count=count, top=5), counts, 5, first, count, what=f"[{first}, +{count})")
    finally:
        R.close()


@pytest.mark.gpu
@pytest.mark.parametrize("stride", (1, 63, 64, 65))
def test_strides_around_the_rank_block(gpu, stride):
    """65 genomes whose columns have 1, 63, 64 and 65 slots: the rebuilt rows end inside, at and one past a block of 64 ranks."""
    from sketchy_amd import api
    ref, col_len, counts = _case(65, stride)
    R = api.ReferenceSketch(ref, col_len)
    try:
        for top in (1, 5, 64):
            _check(R.neighbours(top=top), counts, top, what=f"stride={stride}")
    finally:
        R.close()


@pytest.mark.gpu
def test_duplicates_put_the_excluded_genome_on_the_threshold(gpu):
    """Five identical columns spread over 257 genomes: each one's row lists the other four in index order with shared = the length --
    self ties with all of them and sits exactly on the selection threshold (at top = 4 the threshold count is the duplicates' own)."""
    from sketchy_amd import api
    base, col_len, _ = _case(257)
    ref = base.copy()
    dup = (0, 3, 128, 255, 256)
    ref[list(dup)] = base[40]
    col_len = col_len.copy()
    col_len[list(dup)] = S
    counts = nc.pair_counts(_cols(ref, col_len))
    same = [h for h in range(257) if col_len[h] == S and np.array_equal(ref[h], ref[40])]   # (a clone tree may hold more copies)
    assert set(dup) <= set(same)
    R = api.ReferenceSketch(ref, col_len)
    try:
        for top in (1, 3, 4, 5, 64):
            got = R.neighbours(top=top)
            _check(got, counts, top)
            for g in dup:
                others = [h for h in same if h != g]
                np.testing.assert_array_equal(got[0][g, :len(others)], others[:top])
                assert (got[1][g, :len(others)] == S).all()
    finally:
        R.close()


def _lifted_case():
    """65 genomes; some hold 0xFF..FE and 0xFF..FF at the end of their column: both, one, none -- also at the end of a short column"""
    base, col_len, _ = _case(65)
    ref, col_len = base.copy(), col_len.copy()
    for g in (0, 9, 32, 64):
        ref[g, S - 2:] = (FE, FF)
    for g in (1, 10, 63):
        ref[g, S - 1] = FF
    for g in (2, 34):
        ref[g, S - 1] = FE
    assert col_len[19] == S - 123 and col_len[12] == 1
    ref[19, S - 125:S - 123] = (FE, FF)
    ref[12, 0] = FF
    return ref, col_len


@pytest.mark.gpu
def test_lifted_hashes_count_between_genomes_that_hold_the_same_value(gpu):
    from sketchy_amd import api
    ref, col_len = _lifted_case()
    cols = _cols(ref, col_len)
    counts = nc.pair_counts(cols)
    plain = nc.pair_counts([c[c < FE] for c in cols])
    assert counts[0, 9] == plain[0, 9] + 2 and counts[0, 1] == plain[0, 1] + 1 and counts[1, 2] == plain[1, 2] and counts[12, 63] == 1
    R = api.ReferenceSketch(ref, col_len)
    try:
        for top in (1, 5, 64):
            _check(R.neighbours(top=top), counts, top)
    finally:
        R.close()


@pytest.mark.gpu
@pytest.mark.parametrize("sizes", ((3, 70), (70, 513, 3)))
def test_species_rank_among_themselves(gpu, sizes):
    """Species of unequal size: indices are local, nothing of another species appears (the oracle's counts are per species), `top` is
    bounded per species -- the species of 3 accepts 2 and refuses 3."""
    from sketchy_amd import _lib, api
    refs, _, _ = workload_species(sizes, S, 3, read_len=400, genome_len=40000, rng_seed=61)
    R = api.ReferenceSketch([r["ref"] for r in refs])
    try:
        for sp, n in enumerate(sizes):
            counts = nc.pair_counts(list(refs[sp]["ref"]))
            for top in sorted({1, min(5, n - 1), min(n - 1, 64)}):
                got = R.neighbours(top=top, species=sp)
                assert got[0].max() < n
                _check(got, counts, top, what=f"species {sp}")
        small = sizes.index(3)
        with pytest.raises(ValueError, match="top"):
            R.neighbours(top=3, species=small)
        idx, val = np.zeros((3, 3), np.uint32), np.zeros((3, 3), np.uint32)
        rc = _lib.load().skx_ref_neighbours(R._h, small, 0, 3, 3, idx.ctypes.data_as(C.c_void_p), val.ctypes.data_as(C.c_void_p), None)
        assert rc == _lib.ERR_INVALID and re.search(r"\btop_k\b", _lib.load().skx_last_error().decode())
    finally:
        R.close()


@pytest.mark.gpu
def test_chunks_and_the_rebuilt_rows(gpu, tmp_path):
    """A child process on the experiments build with chunks of 32 genomes: (a) the 70-genome species of a three-species reference, the
    mixed-length 65-genome case and the lifted-hash case give the rows of the uncut call and of the oracle; (b) the rebuilt query rows
    are the columns: ascending, zero-padded, the lifted hashes appended in ascending order, lengths as given."""
    from sketchy_amd import api
    refs, _, _ = workload_species((70, 513, 3), S, 3, read_len=400, genome_len=40000, rng_seed=61)
    ref65, len65, counts65 = _case(65)
    lref, llen = _lifted_case()
    cases = [([r["ref"] for r in refs], [np.full(len(r["ref"]), S, np.uint32) for r in refs]), ([ref65], [len65]), ([lref], [llen])]
    arrays = dict(n_cases=len(cases))
    for i, (mats, lens) in enumerate(cases):
        arrays[f"n_species{i}"], arrays[f"top{i}"] = len(mats), 5
        for sp, (m, c) in enumerate(zip(mats, lens)):
            arrays[f"ref{i}_{sp}"], arrays[f"len{i}_{sp}"] = m, c
    src, dst = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    np.savez(src, **arrays)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "neighbours_worker.py"), src, dst], env=exp_env(SKX_NEIGHBOUR_CHUNK=32),
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    z = np.load(dst)
    R = api.ReferenceSketch(cases[0][0])
    try:
        uncut = R.neighbours(top=5, species=0)
    finally:
        R.close()
    np.testing.assert_array_equal(z["idx0_0"], uncut[0])
    np.testing.assert_array_equal(z["val0_0"], uncut[1])
    _check((z["idx0_0"], z["val0_0"]), nc.pair_counts(list(refs[0]["ref"])), 5, what="chunks of 32 of 70")
    _check((z["idx1_0"], z["val1_0"]), counts65, 5, what="chunks of 32 of 65, mixed lengths")
    _check((z["idx2_0"], z["val2_0"]), nc.pair_counts(_cols(lref, llen)), 5, what="chunks of 32 of 65, lifted hashes")
    for i, (mats, lens) in enumerate(cases):
        for sp, (m, c) in enumerate(zip(mats, lens)):
            want = np.where(np.arange(m.shape[1])[None, :] < c[:, None], m, np.uint64(0))
            np.testing.assert_array_equal(z[f"rlen{i}_{sp}"], c, err_msg=f"case {i} species {sp} lengths")
            np.testing.assert_array_equal(z[f"rows{i}_{sp}"], want, err_msg=f"case {i} species {sp} rows")
    rows, rlen = z["rows2_0"], z["rlen2_0"]
    assert tuple(rows[0, rlen[0] - 2:rlen[0]]) == (FE, FF) and rows[1, rlen[1] - 1] == FF and rows[2, rlen[2] - 1] == FE
    assert tuple(rows[19, S - 125:S - 122]) == (FE, FF, 0) and rows[12, 0] == FF


@pytest.mark.gpu
def test_cross_check_against_rank_sketches_of_a_reference_without_the_genome(gpu):
    """No oracle in between: for three genomes g, skx_rank_sketches of column g against a reference built WITHOUT g gives neighbours(g)
    once the indices >= g are mapped up by one."""
    from sketchy_amd import api
    ref, col_len, _ = _case(65)
    R = api.ReferenceSketch(ref, col_len)
    try:
        for g in (0, 19, 64):   # (19: a short column)
            keep = np.arange(65) != g
            R1 = api.ReferenceSketch(np.ascontiguousarray(ref[keep]), col_len[keep], s=S)
            try:
                idx, val = R1.rank_sketches(ref[g:g + 1], col_len[g:g + 1], top=7)
            finally:
                R1.close()
            got = R.neighbours(first=g, count=1, top=7)
            np.testing.assert_array_equal(got[0][0], idx[0, 0] + (idx[0, 0] >= g))
            np.testing.assert_array_equal(got[1][0], val[0, 0])
    finally:
        R.close()


@pytest.mark.gpu
def test_codes_are_the_consensus_of_the_returned_rows(gpu):
    """want_codes: the codes are consensus_rows of the returned idx; on a table whose votes all tie (every genome its own code in one
    column, two alternating codes under an even `top` in another) the smallest code wins."""
    from sketchy_amd import api
    ref, col_len, _ = _case(65)
    rng = np.random.default_rng(5)
    table = np.stack([rng.integers(0, 4, 65), rng.permutation(65) + 100, np.arange(65) % 2 + 7], axis=1).astype(np.uint32)
    R = api.ReferenceSketch(ref, col_len)
    try:
        with pytest.raises(ValueError, match="genotype"):
            R.neighbours(top=3, want_codes=True)
        R.set_genotypes(table)
        for top in (1, 4, 5, 64):
            idx, val, codes = R.neighbours(top=top, want_codes=True)
            plain = R.neighbours(top=top)
            np.testing.assert_array_equal(idx, plain[0])
            np.testing.assert_array_equal(val, plain[1])
            np.testing.assert_array_equal(codes, R.consensus_rows(idx))
            np.testing.assert_array_equal(codes[:, 1], table[idx, 1].min(axis=1))   # every vote ties: the smallest code
            want0 = [int(np.argmax(np.bincount(table[row, 0]))) for row in idx]   # (argmax: the first, so the smallest, of the most frequent)
            np.testing.assert_array_equal(codes[:, 0], want0)
        part = R.neighbours(first=60, count=5, top=5, want_codes=True)
        full = R.neighbours(top=5, want_codes=True)
        for a, b in zip(part, full):
            np.testing.assert_array_equal(a, b[60:])
    finally:
        R.close()


# ---- CLI on the real library: the text the host's own path prints for the same file (tests/test_neighbours_cpu.py)
@pytest.fixture(scope="module")
def files(tmp_path_factory):
    return nc.write_cli_files(tmp_path_factory.mktemp("neighbours_cli"))


def _cli(*args):
    p = subprocess.run([BIN, *args], capture_output=True)
    return p.returncode, p.stdout.decode(), p.stderr.decode()


@pytest.mark.gpu
def test_cli_on_the_library_prints_the_text_of_the_host_path(gpu, files):
    msh, tsv = files
    assert "skx_ref_neighbours" in subprocess.check_output(["nm", "-D", "--undefined-only", BIN], text=True)
    rc, out, err = _cli("neighbours", "-r", msh, "-t", "3")
    assert rc == 0 and out == nc.expected_rows(3, False), err
    rc, out, err = _cli("neighbours", "-r", msh, "-g", tsv, "-t", "39", "-H")
    assert rc == 0 and out == "sketch_id\tneighbour_id\tshared_hashes\tmlst\tres\n" + nc.expected_rows(39, True), err
    for top in (1, 3, 39):
        rc, out, err = _cli("neighbours", "-r", msh, "-g", tsv, "-c", "-t", str(top))
        assert rc == 0 and out == nc.expected_consensus(top), (top, err)
    for top in (2, 3):
        rc, out, err = _cli("neighbours", "-r", msh, "-g", tsv, "-S", "-t", str(top))
        assert rc == 0 and out == nc.expected_summary(top), (top, err)
    rc, out, err = _cli("neighbours", "-r", msh, "-t", "40")
    assert rc == 2 and out == "", (rc, err)
