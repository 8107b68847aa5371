"""Expectations for the breadth of a stream (skx_stream_enable_coverage), from the oracle alone, and the builders the coverage tests
share (tests/test_coverage_cpu.py, tests/test_gpu_coverage.py, tests/coverage_worker.py).

    covered[g] = |{h in column g : some read pushed so far has h in its bottom-s sketch}|

read by read orc.sketch(seq, k, seed, s) -- truncation to s first --, a running set of seen hashes, and at the requested read counts
covered[g] = |col(g) & seen| with numpy.  Nothing of the library is involved."""
import functools

import numpy as np

import hash_classes as hc
from helpers import unpack_reads

K, SEED = hc.K, hc.SEED


def expected_coverage(refs, col_lens, bases, offsets, s, at):
    """{n_reads: uint32 [n_genomes]} for every read count in `at` (species one after the other, as every genome-indexed array)"""
    from oracle import oracle as orc
    ref, col_len = np.concatenate(refs), np.concatenate(col_lens)
    valid = np.arange(ref.shape[1])[None, :] < col_len[:, None]
    reads = unpack_reads(bases, offsets)
    at = sorted(set(int(a) for a in at))
    assert at and at[-1] <= len(reads)
    seen, out = set(), {}

    def count():
        have = np.isin(ref, np.fromiter(seen, np.uint64, len(seen))) & valid
        return have.sum(axis=1).astype(np.uint32)
    if at[0] == 0:
        out[0] = count()
    for r, seq in enumerate(reads[:at[-1]]):
        seen.update(int(h) for h in orc.sketch(seq, K, SEED, s))
        if r + 1 in at:
            out[r + 1] = count()
    return out


def expected_rank(covered, species, top):
    """(idx, covered) [n_species, top]: (covered desc, index asc) per species, indices local to the species"""
    idx, val = np.zeros((len(species), top), np.uint32), np.zeros((len(species), top), np.uint32)
    g0 = 0
    for sp, n in enumerate(species):
        c = covered[g0:g0 + n].astype(np.int64)
        order = np.lexsort((np.arange(n), -c))[:top]
        idx[sp], val[sp] = order, c[order]
        g0 += n
    return idx, val


def create_reference(design, rare, s=None, pad_to=None):
    """(ReferenceSketch, refs, col_lens) under the policy rare_hash_genomes = rare, reads sketched with an explicit s (default: the
    first column's length, as the reference binary takes it); pad_to: widen the matrices to that many columns, col_len unchanged"""
    from sketchy_amd import api
    refs, col_lens = hc.build_reference(design)
    if pad_to is not None and pad_to > refs[0].shape[1]:
        refs = [np.ascontiguousarray(np.pad(r, ((0, 0), (0, pad_to - r.shape[1])))) for r in refs]
    s = int(col_lens[0][0]) if s is None else int(s)
    before = api.get_option("rare_hash_genomes")
    api.set_option("rare_hash_genomes", rare)
    try:
        R = api.ReferenceSketch(refs[0], col_lens[0], s=s) if len(refs) == 1 else api.ReferenceSketch(refs, col_lens, s=s)
    finally:
        api.set_option("rare_hash_genomes", before)
    return R, refs, col_lens


# the scattered list of the storage-class cases: tile and rank-group edges, the last genome, the lineage starts, one index twice
ROWS_1300 = np.array([0, 255, 256, 511, 512, 1299, *hc.LINEAGE_STARTS, 256], np.uint32)
CUTS_1300 = (0, 500, 501, 1200)
# the read sketch size of the single-species cases: column 0 of the 64-dense design (the other variants' column 0 is longer; they are
# sketched with 48 as well) -- reads of 300 bases have 285 k-mers, every one of them is truncated
S_SINGLE = 48


@functools.lru_cache(maxsize=None)
def single(n_dense):
    """(design, refs, col_lens, bases, offsets) of hc.single_species(n_dense) and hc.reads of it: 1 200 reads of 300 bases"""
    d = hc.single_species(n_dense)
    refs, col_lens = hc.build_reference(d)
    bases, offsets = hc.reads(d)
    for a in (*refs, *col_lens, bases, offsets):
        a.setflags(write=False)
    return d, refs, col_lens, bases, offsets


@functools.lru_cache(maxsize=None)
def single_expected(n_dense, s, at=CUTS_1300[1:]):
    d, refs, col_lens, bases, offsets = single(n_dense)
    exp = expected_coverage(refs, col_lens, bases, offsets, S_SINGLE if s is None else s, at)
    for v in exp.values():
        v.setflags(write=False)
    return exp


def check_queries(S, exp, species, rows, tops, what=""):
    """coverage(), coverage_rows(rows) and coverage_rank(top) of stream S against the expectation `exp` [n_genomes]"""
    got = S.coverage()
    assert got.dtype == np.uint32
    np.testing.assert_array_equal(got, exp, err_msg=f"{what} coverage")
    np.testing.assert_array_equal(S.coverage_rows(rows), exp[rows], err_msg=f"{what} coverage_rows")
    for top in tops:
        idx, val = expected_rank(exp, species, top)
        gi, gv = S.coverage_rank(top)
        np.testing.assert_array_equal(gv, val, err_msg=f"{what} coverage_rank top={top} covered")
        np.testing.assert_array_equal(gi, idx, err_msg=f"{what} coverage_rank top={top} idx")


def check_pushes(R, species, bases, offsets, cuts, exp, rows, tops, what="", top=1):
    """synchronous pushes cut at `cuts`, the three queries after every cut; returns (rows of the last push, table)"""
    from sketchy_amd import api
    n = len(offsets) - 1
    S = api.SumOfSharedHashes(R, top=top, max_batch_reads=n, max_batch_bases=max(1, len(bases)))
    try:
        S.enable_coverage()
        S.enable_coverage()   # (a second call changes nothing)
        parts = []
        for a, b in zip(cuts[:-1], cuts[1:]):
            parts.append(S.push(bases, offsets[a:b + 1]))
            check_queries(S, exp[b], species, rows, tops, what=f"{what} after {b} reads")
        return parts, S.table()
    finally:
        S.close()


def plain_pushes(R, bases, offsets, cuts, top=1):
    """the same pushes on a stream that never enables coverage"""
    from sketchy_amd import api
    n = len(offsets) - 1
    S = api.SumOfSharedHashes(R, top=top, max_batch_reads=n, max_batch_bases=max(1, len(bases)))
    try:
        parts = [S.push(bases, offsets[a:b + 1]) for a, b in zip(cuts[:-1], cuts[1:])]
        return parts, S.table()
    finally:
        S.close()


def enqueue_batches(S, bases, offsets, cuts, query_after=(), on_query=None):
    """the reads as device batches through enqueue_device (table only); on_query(b) after every cut index in query_after"""
    from sketchy_amd import api
    keep = [api.DeviceBuffer.from_numpy(np.ascontiguousarray(bases))]
    try:
        for i, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
            d_o = api.DeviceBuffer.from_numpy(np.ascontiguousarray(offsets[a:b + 1]))
            keep.append(d_o)
            S.enqueue_device(keep[0].ptr, d_o.ptr, b - a, int(offsets[b] - offsets[a]))
            if i + 1 in query_after and on_query:
                on_query(b)
        S.sync()
    finally:
        for d in keep:
            d.free()
