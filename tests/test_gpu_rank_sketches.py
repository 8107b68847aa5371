"""skx_rank_sketches / skx_predict_groups on the device: per query sketch and species the first `top` genomes of
(shared hashes desc, index asc) -- Sketchy::_shared_hashes' tail (src/sketchy.rs:304-312) for many pooled sketches in one call --
and offline `predict` over several inputs.

Expected values come from the oracle alone: counts from orc.common_hashes(ref_row[:col_len], query), rows from
orc.stable_rank(counts of the species)[:top]; pooled sketches from the heap sketcher over a group's records joined with `N`.
Everything is integer: compared exactly."""
import collections
import ctypes as C
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from helpers import exp_env, pack_reads, unpack_reads, workload, workload_species
from mshio import write_msh
from oracle import oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "sketchy_amd", "sketchy-hip")
S = 1000
SIZES = (1, 3, 64, 65, 513, 1100)   # one word, a word boundary, a rank-group boundary (512), several sweep tiles (256)
TOPS = (1, 2, 5, 16, 17, 64)


def _tops(n):
    return sorted({t for t in TOPS + (n,) if t <= min(n, 64)})


def _counts(ref, col_len, queries, qlen):
    return np.array([[orc.common_hashes(ref[g, :col_len[g]], queries[q, :qlen[q]]) for g in range(len(ref))]
                     for q in range(len(queries))], np.uint32).reshape(len(queries), len(ref))


def _rows(counts, species, top):
    """[n_query, n_species, top] (idx, shared) of the oracle's stable rank per species, indices local to the species"""
    nq = len(counts)
    idx, val = np.zeros((nq, len(species), top), np.uint32), np.zeros((nq, len(species), top), np.uint32)
    g0 = 0
    for sp, n in enumerate(species):
        for q in range(nq):
            c = counts[q, g0:g0 + n]
            order = orc.stable_rank(c.astype(np.uint64))[:top]
            idx[q, sp], val[q, sp] = order, c[order]
        g0 += n
    return idx, val


def _queries(ref, col_len, bases, offsets, s, n_groups=30):
    """~40 query sketches: pooled read groups, the first genomes' own columns (count = col_len), an empty one, one whose hashes all
    exceed the reference's largest (no candidates) and one shorter than the stride"""
    reads = unpack_reads(bases, offsets)
    per = max(1, len(reads) // n_groups)
    rows = [orc.sketch(b"N".join(reads[i * per:(i + 1) * per]), 16, 0, s) for i in range(n_groups)]
    rows += [ref[g, :col_len[g]] for g in range(min(len(ref), 5))]
    rows.append(np.zeros(0, np.uint64))
    top = np.uint64(max(int(ref[g, col_len[g] - 1]) for g in range(len(ref))))
    assert int(top) < 2 ** 63
    rows.append(top + np.arange(1, 12, dtype=np.uint64) * np.uint64(3))
    rows.append(rows[0][:37])
    q, qlen = np.zeros((len(rows), s), np.uint64), np.array([len(r) for r in rows], np.uint32)
    for i, r in enumerate(rows):
        q[i, :len(r)] = r
    return q, qlen


@functools.lru_cache(maxsize=None)
def _case(n_genomes, s=S):
    ref, bases, offsets = workload(n_genomes, s, 900, read_len=400, genome_len=40000, rng_seed=500 + n_genomes)
    col_len = ref["col_len"].copy()
    col_len[np.arange(n_genomes) % 7 == 5] = s - 123   # (genomes from index 5 on: some shorter columns)
    q, qlen = _queries(ref["ref"], col_len, bases, offsets, s)
    counts = _counts(ref["ref"], col_len, q, qlen)
    for a in (ref["ref"], col_len, q, qlen, counts):
        a.setflags(write=False)
    return ref["ref"], col_len, q, qlen, counts


def _check(got, counts, species, top, what=""):
    idx, val = _rows(counts, species, top)
    np.testing.assert_array_equal(got[1], val, err_msg=f"{what} top={top} shared")
    np.testing.assert_array_equal(got[0], idx, err_msg=f"{what} top={top} idx")
    if len(got) > 2:
        np.testing.assert_array_equal(got[2], counts, err_msg=f"{what} top={top} common")


@pytest.mark.gpu
@pytest.mark.parametrize("n_genomes", SIZES)
def test_sizes(gpu, n_genomes):
    """Rows and counts for ~40 queries in one call at every `top`; own-column queries count col_len = 1000 > 448 (the counter's block)
    and > 255 (a byte of the radix select); the old kernel's counts (skx_common_hashes) agree."""
    from sketchy_amd import api
    ref, col_len, q, qlen, counts = _case(n_genomes)
    assert counts.max() == S and counts[len(q) - 3].max() == 0 and counts[len(q) - 2].max() == 0
    R = api.ReferenceSketch(ref, col_len)
    try:
        for top in _tops(n_genomes):
            _check(R.rank_sketches(q, qlen, top=top, want_common=True), counts, [n_genomes], top, what=f"n={n_genomes}")
        got = R.rank_sketches(q, qlen, top=1)   # (without the counts)
        assert len(got) == 2
        _check(got, counts, [n_genomes], 1)
        np.testing.assert_array_equal(R.rank_sketches(q, qlen, top=1, want_common=True)[2], R.common_hashes(q, qlen))
        full = R.rank_sketches(ref, top=1)       # query_len = None: whole rows; as many queries as genomes
        assert full[1][0, 0, 0] == S
    finally:
        R.close()


@pytest.mark.gpu
def test_counts_above_4096(gpu):
    """s = 5 000, 64 genomes, genomes' own columns as queries: counts of 5 000 (two significant bytes, beyond 12 bits)."""
    from sketchy_amd import api
    s = 5000
    ref, bases, offsets = workload(64, s, 200, read_len=400, genome_len=40000, rng_seed=91)
    col_len = ref["col_len"]
    reads = unpack_reads(bases, offsets)
    rows = [ref["ref"][0], ref["ref"][63], ref["ref"][17], orc.sketch(b"N".join(reads), 16, 0, s)]
    q, qlen = np.zeros((len(rows), s), np.uint64), np.array([len(r) for r in rows], np.uint32)
    for i, r in enumerate(rows):
        q[i, :len(r)] = r
    counts = _counts(ref["ref"], col_len, q, qlen)
    assert counts.max() == s > 4096
    R = api.ReferenceSketch(ref["ref"], col_len)
    try:
        for top in (1, 5, 64):
            _check(R.rank_sketches(q, qlen, top=top, want_common=True), counts, [64], top)
    finally:
        R.close()


@pytest.mark.gpu
def test_ties_across_the_cut(gpu):
    """200 genomes = 20 distinct columns x 10 copies, interleaved: every count occurs ten times, so rank `top` and rank `top + 1` tie
    and the cut goes by index.  A query none of whose hashes any genome holds: indices 0 .. top-1 with 0."""
    from sketchy_amd import api
    base, bases, offsets = workload(20, S, 300, read_len=400, genome_len=40000, rng_seed=33)
    ref = np.ascontiguousarray(base["ref"][np.arange(200) % 20])
    col_len = np.full(200, S, np.uint32)
    q, qlen = _queries(ref, col_len, bases, offsets, S, n_groups=6)
    held = set(ref.ravel().tolist())
    absent = np.array([h for h in range(int(ref.min()) + 1, int(ref.min()) + 400) if h not in held][:50], np.uint64)
    assert len(absent) == 50 and absent.max() < ref.max()   # candidates (<= the reference's largest hash) that hit nothing
    q = np.concatenate([q, np.zeros((1, S), np.uint64)])
    q[-1, :50] = absent
    qlen = np.concatenate([qlen, [50]]).astype(np.uint32)
    counts = _counts(ref, col_len, q, qlen)
    assert counts[-1].max() == 0 and counts[0].max() > 0
    R = api.ReferenceSketch(ref, col_len)
    try:
        for top in (1, 7, 16, 33):
            idx, val = _rows(counts, [200], top + 1)
            assert (val[:, 0, top - 1] == val[:, 0, top]).all()   # the tie across the cut, on the expected data
            got = R.rank_sketches(q, qlen, top=top, want_common=True)
            _check(got, counts, [200], top)
            np.testing.assert_array_equal(got[0][-1, 0], np.arange(top))
            assert (got[1][-1] == 0).all()
    finally:
        R.close()


@pytest.mark.gpu
def test_three_species(gpu):
    """Species of 3, 70 and 513 genomes: rows per species with local indices, counts concatenated in species order."""
    from sketchy_amd import api
    sizes = (3, 70, 513)
    refs, bases, offsets = workload_species(sizes, S, 300, read_len=400, genome_len=40000, rng_seed=61)
    allref = np.concatenate([r["ref"] for r in refs])
    col_len = np.full(len(allref), S, np.uint32)
    q, qlen = _queries(allref, col_len, bases, offsets, S, n_groups=12)
    q = np.concatenate([q, refs[1]["ref"][:2], refs[2]["ref"][511:513]])
    qlen = np.concatenate([qlen, [S] * 4]).astype(np.uint32)
    counts = _counts(allref, col_len, q, qlen)
    R = api.ReferenceSketch([r["ref"] for r in refs])
    try:
        got = R.rank_sketches(q, qlen, top=3, want_common=True)
        assert got[0].shape == (len(q), 3, 3)
        _check(got, counts, sizes, 3)
        assert got[0][-1, 2, 0] == 512 and got[1][-1, 2, 0] == S   # genome 512 of the third species, by its local index
    finally:
        R.close()


@pytest.mark.gpu
@pytest.mark.parametrize("rare", (0, 2, None))
def test_several_passes_index_on_and_off(gpu, rare):
    """stream_query_rows = s cuts the 40 queries into many passes; with no rare-hash index, one that lists hashes of at most two
    genomes, and the default one.  Rows and counts as the uncut run and as the oracle."""
    from sketchy_amd import api
    ref, col_len, q, qlen, counts = _case(513)
    rare_default = api.get_option("rare_hash_genomes")
    try:
        if rare is not None:
            api.set_option("rare_hash_genomes", rare)
        R = api.ReferenceSketch(ref, col_len)
    finally:
        api.set_option("rare_hash_genomes", rare_default)
    try:
        if rare == 0:
            assert R.rare_index["keys"] == 0
        uncut = R.rank_sketches(q, qlen, top=5, want_common=True)
        try:
            api.set_option("stream_query_rows", S)
            cut = R.rank_sketches(q, qlen, top=5, want_common=True)
        finally:
            api.set_option("stream_query_rows", 0)
        for a, b in zip(cut, uncut):
            np.testing.assert_array_equal(a, b)
        _check(cut, counts, [513], 5, what=f"rare={rare}")
    finally:
        R.close()


@pytest.mark.gpu
def test_predict_groups(gpu):
    """Groups of 0, 1, 2, 5 and 65 records of 0 .. 4 000 bases (one with non-ACGT) at top = 5: rows of the oracle's pooled sketch per
    group; the optional sketches are skx_sketch_groups'."""
    from sketchy_amd import api
    sizes = (0, 1, 2, 5, 65)
    ref, bases, offsets = workload(64, S, sum(sizes), read_len=4000, genome_len=40000, rng_seed=71, err=0.01)
    rng = np.random.default_rng(72)
    lens = rng.integers(0, 4001, sum(sizes))
    lens[[0, 4]] = (4000, 0)
    records = [r[:int(m)] for r, m in zip(unpack_reads(bases, offsets), lens)]
    records[2] = records[2][:50] + b"NNRYK-" + records[2][50:].lower()
    first = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32)
    b, o = pack_reads(records)
    q, qlen = np.zeros((len(sizes), S), np.uint64), np.zeros(len(sizes), np.uint32)
    for g in range(len(sizes)):
        recs = records[int(first[g]):int(first[g + 1])]
        if recs:
            h = orc.sketch(b"N".join(recs), 16, 0, S)
            q[g, :len(h)], qlen[g] = h, len(h)
    counts = _counts(ref["ref"], ref["col_len"], q, qlen)
    assert counts[0].max() == 0 and counts[4].max() > 255
    R = api.ReferenceSketch(ref["ref"], ref["col_len"])
    try:
        idx, val, sk, sl, vk = R.predict_groups(b, o, first, top=5, want_sketches=True, want_valid_kmers=True)
        _check((idx, val), counts, [64], 5)
        np.testing.assert_array_equal(idx[0, 0], np.arange(5))   # the empty group: no hashes, rows 0 .. 4 with 0
        pooled = api.sketch_groups(b, o, first, k=16, seed=0, s=S, want_valid_kmers=True)
        for a, e in zip((sk, sl, vk), pooled):
            np.testing.assert_array_equal(a, e)
        np.testing.assert_array_equal(sl, qlen)
        np.testing.assert_array_equal(sk, q)
        plain = R.predict_groups(b, o, first, top=1)
        assert len(plain) == 2
        _check(plain, counts, [64], 1)
    finally:
        R.close()


@functools.lru_cache(maxsize=None)
def _groups_input():
    sizes = (0, 1, 2, 5, 65, 0, 3)
    ref, bases, offsets = workload(64, S, sum(sizes), read_len=4000, genome_len=40000, rng_seed=71, err=0.01)
    rng = np.random.default_rng(72)
    lens = rng.integers(0, 4001, sum(sizes))
    lens[[0, 4]] = (4000, 0)
    records = [r[:int(m)] for r, m in zip(unpack_reads(bases, offsets), lens)]
    first = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32)
    q, qlen = np.zeros((len(sizes), S), np.uint64), np.zeros(len(sizes), np.uint32)
    for g in range(len(sizes)):
        recs = records[int(first[g]):int(first[g + 1])]
        if recs:
            h = orc.sketch(b"N".join(recs), 16, 0, S)
            q[g, :len(h)], qlen[g] = h, len(h)
    return ref, records, first, q, qlen, _counts(ref["ref"], ref["col_len"], q, qlen)


def _topk_cases():
    """synthetic count rows for the selection kernel alone: bounds of one, three and four significant bytes, few distinct values
    (ties in every byte, across the cut), values that differ in one byte only, 1 100 genomes (several sweep tiles, pad genomes)"""
    rng = np.random.default_rng(404)
    cases = []
    for bound in (200, 70000, 0x01000000, 0xFFFFFFFF):
        rows = [rng.choice(rng.integers(0, bound + 1, 40, dtype=np.uint64), 1100),          # 40 distinct values: ties everywhere
                rng.integers(0, bound + 1, 1100, dtype=np.uint64),                           # (nearly) all distinct
                np.full(1100, bound, np.uint64),                                             # all equal to the bound
                (np.uint64(bound) >> np.uint64(8)) * np.uint64(256) + rng.integers(0, 3, 1100).astype(np.uint64)]  # low byte only
        rows[3] = np.minimum(rows[3], np.uint64(bound))
        cases.append((bound, np.array(rows).astype(np.uint32)))
    return cases


@pytest.mark.gpu
def test_chunks_of_groups_and_the_wide_bytes_of_the_selection(gpu, tmp_path):
    """A child process on the experiments build: (a) predict_groups with the groups cut into chunks of 2 (SKX_PREDICT_GROUPS; seven
    groups, two of them empty, chunks that start in the middle of the records): rows, sketches and k-mer counts as the oracle's
    and as one chunk's; (b) row_topk_kernel alone on synthetic counts whose bound has three and four significant bytes -- every
    byte pass of the radix select -- against orc.stable_rank."""
    ref, records, first, q, qlen, counts = _groups_input()
    b, o = pack_reads(records)
    cases = _topk_cases()
    tops = (1, 5, 64)
    arrays = dict(ref=ref["ref"], col_len=ref["col_len"], bases=b, offsets=o, first=first, top=5, n_topk=len(cases), tops=np.array(tops))
    for i, (bound, c) in enumerate(cases):
        arrays[f"counts{i}"], arrays[f"bound{i}"] = c, np.uint64(bound)
    src, dst = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    np.savez(src, **arrays)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "rank_sketches_worker.py"), src, dst], env=exp_env(SKX_PREDICT_GROUPS=2),
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    z = np.load(dst)
    _check((z["idx"], z["val"]), counts, [64], 5, what="chunks of 2 groups")
    np.testing.assert_array_equal(z["sl"], qlen)
    np.testing.assert_array_equal(z["sk"], q)
    valid = [sum(len(orc.kmer_hashes(rec, 16, 0)[0]) for rec in records[int(first[g]):int(first[g + 1])]) for g in range(len(first) - 1)]
    np.testing.assert_array_equal(z["vk"], np.array(valid, np.uint64))
    for i, (bound, c) in enumerate(cases):
        assert int(c.max()) <= bound
        for top in tops:
            idx, val = _rows(c, [c.shape[1]], top)
            np.testing.assert_array_equal(z[f"tv{i}_{top}"], val[:, 0], err_msg=f"bound={bound} top={top} values")
            np.testing.assert_array_equal(z[f"ti{i}_{top}"], idx[:, 0], err_msg=f"bound={bound} top={top} idx")


@pytest.mark.gpu
def test_argument_checks_with_a_reference_handle(gpu):
    """What needs a handle and so a device: an unsorted row is SKX_ERR_UNSORTED, top_k above the smallest species and every NULL
    required pointer SKX_ERR_INVALID, a query_len above the stride SKX_ERR_INVALID; no queries / no groups: SKX_OK, outputs untouched."""
    from sketchy_amd import _lib, api
    L = _lib.load()
    R = api.ReferenceSketch([np.arange(1, 13, dtype=np.uint64).reshape(3, 4), np.arange(21, 41, dtype=np.uint64).reshape(5, 4)])

    def p(a):
        return None if a is None else a.ctypes.data_as(C.c_void_p)

    def rank(query=np.array([[1, 2, 3, 4], [5, 6, 8, 7]], np.uint64), query_len=np.array([4, 3], np.uint32), n_query=2, top_k=1,
             top_idx="ok", top_shared="ok"):
        ti = np.zeros((2, 2, 64), np.uint32) if isinstance(top_idx, str) else top_idx
        tv = np.zeros((2, 2, 64), np.uint32) if isinstance(top_shared, str) else top_shared
        rc = L.skx_rank_sketches(R._h, p(query), p(query_len), n_query, 4, top_k, p(ti), p(tv), None)
        return rc, L.skx_last_error().decode()

    def predict(n_records=1, n_groups=1, top_k=1, idx=None):
        bases, offsets, first = np.frombuffer(b"ACGTACGTACGTACGTACGT", np.uint8).copy(), np.array([0, 20], np.uint64), np.array([0, n_records], np.uint32)
        idx = np.zeros(128, np.uint32) if idx is None else idx
        rc = L.skx_predict_groups(R._h, p(bases), p(offsets), n_records, p(first), n_groups, top_k, p(idx), p(np.zeros(128, np.uint32)), None, None, None)
        return rc, L.skx_last_error().decode()
    try:
        rc, msg = rank()   # (query_len 3: the second row's first three are ascending)
        assert rc == _lib.OK, (rc, msg)
        rc, msg = rank(query_len=np.array([4, 4], np.uint32))
        assert rc == _lib.ERR_UNSORTED and "query 1" in msg, (rc, msg)
        for top, ok in ((3, True), (4, False), (5, False)):   # the smallest species has 3 genomes
            rc, msg = rank(top_k=top)
            assert (rc == _lib.OK) if ok else (rc == _lib.ERR_INVALID and re.search(r"\btop_k\b", msg)), (top, rc, msg)
            rc, msg = predict(top_k=top)
            assert (rc == _lib.OK) if ok else (rc == _lib.ERR_INVALID and re.search(r"\btop_k\b", msg)), (top, rc, msg)
        for name in ("query", "query_len", "top_idx", "top_shared"):
            rc, msg = rank(**{name: None})
            assert rc == _lib.ERR_INVALID and "NULL" in msg, (name, rc, msg)
        rc, msg = rank(query_len=np.array([4, 5], np.uint32))
        assert rc == _lib.ERR_INVALID and "q_stride" in msg, (rc, msg)
        untouched = np.full((2, 2, 64), 77, np.uint32)
        rc, msg = rank(n_query=0, top_idx=untouched)
        assert rc == _lib.OK and (untouched == 77).all(), (rc, msg)
        rc, msg = predict(n_groups=0)   # (one record, no group to hold it)
        assert rc == _lib.ERR_INVALID and "group_first" in msg, (rc, msg)
        untouched = np.full(128, 77, np.uint32)
        rc, msg = predict(n_records=0, n_groups=0, idx=untouched)
        assert rc == _lib.OK and (untouched == 77).all(), (rc, msg)
        # the wrapper: rows without a slot are empty queries
        idx, val = R.rank_sketches(np.zeros((3, 0), np.uint64), top=2)
        np.testing.assert_array_equal(idx, np.broadcast_to(np.arange(2, dtype=np.uint32), (3, 2, 2)))
        assert not val.any()
    finally:
        R.close()


# ---- CLI: offline predict over several inputs
def _cli(*args):
    p = subprocess.run([BIN, *args], capture_output=True)
    return p.returncode, p.stdout.decode(), p.stderr.decode()


@pytest.fixture(scope="module")
def cli_inputs(tmp_path_factory):
    d = tmp_path_factory.mktemp("rank_cli")
    ref, bases, offsets = workload(64, S, 5701, read_len=400, genome_len=40000, rng_seed=77)
    names = [f"genome{i:02d}.fa" for i in range(64)]
    msh, tsv = str(d / "ref.msh"), str(d / "geno.tsv")
    write_msh(msh, names, ref["ref"], kmer=16, seed=0, lengths=[40000] * 64)
    with open(tsv, "w") as f:
        f.write("id\tmlst\n" + "".join(f"{nm}\tST{i % 7}\n" for i, nm in enumerate(names)))
    reads = unpack_reads(bases, offsets)
    parts = [reads[:5000], reads[5000:5001], reads[5001:]]
    files = []
    for j, part in enumerate(parts):
        files.append(str(d / f"sample{j}.fq"))
        with open(files[-1], "w") as f:
            f.write("".join(f"@r{i}\n{r.decode()}\n+\n{'I' * len(r)}\n" for i, r in enumerate(part)))
    return ref["ref"], names, msh, tsv, files, parts


def _oracle_block(ref, names, reads, top, consensus):
    pooled = orc.sketch(b"N".join(reads), 16, 0, S)
    common = np.array([orc.common_hashes(ref[g], pooled) for g in range(len(ref))])
    order = orc.stable_rank(common.astype(np.uint64))[:top]
    if not consensus:
        return "".join(f"{len(reads)}\t{names[g]}\t{common[g]}\tST{g % 7}\n" for g in order)
    votes = collections.Counter(f"ST{g % 7}" for g in order)
    best = max(votes.values())
    return f"{len(reads)}\t-\t-\t{min(v for v, c in votes.items() if c == best)}\n"   # (ties: the smallest value, as the host's)


@pytest.mark.gpu
@pytest.mark.parametrize("extra", (("-t", "5", "-H"), ("-t", "5", "-H", "-l", "600"), ("-c", "-t", "5")), ids=("top5", "limit", "consensus"))
def test_cli_predict_over_three_inputs(gpu, cli_inputs, extra):
    """Three FASTQ files of 5 000, 1 and 700 reads: the output of one run over all three is the three single-file outputs one after
    the other (the header once); the first file's block is the oracle's text."""
    ref, names, msh, tsv, files, parts = cli_inputs
    header = "reads\tsketch_id\tshared_hashes\tmlst\n" if "-H" in extra else ""
    blocks = []
    for f in files:
        rc, out, err = _cli("predict", "-r", msh, "-g", tsv, "-i", f, *extra)
        assert rc == 0, err
        assert out.startswith(header)
        blocks.append(out[len(header):])
    rc, out, err = _cli("predict", "-r", msh, "-g", tsv, "-i", *files, *extra)
    assert rc == 0, err
    assert out == header + "".join(blocks)
    limit = 600 if "-l" in extra else 0
    first = parts[0][:limit] if limit else parts[0]
    assert blocks[0] == _oracle_block(ref, names, first, 5, "-c" in extra)
    assert blocks[1].split("\t")[0] == "1" and blocks[2].split("\t")[0] == str(min(700, limit) if limit else 700)


@pytest.mark.gpu
def test_cli_streaming_takes_one_input_and_the_binary_links_the_ranking(gpu, cli_inputs):
    ref, names, msh, tsv, files, parts = cli_inputs
    rc, out, err = _cli("predict", "-r", msh, "-g", tsv, "-s", "-i", files[1], files[2])
    assert rc == 2 and out == "" and "one input" in err, (rc, err)
    und = subprocess.check_output(["nm", "-D", "--undefined-only", BIN], text=True)
    assert "skx_rank_sketches" in und
