"""Consensus genotypes on the device: skx_consensus_rows alone, and the codes every stream entry point returns through a bound
output, against a numpy restatement of the semantics (test_consensus_cpu.consensus_ref: the most frequent code among a row's genomes
per column, ties to the smallest code).  The vote is a pure function of the rows, so the stream cases compare the codes with the
restatement applied to the rows a SECOND stream returns for the same reads with nothing bound -- and the bound stream's own rows
with those rows."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from helpers import pack_reads, unpack_reads, workload, workload_species
from mshio import write_msh
from test_consensus_cpu import consensus_of_rows, consensus_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "sketchy_amd", "sketchy-hip")
TOPS = (1, 2, 3, 5, 7, 8, 9, 16, 17, 63, 64)   # the register path (<= 8), the generic one, their boundary
ROWS = (1, 63, 64, 65, 1000)
ALPHABETS = ("two", "three", "distinct", "extreme")


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def make_codes(n_genomes, n_feat, kind, rng):
    if kind == "two":
        return rng.integers(0, 2, (n_genomes, n_feat)).astype(np.uint32)
    if kind == "three":
        return (rng.integers(0, 3, (n_genomes, n_feat)) * 1000 + 7).astype(np.uint32)
    if kind == "distinct":  # every count is 1: the smallest code of the row must win
        return np.stack([rng.permutation(n_genomes) + 10 * f for f in range(n_feat)], axis=1).astype(np.uint32)
    codes = rng.integers(0, 3, (n_genomes, n_feat)).astype(np.uint32)
    codes[:, 0] = np.where(rng.integers(0, 2, n_genomes) == 1, 0xFFFFFFFF, 0)  # "extreme"
    return codes


def tiny_ref(species, api):
    """a reference whose hashes do not matter: `species` collections of four hashes per genome"""
    mats = [(np.arange(n * 4, dtype=np.uint64).reshape(n, 4) * 3 + 1 + 100000 * i) for i, n in enumerate(species)]
    return api.ReferenceSketch(mats if len(mats) > 1 else mats[0])


def random_rows(species, n_rows, top, rng):
    """[n_rows, n_species, top] distinct genomes per row (as a ranking returns them)"""
    return np.stack([np.argsort(rng.random((n_rows, n)), axis=1)[:, :top] for n in species], axis=1).astype(np.uint32)


def n_tied(idx, codes, species):
    """(row, species, column)s whose most frequent code is not alone at the top"""
    base = np.concatenate([[0], np.cumsum(species)])[:-1]
    n = 0
    for r in range(idx.shape[0]):
        for sp in range(idx.shape[1]):
            for f in range(codes.shape[1]):
                c = np.unique(codes[base[sp] + idx[r, sp].astype(np.int64), f], return_counts=True)[1]
                n += int((c == c.max()).sum() > 1)
    return n


# ---------------------------------------------------------------- the operator alone
@pytest.mark.parametrize("n_feat", (1, 3, 16, 64))
@pytest.mark.parametrize("species", ((300,), (70, 129, 64)), ids=("one_species", "three_species"))
def test_operator_against_the_restatement(gpu, species, n_feat):
    from sketchy_amd import api
    rng = np.random.default_rng(1000 * len(species) + n_feat)
    rows = {top: random_rows(species, max(ROWS), top, rng) for top in TOPS}
    for kind in ALPHABETS:
        codes = make_codes(sum(species), n_feat, kind, rng)
        R = tiny_ref(species, api)
        try:
            assert R.n_features == 0
            R.set_genotypes(codes)
            assert R.n_features == n_feat
            for top in TOPS:
                want = consensus_ref(rows[top], codes, species)  # (rows are voted on one by one: a prefix's codes are a prefix)
                if kind == "three" and top in (2, 3, 9):
                    assert n_tied(rows[top][:40], codes, species) > 0, (top, "the case must exercise the tie rule")
                if kind == "distinct":
                    assert n_tied(rows[top][:5], codes, species) == (0 if top == 1 else 5 * len(species) * n_feat)
                for n_rows in ROWS:
                    idx = rows[top][:n_rows] if len(species) > 1 else rows[top][:n_rows, 0]
                    got = R.consensus_rows(idx)
                    assert got.shape == idx.shape[:-1] + (n_feat,) and got.dtype == np.uint32
                    np.testing.assert_array_equal(got.reshape(n_rows, len(species), n_feat), want[:n_rows],
                                                  err_msg=f"{kind} top {top} rows {n_rows}")
        finally:
            R.close()


def test_operator_rows_with_a_repeated_genome(gpu):
    from sketchy_amd import api
    rng = np.random.default_rng(77)
    species = (70, 129, 64)
    codes = make_codes(sum(species), 16, "three", rng)
    R = tiny_ref(species, api)
    try:
        R.set_genotypes(codes)
        for top in (3, 8, 9, 64):
            idx = np.stack([rng.integers(0, n, (200, top)) for n in species], axis=1).astype(np.uint32)  # with replacement
            idx[:, :, -1] = idx[:, :, 0]
            np.testing.assert_array_equal(R.consensus_rows(idx), consensus_ref(idx, codes, species))
            same = np.broadcast_to(idx[:, :, :1], idx.shape).copy()  # one genome top times: its own codes
            base = np.array([0, 70, 199])
            np.testing.assert_array_equal(R.consensus_rows(same), codes[same[:, :, 0].astype(np.int64) + base[None, :]])
    finally:
        R.close()


def test_operator_errors(gpu):
    from sketchy_amd import _lib, api
    L = _lib.load()
    species = (70, 129, 64)
    R = tiny_ref(species, api)
    try:
        idx = random_rows(species, 4, 3, np.random.default_rng(1))
        out = np.full((4, 3, 2), 0xABCD, np.uint32)
        assert L.skx_consensus_rows(R._h, _p(idx), 4, 3, _p(out)) == _lib.ERR_INVALID  # no table yet
        assert "genotype table" in L.skx_last_error().decode()
        codes = make_codes(sum(species), 2, "two", np.random.default_rng(2))
        R.set_genotypes(codes)
        with pytest.raises(_lib.SketchyHipError) as e:
            R.set_genotypes(codes)  # a second table
        assert e.value.code == _lib.ERR_INVALID
        for sp, n in enumerate(species):  # an index out of ITS species' range (in range for a larger one)
            bad = idx.copy()
            bad[2, sp, 1] = n
            assert L.skx_consensus_rows(R._h, _p(bad), 4, 3, _p(out)) == _lib.ERR_INVALID, sp
            assert f"species {sp}" in L.skx_last_error().decode()
        for top in (0, 65):
            assert L.skx_consensus_rows(R._h, _p(idx), 4, top, _p(out)) == _lib.ERR_INVALID
        assert L.skx_consensus_rows(R._h, _p(idx), 0, 3, _p(out)) == _lib.OK
        assert (out == 0xABCD).all()  # nothing above wrote a code
        assert L.skx_consensus_rows(R._h, _p(idx), 4, 3, _p(out)) == _lib.OK
        np.testing.assert_array_equal(out, consensus_ref(idx, codes, species))
    finally:
        R.close()


# ---------------------------------------------------------------- streams
def drive(S, entry, bases, offsets, cuts, top, n_sp, n_feat, bind, null_rows=False):
    """every batch [cuts[i], cuts[i + 1]) through one entry point -> (rows idx [n, n_sp, top] or None, codes [n, n_sp, n_feat] or
    None); bind: give every batch a consensus output; null_rows: (submit / push_device never here) pass no row arrays"""
    from sketchy_amd import api
    n_all = cuts[-1] - cuts[0]
    if entry == "push":
        parts = [S.push(bases, offsets[a:b + 1], want_consensus=bind) for a, b in zip(cuts[:-1], cuts[1:])]
        idx = np.concatenate([p["topk_idx"] for p in parts]).reshape(n_all, n_sp, top)
        return idx, (np.concatenate([p["consensus"] for p in parts]).reshape(n_all, n_sp, n_feat) if bind else None)
    if entry == "submit":
        at = lambda buf, off: C.c_void_p(buf.ptr.value + off)
        hb, ho = api.HostBuffer(len(bases)), api.HostBuffer(len(offsets) * 8)
        hi, hs, hc = api.HostBuffer(n_all * n_sp * top * 4), api.HostBuffer(n_all * n_sp * top * 8), api.HostBuffer(n_all * n_sp * n_feat * 4)
        try:
            hb.view(np.uint8)[:] = bases
            ho.view(np.uint64)[:] = offsets
            hi.view(np.uint32)[:] = 0xFFFFFFFF
            hc.view(np.uint32)[:] = 0xFFFFFFFF
            for a, b in zip(cuts[:-1], cuts[1:]):
                r = a - cuts[0]
                S.submit(hb.ptr, at(ho, a * 8), b - a, None if null_rows else at(hi, r * n_sp * top * 4),
                         None if null_rows else at(hs, r * n_sp * top * 8), consensus=at(hc, r * n_sp * n_feat * 4) if bind else None)
            S.drain()
            idx = None if null_rows else hi.view(np.uint32).reshape(n_all, n_sp, top).copy()
            return idx, (hc.view(np.uint32).reshape(n_all, n_sp, n_feat).copy() if bind else None)
        finally:
            for h in (hb, ho, hi, hs, hc):
                h.free()
    d_b = api.DeviceBuffer.from_numpy(bases)
    bufs, rows = [d_b], []
    try:
        for a, b in zip(cuts[:-1], cuts[1:]):
            n = b - a
            d_o = api.DeviceBuffer.from_numpy(np.ascontiguousarray(offsets[a:b + 1], np.uint64))
            d_i, d_s, d_c = api.DeviceBuffer(n * n_sp * top * 4), api.DeviceBuffer(n * n_sp * top * 8), api.DeviceBuffer(n * n_sp * n_feat * 4)
            bufs += [d_o, d_i, d_s, d_c]
            rows.append((n, d_i, d_c))
            fn = S.enqueue_device if entry == "enqueue_device" else S.push_device
            fn(d_b.ptr, d_o.ptr, n, int(offsets[b] - offsets[a]), d_i.ptr, d_s.ptr, consensus=d_c.ptr if bind else None)
        S.sync()
        idx = np.concatenate([d_i.to_numpy(np.uint32, (n, n_sp, top)) for n, d_i, _ in rows])
        return idx, (np.concatenate([d_c.to_numpy(np.uint32, (n, n_sp, n_feat)) for n, _, d_c in rows]) if bind else None)
    finally:
        for d in bufs:
            d.free()


@pytest.fixture(scope="module")
def small(gpu):
    """600 genomes, s = 64, 2 800 reads of 200 to 400 bases, 16 genotype columns"""
    from sketchy_amd import api, synth
    ref = synth.make_reference(600, 64, rng_seed=901, device="numpy")
    bases, offsets = synth.make_reads(ref["genome"], 2800, 300, rng_seed=902, lognormal_sigma=0.4, min_len=200, max_len=400)
    codes = make_codes(600, 16, "three", np.random.default_rng(903))
    R = api.ReferenceSketch(ref["ref"], ref["col_len"])
    R.set_genotypes(codes)
    out = dict(R=R, ref=ref, bases=bases, offsets=offsets, codes=codes, cuts=[0, 700, 1400, 2100, 2800], plain={})
    yield out
    R.close()


def plain_rows(small, top):
    """the rows of the 2 800 reads from a stream that never binds (pushed in the same four batches), once per top"""
    from sketchy_amd import api
    if top not in small["plain"]:
        S = api.SumOfSharedHashes(small["R"], top=top, max_batch_reads=700, max_batch_bases=700 * 400)
        small["plain"][top] = drive(S, "push", small["bases"], small["offsets"], small["cuts"], top, 1, 16, bind=False)[0]
        S.close()
    return small["plain"][top]


@pytest.mark.parametrize("entry,null_rows", [("push", False), ("push_device", False), ("enqueue_device", False), ("submit", False),
                                             ("submit", True)], ids=("push", "push_device", "enqueue_device", "submit", "submit_null_rows"))
def test_every_entry_point_returns_the_codes_of_its_rows(small, entry, null_rows):
    from sketchy_amd import api
    rows = plain_rows(small, 5)
    S = api.SumOfSharedHashes(small["R"], top=5, max_batch_reads=700, max_batch_bases=700 * 400)
    idx, codes = drive(S, entry, small["bases"], small["offsets"], small["cuts"], 5, 1, 16, bind=True, null_rows=null_rows)
    if entry == "enqueue_device":
        assert S.stats()["passes_shared"] >= 1  # the four batches shared a pass: their chains ran on both lanes
    S.close()
    if not null_rows:
        np.testing.assert_array_equal(idx, rows, err_msg="a binding changed the rows")
    np.testing.assert_array_equal(codes, consensus_ref(rows, small["codes"], [600]))


@pytest.mark.parametrize("top", (1, 5, 17))
def test_ranking_paths(small, top):
    """top 1 (rank_seg_top1), 5 (the fast top-k) and 17 (the generic ranking) in front of the vote"""
    from sketchy_amd import api
    rows = plain_rows(small, top)
    S = api.SumOfSharedHashes(small["R"], top=top, max_batch_reads=700, max_batch_bases=700 * 400)
    idx, codes = drive(S, "enqueue_device", small["bases"], small["offsets"], small["cuts"], top, 1, 16, bind=True)
    S.close()
    np.testing.assert_array_equal(idx, rows)
    np.testing.assert_array_equal(codes, consensus_ref(rows, small["codes"], [600]))
    if top == 1:
        np.testing.assert_array_equal(codes[:, 0], small["codes"][rows[:, 0, 0]])


def test_a_batch_cut_into_several_passes(small):
    """stream_query_rows = s: a batch's distinct hashes exceed a pass's rows, so it is ranked pass by pass -- one vote per pass, each
    at its own first row"""
    from sketchy_amd import api
    rows = plain_rows(small, 5)[:700]
    try:
        api.set_option("stream_query_rows", 64)
        S = api.SumOfSharedHashes(small["R"], top=5, max_batch_reads=700, max_batch_bases=700 * 400)
    finally:
        api.set_option("stream_query_rows", 0)
    for entry in ("push", "push_device"):
        S.reset()
        idx, codes = drive(S, entry, small["bases"], small["offsets"], [0, 700], 5, 1, 16, bind=True)
        assert S.stats()["last_passes"] > 1, S.stats()
        np.testing.assert_array_equal(idx, rows)
        np.testing.assert_array_equal(codes, consensus_ref(rows, small["codes"], [600]))
    S.close()


def test_multi_species(gpu):
    from sketchy_amd import api
    sizes = (70, 129, 64)
    refs, bases, offsets = workload_species(sizes, 64, 900, read_len=300, rng_seed=931)
    codes = make_codes(sum(sizes), 16, "three", np.random.default_rng(932))
    R = api.ReferenceSketch([r["ref"] for r in refs])
    try:
        R.set_genotypes(codes)
        S0 = api.SumOfSharedHashes(R, top=3, max_batch_reads=300, max_batch_bases=300 * 300)
        rows = drive(S0, "push", bases, offsets, [0, 300, 600, 900], 3, 3, 16, bind=False)[0]
        want = consensus_ref(rows, codes, sizes)
        assert (want[:, 0] != want[:, 1]).any() and (want[:, 1] != want[:, 2]).any()
        for entry in ("push", "enqueue_device", "submit"):
            S = api.SumOfSharedHashes(R, top=3, max_batch_reads=300, max_batch_bases=300 * 300)
            idx, got = drive(S, entry, bases, offsets, [0, 300, 600, 900], 3, 3, 16, bind=True)
            np.testing.assert_array_equal(idx, rows)
            np.testing.assert_array_equal(got, want, err_msg=entry)
            if entry == "push":
                np.testing.assert_array_equal(S.consensus(), consensus_ref(S.rank()[0][None], codes, sizes)[0])
            S.close()
        S0.close()
    finally:
        R.close()


def test_compact_ranking(gpu):
    """A truth-strain stream long enough that batches are ranked on their candidates (rows through launch_cand_rows_back): the vote
    must read the rows AFTER they were mapped back to genome indices."""
    import tempfile
    from sketchy_amd import api
    from test_gpu_patterns import B, NB, _generate
    d = tempfile.mkdtemp(prefix="skx_cons_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    try:
        _generate(d)
        ref, bases, offsets = np.load(d + "/ref.npy"), np.load(d + "/bases.npy"), np.load(d + "/offsets.npy")
    finally:
        for f in os.listdir(d):
            os.remove(os.path.join(d, f))
        os.rmdir(d)
    codes = make_codes(len(ref), 16, "three", np.random.default_rng(941))
    R = api.ReferenceSketch(ref)
    try:
        R.set_genotypes(codes)
        cuts = [i * B for i in range(NB + 1)]
        cap = int(np.max(offsets[B::B] - offsets[:-B:B]))
        S0 = api.SumOfSharedHashes(R, top=3, max_batch_reads=B, max_batch_bases=cap)
        rows = drive(S0, "enqueue_device", bases, offsets, cuts, 3, 1, 16, bind=False)[0]
        S0.close()
        S = api.SumOfSharedHashes(R, top=3, max_batch_reads=B, max_batch_bases=cap)
        idx, got = drive(S, "enqueue_device", bases, offsets, cuts, 3, 1, 16, bind=True)
        st = S.stats()
        S.close()
        assert st["batches_compact"] > 0, st  # (stats()[16]: the case must keep covering that path)
        np.testing.assert_array_equal(idx, rows)
        np.testing.assert_array_equal(got, consensus_ref(rows, codes, [len(ref)]))
    finally:
        R.close()


def test_one_shot_binding(small):
    from sketchy_amd import _lib, api
    L = _lib.load()
    b, o = small["bases"], small["offsets"]
    S = api.SumOfSharedHashes(small["R"], top=5, max_batch_reads=700, max_batch_bases=700 * 400)
    first = S.push(b, o[:101], want_consensus=True)
    np.testing.assert_array_equal(first["consensus"], consensus_ref(first["topk_idx"][:, None], small["codes"], [600])[:, 0])
    # the next push is unbound: the old buffer, refilled with a sentinel, stays as it is
    first["consensus"][:] = 0xDEADBEEF
    S.push(b, o[100:201])
    assert (first["consensus"] == 0xDEADBEEF).all()
    # a bound call that fails has consumed the binding: push_device without its own row array
    sink = np.full((100, 16), 0xDEADBEEF, np.uint32)
    d_b, d_o = api.DeviceBuffer.from_numpy(b), api.DeviceBuffer.from_numpy(np.ascontiguousarray(o[200:301]))
    d_c = api.DeviceBuffer.from_numpy(sink)
    try:
        S.bind_consensus(d_c.ptr)
        rc = L.skx_stream_push_device(S._h, d_b.ptr, d_o.ptr, 100, int(o[300] - o[200]), None, None)
        assert rc == _lib.ERR_INVALID and "d_topk_idx" in L.skx_last_error().decode()
        reads = S.reads
        S.push_device(d_b.ptr, d_o.ptr, 100, int(o[300] - o[200]), None, None)  # unbound now: as ever, and no codes anywhere
        S.sync()
        assert S.reads == reads + 100
        assert (d_c.to_numpy(np.uint32, (100, 16)) == 0xDEADBEEF).all()
    finally:
        for d in (d_b, d_o, d_c):
            d.free()
    S.close()
    # a stream without a ranking: binding succeeds, the batch call fails
    S = api.SumOfSharedHashes(small["R"], top=0, max_batch_reads=700, max_batch_bases=700 * 400)
    S.bind_consensus(_p(sink))
    with pytest.raises(_lib.SketchyHipError) as e:
        S.push(b, o[:101])
    assert e.value.code == _lib.ERR_INVALID and "top_k" in str(e.value)
    assert S.reads == 0
    S.push(b, o[:101])  # (the binding went with the failed call)
    assert S.reads == 100 and (sink == 0xDEADBEEF).all()
    S.close()
    # a reference without a table: the same
    R = api.ReferenceSketch(small["ref"]["ref"], small["ref"]["col_len"])
    S = api.SumOfSharedHashes(R, top=5, max_batch_reads=700, max_batch_bases=700 * 400)
    S.bind_consensus(_p(sink))
    with pytest.raises(_lib.SketchyHipError) as e:
        S.push(b, o[:101])
    assert e.value.code == _lib.ERR_INVALID and "genotype table" in str(e.value)
    got = S.push(b, o[:101])
    np.testing.assert_array_equal(got["topk_idx"], first["topk_idx"])
    assert (sink == 0xDEADBEEF).all()
    S.close()
    R.close()


def test_against_the_oracle_at_c0(gpu):
    """BASELINE configs[0] (tests/test_gpu_parity.py): the restatement applied to the ORACLE's rows is what the device returns"""
    from oracle import oracle as orc
    from sketchy_amd import api
    ref, bases, offsets = workload(500, 1000, 1000)
    exp = orc.stream(16, 0, 1000, ref["ref"], ref["col_len"], bases, offsets, top_k=5)
    codes = make_codes(500, 16, "three", np.random.default_rng(951))
    R = api.ReferenceSketch(ref["ref"], ref["col_len"])
    R.set_genotypes(codes)
    S = api.SumOfSharedHashes(R, top=5, max_batch_reads=1000, max_batch_bases=len(bases))
    got = S.push(bases, offsets, want_consensus=True)
    np.testing.assert_array_equal(got["topk_idx"], exp["topk_idx"])
    np.testing.assert_array_equal(got["consensus"], consensus_ref(exp["topk_idx"][:, None], codes, [500])[:, 0])
    np.testing.assert_array_equal(S.consensus(), got["consensus"][-1])
    S.close()
    R.close()


# ---------------------------------------------------------------- the CLI with the real library
def _cli(*args):
    p = subprocess.run([BIN, *args], capture_output=True)
    return p.returncode, p.stdout.decode(), p.stderr.decode()


@pytest.fixture(scope="module")
def cli_inputs(tmp_path_factory):
    d = tmp_path_factory.mktemp("consensus_cli")
    ref, bases, offsets = workload(64, 200, 360, read_len=400, genome_len=40000, rng_seed=961)
    names = [f"genome{i:02d}.fa" for i in range(64)]
    msh = str(d / "ref.msh")
    write_msh(msh, names, ref["ref"], kmer=16, seed=0, lengths=[40000] * 64)
    tsvs = {}
    # "plain": few values per column; "ties": every genome its own value in one column (all five tie: the smallest string wins),
    # strings whose byte order is not their numeric order, and a column of two values that is mostly 2 : 2 : 1 with a third
    cols = dict(plain=lambda i: [f"ST{i % 3}", "+-"[i % 2], f"t{i % 2}"],
                ties=lambda i: [f"ST{(i * 37) % 64}", f"v{i % 5}", "Aa"[i % 2] + str(i % 3)])
    for key, fn in cols.items():
        tsvs[key] = str(d / f"{key}.tsv")
        with open(tsvs[key], "w") as f:
            f.write("id\tmlst\tmec\ttype\n" + "".join(nm + "\t" + "\t".join(fn(i)) + "\n" for i, nm in enumerate(names)))
    reads = unpack_reads(bases, offsets)
    files = []
    for j, part in enumerate((reads[:300], reads[300:])):
        files.append(str(d / f"sample{j}.fq"))
        with open(files[-1], "w") as f:
            f.write("".join(f"@r{i}\n{r.decode()}\n+\n{'I' * len(r)}\n" for i, r in enumerate(part)))
    return msh, tsvs, files


@pytest.mark.parametrize("table", ("plain", "ties"))
def test_cli_consensus_is_the_vote_over_the_rows_it_prints_without_c(gpu, cli_inputs, table):
    msh, tsvs, files = cli_inputs
    nm = subprocess.check_output(["nm", "-D", BIN], text=True)
    assert "skx_stream_bind_consensus" in nm and "skx_consensus_rows" in nm
    for args in (("-s", "-H", "-b", "64", "-i", files[0]), ("-i", *files)):
        rc, rows, err = _cli("predict", "-r", msh, "-g", tsvs[table], "-t", "5", *args)
        assert rc == 0 and rows, err
        rc, cons, err = _cli("predict", "-r", msh, "-g", tsvs[table], "-t", "5", "-c", *args)
        assert rc == 0, err
        header = "reads\tsketch_id\tshared_hashes\tmlst\tmec\ttype\n" if "-H" in args else ""
        assert rows.startswith(header) and cons.startswith(header)
        want = consensus_of_rows(rows[len(header):], 5)
        assert cons[len(header):] == want, args
        assert want.count("\n") == (300 if "-s" in args else 2)
        if table == "ties" and "-s" in args:
            # how many reads' first column is a five-way tie (every genome has its own value there)
            lines = [ln.split("\t") for ln in rows[len(header):].splitlines()]
            tied = sum(len({g[3] for g in lines[i:i + 5]}) == 5 for i in range(0, len(lines), 5))
            assert tied == 300, tied
