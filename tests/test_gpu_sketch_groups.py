"""skx_sketch_groups on the device: ONE bottom-s sketch per group of records, pooled by the merge tree.

Expected values come from the oracle alone: the heap sketcher over the group's records joined with `N` (an N breaks every
window, so no k-mer spans two records) for rows and lengths, the sum of the records' k-mer counts for valid_kmers.  Compared
hash by hash; padding beyond sketch_len must be zero."""
import functools
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import exp_env, pack_reads, unpack_reads, workload
from mshio import read_msh, write_msh
from oracle import oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "sketchy_amd", "sketchy-hip")
ACGT = np.frombuffer(b"ACGT", np.uint8)
GROUP_SIZES = (0, 1, 2, 3, 4, 5, 33, 64, 65, 130)
PARAMS = ((16, 0, 64), (16, 0, 1000), (21, 5, 1000), (32, 7, 1), (1, 0, 3))


def _dna(rng, n):
    return ACGT[rng.integers(0, 4, int(n))].tobytes()


def _first(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32)


def _expected(records, first, k, seed, s):
    ng = len(first) - 1
    rows, lens, valid = np.zeros((ng, s), np.uint64), np.zeros(ng, np.uint32), np.zeros(ng, np.uint64)
    for g in range(ng):
        recs = records[int(first[g]):int(first[g + 1])]
        if not recs:
            continue
        h = orc.sketch(b"N".join(recs), k, seed, s)
        rows[g, :len(h)], lens[g] = h, len(h)
        valid[g] = sum(len(orc.kmer_hashes(r, k, seed)[0]) for r in recs)
    return rows, lens, valid


def _check(got, exp, what=""):
    np.testing.assert_array_equal(got[1], exp[1], err_msg=f"{what} sketch_len")
    np.testing.assert_array_equal(got[0], exp[0], err_msg=f"{what} rows")  # (zero padding included)
    if len(got) > 2:
        np.testing.assert_array_equal(got[2], exp[2], err_msg=f"{what} valid_kmers")


def _run(records, first, k, seed, s, **kw):
    from sketchy_amd import api
    bases, offsets = pack_reads(records)
    return api.sketch_groups(bases, offsets, first, k=k, seed=seed, s=s, want_valid_kmers=True, **kw)


@functools.lru_cache(maxsize=None)
def _group_sizes_input():
    rng = np.random.default_rng(2024)
    n = sum(GROUP_SIZES)
    lens = rng.integers(0, 4001, n)
    lens[[0, 5, 40, 200]] = (0, 3, 15, 31)  # empty, and shorter than k = 16 / 21 / 32
    return [_dna(rng, m) for m in lens], _first(GROUP_SIZES)


@functools.lru_cache(maxsize=None)
def _group_sizes_expected(k, seed, s):
    records, first = _group_sizes_input()
    return _expected(records, first, k, seed, s)


@functools.lru_cache(maxsize=None)
def _long_input():
    rng = np.random.default_rng(7)
    records = [_dna(rng, 60000), _dna(rng, 25000), _dna(rng, 9000)]
    starts = rng.integers(0, 60000 - 1500, 20)
    records += [records[0][int(a):int(a) + 1500] for a in starts]
    order = rng.permutation(len(records))  # long and short records interleaved
    return [records[i] for i in order], _first([len(records)])


@functools.lru_cache(maxsize=None)
def _long_expected():
    records, first = _long_input()
    return _expected(records, first, 16, 0, 10000)


@pytest.mark.gpu
@pytest.mark.parametrize("k, seed, s", PARAMS)
def test_group_sizes(gpu, k, seed, s):
    """Groups of 0, 1, 2, 3, 4, 5, 33, 64, 65 and 130 records in one call: empty groups, odd carries, more rows than a wave
    or a workgroup has lanes; records of 0 .. 4000 bases, some shorter than k."""
    records, first = _group_sizes_input()
    _check(_run(records, first, k, seed, s), _group_sizes_expected(k, seed, s))


@pytest.mark.gpu
def test_duplicates_and_sizes_of_the_union(gpu):
    rng = np.random.default_rng(99)
    one = _dna(rng, 3000)
    text = _dna(rng, 6000)
    shared = [text[i * 500:i * 500 + 1000] for i in range(11)]  # neighbours share half their text
    dirty = _dna(rng, 1000) + b"NNNNNRYK" + _dna(rng, 2000).lower()
    records = [one] * 8 + shared + [dirty, _dna(rng, 700)]
    first = _first([8, len(shared), 2])
    exp = _expected(records, first, 16, 0, 1000)
    got = _run(records, first, 16, 0, 1000)
    _check(got, exp)
    own = orc.sketch(one, 16, 0, 1000)
    np.testing.assert_array_equal(got[0][0, :len(own)], own)  # 8 copies pool to the record's own sketch
    assert got[1][0] == len(own)
    # s larger than the union, exactly the union's size, one less, and 1
    union = len(np.unique(np.concatenate([orc.kmer_hashes(r, 16, 0)[0] for r in shared])))
    for s in (union + 17, union, union - 1, 1):
        got = _run(shared, _first([len(shared)]), 16, 0, s)
        _check(got, _expected(shared, _first([len(shared)]), 16, 0, s), what=f"s={s}")
        assert got[1][0] == min(s, union)


@pytest.mark.gpu
def test_long_records_feed_the_same_group(gpu):
    """Records of 60 000, 25 000 and 9 000 bases (block sketcher, rows of full length s) and 20 reads of 1 500 bases cut from
    the first one (wave sketcher) in ONE group at s = 10 000: duplicates across the two paths."""
    records, first = _long_input()
    exp = _long_expected()
    assert exp[1][0] == 10000
    _check(_run(records, first, 16, 0, 10000), exp)


@pytest.mark.gpu
def test_many_small_groups(gpu):
    rng = np.random.default_rng(5)
    sizes = rng.integers(1, 6, 3000)
    first = _first(sizes)
    assert np.count_nonzero(first[1:-1] % 64 == 0) >= 5  # several boundaries on multiples of 64 records
    records = [_dna(rng, m) for m in rng.integers(200, 1501, int(first[-1]))]
    _check(_run(records, first, 16, 0, 1000), _expected(records, first, 16, 0, 1000))


@pytest.mark.gpu
def test_one_large_group(gpu):
    """The offline shape: 8 192 reads of 1 500 bases in one group at s = 10 000 -- 13 rounds, union far larger than s."""
    rng = np.random.default_rng(6)
    records = [_dna(rng, 1500) for _ in range(8192)]
    first = _first([8192])
    exp = _expected(records, first, 16, 0, 10000)
    assert exp[1][0] == 10000
    _check(_run(records, first, 16, 0, 10000), exp)


@pytest.mark.gpu
def test_sliced_run_matches(gpu, tmp_path):
    """The group-size and long-record cases again in a child process that loads the experiments build with the row budget
    forced to 7 rows: dozens of slices, groups open across slice boundaries -- same rows as the oracle (and so as the
    unsliced runs above)."""
    cases = [(_group_sizes_input(), p, _group_sizes_expected(*p)) for p in PARAMS] + [(_long_input(), (16, 0, 10000), _long_expected())]
    arrays = dict(n_cases=len(cases))
    for i, ((records, first), p, _) in enumerate(cases):
        arrays[f"bases{i}"], arrays[f"offsets{i}"] = pack_reads(records)
        arrays[f"first{i}"], arrays[f"params{i}"] = first, np.array(p, np.int64)
    src, dst = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    np.savez(src, **arrays)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "sketch_groups_worker.py"), src, dst], env=exp_env(SKX_POOL_ROWS=7),
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    z = np.load(dst)
    for i, (_, p, exp) in enumerate(cases):
        _check((z[f"sk{i}"], z[f"sl{i}"], z[f"vk{i}"]), exp, what=f"sliced {p}")


@pytest.mark.gpu
def test_offsets_need_not_start_at_zero_and_calls_are_independent(gpu):
    from sketchy_amd import api
    rng = np.random.default_rng(12)
    records = [_dna(rng, m) for m in (900, 40, 1700, 0, 650)]
    first = _first([2, 0, 3])
    bases, offsets = pack_reads(records)
    shifted = np.concatenate([np.frombuffer(b"G" * 37, np.uint8), bases])
    exp = _expected(records, first, 16, 0, 500)
    _check(api.sketch_groups(shifted, offsets + np.uint64(37), first, k=16, seed=0, s=500, want_valid_kmers=True), exp)
    other = [_dna(rng, 2500)]
    _check(_run(other, _first([1]), 21, 3, 100), _expected(other, _first([1]), 21, 3, 100))
    _check(api.sketch_groups(shifted, offsets + np.uint64(37), first, k=16, seed=0, s=500, want_valid_kmers=True), exp, what="second call")
    sk, sl = api.sketch_groups(bases, offsets, first, k=16, seed=0, s=500)  # without valid_kmers
    _check((sk, sl), exp[:2])


def _cli(*args, stdin=None):
    p = subprocess.run([BIN, *args], input=stdin, capture_output=True)
    return p.returncode, p.stdout.decode(), p.stderr.decode()


@pytest.mark.gpu
def test_cli_sketch_pools_files_on_the_device(gpu, tmp_path):
    rng = np.random.default_rng(11)
    files, contigs_of = [], []
    for gi, sizes in enumerate(([60000, 3000, 10], [25000] * 4, [900], [2000] * 70)):
        contigs = [_dna(rng, n) for n in sizes]
        if gi == 0:
            contigs[1] = contigs[1][:1000] + b"NNNNNRYK" + contigs[1][1000:].lower()
        path = str(tmp_path / f"genome{gi}.fa") + (".gz" if gi == 1 else "")
        with (gzip.open if gi == 1 else open)(path, "wt") as f:
            for ci, c in enumerate(contigs):
                t = c.decode()
                f.write(f">contig{ci} some description\n" + "\n".join(t[j:j + 60] for j in range(0, len(t), 60)) + "\n")
        files.append(path); contigs_of.append(contigs)
    out = str(tmp_path / "db.msh")
    for s, k, seed in ((1000, 16, 0), (64, 21, 5)):
        rc, so, err = _cli("sketch", "-i", *files, "-o", out, "-s", str(s), "-k", str(k), "-e", str(seed))
        assert rc == 0, err
        kk, sd, recs = read_msh(out)
        assert (kk, sd) == (k, seed)
        assert [r["name"] for r in recs] == [os.path.basename(p) for p in files]
        for r, contigs in zip(recs, contigs_of):
            rows, lens, valid = _expected(contigs, _first([len(contigs)]), k, seed, s)
            np.testing.assert_array_equal(r["hashes"], rows[0, :lens[0]])
            assert r["length"] == sum(len(c) for c in contigs)
            assert r["num_valid_kmers"] == int(valid[0])
    und = subprocess.check_output(["nm", "-D", "--undefined-only", BIN], text=True)
    assert "skx_sketch_groups" in und  # the product binary is linked to the pooled entry point


@pytest.mark.gpu
def test_cli_offline_predict_pools_batches_on_the_device(gpu, tmp_path):
    """Offline `predict -b 4096` on 5 000 reads (two batches, one pooled row each, merged on the host) against 64 genomes at
    s = 1000."""
    ref, bases, offsets = workload(64, 1000, 5000, read_len=400, genome_len=40000, rng_seed=77)
    names = [f"genome{i:02d}.fa" for i in range(64)]
    msh, tsv, fq = str(tmp_path / "ref.msh"), str(tmp_path / "geno.tsv"), str(tmp_path / "reads.fq")
    write_msh(msh, names, ref["ref"], kmer=16, seed=0, lengths=[40000] * 64)
    with open(tsv, "w") as f:
        f.write("id\tmlst\n" + "".join(f"{nm}\tST{i % 7}\n" for i, nm in enumerate(names)))
    reads = unpack_reads(bases, offsets)
    with open(fq, "w") as f:
        f.write("".join(f"@r{i}\n{r.decode()}\n+\n{'I' * len(r)}\n" for i, r in enumerate(reads)))
    for limit in (0, 4500):
        use = reads if not limit else reads[:limit]
        pooled = orc.sketch(b"N".join(use), 16, 0, 1000)
        common = np.array([orc.common_hashes(ref["ref"][g], pooled) for g in range(64)])
        assert common.max() > 0
        order = orc.stable_rank(common.astype(np.uint64))[:5]
        want = "".join(f"{len(use)}\t{names[g]}\t{common[g]}\tST{g % 7}\n" for g in order)
        rc, so, err = _cli("predict", "-r", msh, "-g", tsv, "-i", fq, "-t", "5", "-b", "4096", *(["-l", str(limit)] if limit else []))
        assert rc == 0, err
        assert so == want
