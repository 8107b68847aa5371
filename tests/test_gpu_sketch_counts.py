"""skx_sketch_groups_counts on the device: the pooled bottom-s sketch of every group of records AND the abundance of each of its
hashes (finch's KmerCount.count, Mash's counts32).

Expected values come from the oracle alone: rows, lengths and valid_kmers as in tests/test_gpu_sketch_groups.py (the heap sketcher
over the group's records joined with `N`); counts[g][j] = occurrences of rows[g][j] among the canonical hashes of all valid k-mer
windows of the group's records (orc.kmer_hashes per record, np.unique over the group).  Every test also holds the counted call
against the plain one (rows, lengths, valid_kmers identical), wants zero counts in the padding, and checks the sum rule: the counts
of a group add up to its valid k-mers when its sketch is the whole union (sketch_len < s), and to no more elsewhere."""
import functools
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import exp_env, pack_reads
from oracle import oracle as orc
from test_gpu_sketch_groups import (GROUP_SIZES, PARAMS, _dna, _expected, _first, _group_sizes_expected, _group_sizes_input, _long_expected,
                                    _long_input)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "sketchy_amd", "sketchy-hip")
COMP = bytes.maketrans(b"ACGT", b"TGCA")


def _expected_counts(records, first, k, seed, rows, lens):
    """counts [groups][s] for the oracle's rows: np.unique over all k-mer hashes of the group's records, looked up at the row."""
    counts = np.zeros(rows.shape, np.uint32)
    for g in range(len(first) - 1):
        n = int(lens[g])
        if not n:
            continue
        hs = np.concatenate([orc.kmer_hashes(r, k, seed)[0] for r in records[int(first[g]):int(first[g + 1])]])
        u, c = np.unique(hs, return_counts=True)
        at = np.searchsorted(u, rows[g, :n])
        np.testing.assert_array_equal(u[at], rows[g, :n])  # (every sketch hash is a hash of the group)
        counts[g, :n] = np.minimum(c[at], 0xFFFFFFFF)
    return counts


def _check(got, plain, exp, exp_counts, s, what=""):
    """got = (rows, lengths, valid_kmers, counts) of the counted call; plain = the plain call's triple; exp = the oracle's triple"""
    sk, sl, vk, kc = got
    assert kc.dtype == np.uint32 and kc.shape == sk.shape == (len(sl), s)
    for a, b, name in zip(got[:3], plain, ("rows", "sketch_len", "valid_kmers")):
        np.testing.assert_array_equal(a, b, err_msg=f"{what} {name}: counted call against the plain call")
    np.testing.assert_array_equal(sl, exp[1], err_msg=f"{what} sketch_len")
    np.testing.assert_array_equal(sk, exp[0], err_msg=f"{what} rows")
    np.testing.assert_array_equal(vk, exp[2], err_msg=f"{what} valid_kmers")
    pad = np.arange(s)[None, :] >= sl[:, None]
    assert not kc[pad].any(), f"{what} counts in the padding"
    assert (kc[~pad] >= 1).all(), f"{what} a sketch hash with count 0"
    sums = kc.astype(np.uint64).sum(axis=1)
    whole = sl < s
    np.testing.assert_array_equal(sums[whole], vk[whole], err_msg=f"{what} the whole union: counts must add up to valid_kmers")
    assert (sums <= vk).all(), f"{what} more counts than valid k-mers"
    np.testing.assert_array_equal(kc, exp_counts, err_msg=f"{what} counts")


def _both(records, first, k, seed, s, shift=0):
    from sketchy_amd import api
    bases, offsets = pack_reads(records)
    if shift:
        bases, offsets = np.concatenate([np.frombuffer(b"G" * shift, np.uint8), bases]), offsets + np.uint64(shift)
    plain = api.sketch_groups(bases, offsets, first, k=k, seed=seed, s=s, want_valid_kmers=True)
    got = api.sketch_groups(bases, offsets, first, k=k, seed=seed, s=s, want_valid_kmers=True, want_counts=True)
    assert len(plain) == 3 and len(got) == 4
    return got, plain


def _case(records, first, k, seed, s, exp=None, what="", shift=0):
    exp = exp or _expected(records, first, k, seed, s)
    got, plain = _both(records, first, k, seed, s, shift=shift)
    _check(got, plain, exp, _expected_counts(records, first, k, seed, exp[0], exp[1]), s, what=what)
    return got


@functools.lru_cache(maxsize=None)
def _group_sizes_counts(k, seed, s):
    records, first = _group_sizes_input()
    exp = _group_sizes_expected(k, seed, s)
    return _expected_counts(records, first, k, seed, exp[0], exp[1])


@functools.lru_cache(maxsize=None)
def _long_counts():
    records, first = _long_input()
    exp = _long_expected()
    return _expected_counts(records, first, 16, 0, exp[0], exp[1])


@pytest.mark.gpu
@pytest.mark.parametrize("k, seed, s", PARAMS)
def test_group_sizes(gpu, k, seed, s):
    """Groups of 0 .. 130 records, records of 0 .. 4000 bases (some shorter than k).  k = 1 has two hashes with counts in the
    hundreds of thousands: every lane's increment goes to one of two addresses."""
    records, first = _group_sizes_input()
    assert len(first) - 1 == len(GROUP_SIZES)
    got, plain = _both(records, first, k, seed, s)
    kc = _group_sizes_counts(k, seed, s)
    if k == 1:
        assert kc.max() > 100000
    _check(got, plain, _group_sizes_expected(k, seed, s), kc, s)


@pytest.mark.gpu
def test_duplicates(gpu):
    rng = np.random.default_rng(99)
    one = _dna(rng, 3000)
    # one record eight times: the record's own sketch, every count x 8
    alone = _case([one], _first([1]), 16, 0, 1000, what="alone")
    eight = _case([one] * 8, _first([8]), 16, 0, 1000, what="x 8")
    np.testing.assert_array_equal(eight[0], alone[0])
    np.testing.assert_array_equal(eight[3], alone[3] * np.uint32(8))
    # a record and its reverse complement: the same canonical k-mers once more
    both = _case([one, one.translate(COMP)[::-1]], _first([2]), 16, 0, 1000, what="+ reverse complement")
    np.testing.assert_array_equal(both[0], alone[0])
    np.testing.assert_array_equal(both[3], alone[3] * np.uint32(2))
    # overlapping cuts of one text: neighbours share half their windows
    text = _dna(rng, 6000)
    shared = [text[i * 500:i * 500 + 1000] for i in range(11)]
    got = _case(shared, _first([len(shared)]), 16, 0, 20000, what="overlapping cuts")
    assert got[3].max() >= 2 and got[1][0] < 20000


@pytest.mark.gpu
def test_dirty_input(gpu):
    """Lower case, U, N, IUPAC codes and removed whitespace inside records: a window across a line break still counts, a window
    across an N does not."""
    rng = np.random.default_rng(3)
    a, b, c = _dna(rng, 1500), _dna(rng, 2200), _dna(rng, 900)
    wrapped = b"\n".join(b[i:i + 60] for i in range(0, len(b), 60)) + b"\n"
    records = [
        a[:700] + b"NNNNNRYK" + a[700:].lower(),
        wrapped,
        b,                                                   # the same text unwrapped: every count of it twice
        c.replace(b"T", b"U")[:450] + b" \t" + c[450:460] + b"\r\n" + c[460:].lower().replace(b"t", b"u"),
        b"acgtnACGTRYKMSWBDHVacgt" * 30 + b" " + a[:25],
        b"\n \n", b"", b"ACGT\nACGT\nACGT\nACG",
    ]
    first = _first([3, 2, 3])
    for k, seed, s in ((16, 0, 5000), (21, 5, 300), (4, 0, 40)):
        _case(records, first, k, seed, s, what=f"k={k}")
    # a line break between every two bases changes nothing
    spaced = b"\n".join(bytes([x]) for x in c)
    got = _case([c, spaced], _first([1, 1]), 16, 0, 1000, what="one base per line")
    np.testing.assert_array_equal(got[0][0], got[0][1])
    np.testing.assert_array_equal(got[3][0], got[3][1])


@pytest.mark.gpu
def test_counts_past_16_bits(gpu):
    """70 000 x A and 70 000 x T in one group at k = 16: ONE canonical hash, 2 x (70 000 - 15) = 139 970 occurrences -- a 32-bit
    count, the block sketcher's long-record path, and every increment of the kernel on a single counter."""
    records = [b"A" * 70000, b"T" * 70000]
    got = _case(records, _first([2]), 16, 0, 1000)
    assert got[1][0] == 1 and int(got[3][0, 0]) == 139970 and int(got[2][0]) == 139970


@pytest.mark.gpu
def test_long_and_short_records_in_one_group(gpu):
    """60 000 / 25 000 / 9 000 bases (block sketcher) + 20 reads of 1 500 bases cut from the first (wave sketcher) at s = 10 000."""
    records, first = _long_input()
    got, plain = _both(records, first, 16, 0, 10000)
    kc = _long_counts()
    assert kc.max() >= 2
    _check(got, plain, _long_expected(), kc, 10000)


@pytest.mark.gpu
def test_threshold_edges(gpu):
    """s above the union, the union, one less and 1: the row shorter than s against the full row -- the compare with the row's last
    value and the last position."""
    rng = np.random.default_rng(99)
    text = _dna(rng, 6000)
    shared = [text[i * 500:i * 500 + 1000] for i in range(11)]
    first = _first([len(shared)])
    union = len(np.unique(np.concatenate([orc.kmer_hashes(r, 16, 0)[0] for r in shared])))
    for s in (union + 17, union, union - 1, 1):
        got = _case(shared, first, 16, 0, s, what=f"s={s}")
        assert got[1][0] == min(s, union)


@pytest.mark.gpu
def test_sliced_run_matches(gpu, tmp_path):
    """The group-size and long-record cases again in a child process on the experiments build with the row budget forced to 7
    rows: groups open across dozens of slice boundaries, the carry merge adds counts and a carried row is cut again later."""
    cases = [(_group_sizes_input(), p, _group_sizes_expected(*p), _group_sizes_counts(*p)) for p in PARAMS]
    cases.append((_long_input(), (16, 0, 10000), _long_expected(), _long_counts()))
    arrays = dict(n_cases=len(cases))
    for i, ((records, first), p, _, _) in enumerate(cases):
        arrays[f"bases{i}"], arrays[f"offsets{i}"] = pack_reads(records)
        arrays[f"first{i}"], arrays[f"params{i}"] = first, np.array(p, np.int64)
    src, dst = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    np.savez(src, **arrays)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "sketch_counts_worker.py"), src, dst], env=exp_env(SKX_POOL_ROWS=7),
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    z = np.load(dst)
    for i, (_, p, exp, kc) in enumerate(cases):
        _check((z[f"sk{i}"], z[f"sl{i}"], z[f"vk{i}"], z[f"kc{i}"]), (z[f"psk{i}"], z[f"psl{i}"], z[f"pvk{i}"]), exp, kc, p[2], what=f"sliced {p}")


@pytest.mark.gpu
def test_offsets_need_not_start_at_zero_and_calls_are_independent(gpu):
    rng = np.random.default_rng(12)
    records = [_dna(rng, m) for m in (900, 40, 1700, 0, 650)]
    records[2] = records[2][:800] + records[0][100:600] + records[2][800:]  # (counts of 2 inside group 0 ... and across groups none)
    first = _first([2, 0, 3])
    one = _case(records, first, 16, 0, 500, what="shifted", shift=37)
    other = [_dna(rng, 2500)]
    _case(other, _first([1]), 21, 3, 100, what="other")
    again = _case(records, first, 16, 0, 500, what="second call", shift=37)
    for a, b in zip(one, again):
        np.testing.assert_array_equal(a, b)
    from sketchy_amd import api
    bases, offsets = pack_reads(records)
    sk, sl, kc = api.sketch_groups(bases, offsets, first, k=16, seed=0, s=500, want_counts=True)  # without valid_kmers: counts stay last
    np.testing.assert_array_equal(kc, one[3])
    np.testing.assert_array_equal(sk, one[0])


def _cli(*args):
    p = subprocess.run([BIN, *args], capture_output=True)
    return p.returncode, p.stdout.decode(), p.stderr.decode()


@pytest.mark.gpu
def test_cli_sketch_counts(gpu, tmp_path):
    """`sketchy-hip sketch --counts` on three small FASTA files (one gzip, one multi-contig with 60-column lines), read back with
    sketchy_amd.mshio.read_msh; without --counts the file has no counts list."""
    from sketchy_amd.mshio import read_msh
    rng = np.random.default_rng(21)
    files, contigs_of = [], []
    for gi, sizes in enumerate(([9000, 3000, 10, 700], [5000] * 2, [900])):
        contigs = [_dna(rng, n) for n in sizes]
        if gi == 0:
            contigs[1] = contigs[1][:1000] + b"NNNNNRYK" + contigs[0][200:1200].lower()  # (repeats contig 0: counts of 2)
        if gi == 1:
            contigs[1] = contigs[0]
        path = str(tmp_path / f"genome{gi}.fa") + (".gz" if gi == 1 else "")
        with (gzip.open if gi == 1 else open)(path, "wt") as f:
            for ci, c in enumerate(contigs):
                t = c.decode()
                f.write(f">contig{ci} some description\n" + "\n".join(t[j:j + 60] for j in range(0, len(t), 60)) + "\n")
        files.append(path); contigs_of.append(contigs)
    out = str(tmp_path / "db.msh")
    for s, k, seed in ((1000, 16, 0), (64, 21, 5)):
        rc, so, err = _cli("sketch", "-i", *files, "-o", out, "-s", str(s), "-k", str(k), "-e", str(seed), "--counts")
        assert rc == 0, err
        kk, sd, recs = read_msh(out)
        assert (kk, sd) == (k, seed)
        assert [r["name"] for r in recs] == [os.path.basename(p) for p in files]
        for r, contigs in zip(recs, contigs_of):
            first = _first([len(contigs)])
            rows, lens, valid = _expected(contigs, first, k, seed, s)
            np.testing.assert_array_equal(r["hashes"], rows[0, :lens[0]])
            np.testing.assert_array_equal(r["counts"], _expected_counts(contigs, first, k, seed, rows, lens)[0, :lens[0]])
            assert r["counts"].dtype == np.uint32
            assert r["length"] == sum(len(c) for c in contigs)
            assert r["num_valid_kmers"] == int(valid[0])
        assert (recs[1]["counts"] == 2).all()  # (its second contig repeats the first)
        plain = str(tmp_path / "plain.msh")
        rc, so, err = _cli("sketch", "-i", *files, "-o", plain, "-s", str(s), "-k", str(k), "-e", str(seed))
        assert rc == 0, err
        _, _, precs = read_msh(plain)
        for r, p in zip(recs, precs):
            assert len(p["counts"]) == 0
            np.testing.assert_array_equal(p["hashes"], r["hashes"])
    und = subprocess.check_output(["nm", "-D", "--undefined-only", BIN], text=True)
    assert "skx_sketch_groups_counts" in und  # bound through a weak reference to the counted entry point
