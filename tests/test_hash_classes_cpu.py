"""The designed references of tests/hash_classes.py, checked without a device: the builder's invariants (ascending columns, every
storage class present with its intended count, the signature condition that makes the number of pattern lists exact by construction)
and the agreement of the two expectations the GPU tests use -- orc.common_hashes per genome, and the counts read off the design."""
import collections
import functools

import numpy as np
import pytest

import hash_classes as hc
from oracle import oracle as orc

R, N = hc.R_TEST, hc.N_SINGLE
design = functools.lru_cache(maxsize=None)(hc.single_species)


def _ascending(refs, col_lens):
    for ref, col_len in zip(refs, col_lens):
        for g in range(len(ref)):
            col = ref[g, :col_len[g]]
            assert (col[1:] > col[:-1]).all()
            assert not ref[g, col_len[g]:].any()


def test_mix32_is_the_kernels():
    """three values worked out by hand from list_sig_kernel's mix32 (32-bit wrap-around), and no collision among the genomes"""
    def scalar(x):
        x = ((x ^ (x >> 16)) * 0x7FEB352D) & 0xFFFFFFFF
        x = ((x ^ (x >> 15)) * 0x846CA68B) & 0xFFFFFFFF
        return x ^ (x >> 16)
    assert [int(v) for v in hc.mix32([0, 1, 1299, 0xFFFFFFFF])] == [scalar(0), scalar(1), scalar(1299), scalar(0xFFFFFFFF)]
    assert scalar(0) == 0 and scalar(1) != 1
    assert len(set(hc.mix32(np.arange(N)).tolist())) == N


@pytest.mark.parametrize("n_dense", (64, 65, 900))
def test_single_species_classes(n_dense):
    d = design(n_dense)
    refs, col_lens = hc.build_reference(d)
    _ascending(refs, col_lens)
    stride = refs[0].shape[1]
    assert refs[0].shape[0] == N and 100 <= stride <= 300
    genome, hashes = hc.genome_hashes()
    assert sorted(d.members) == [int(h) for h in hashes] and int(hashes[-1]) < hc.FE      # every hash of the genome, none lifted
    assert col_lens[0].min() > 0
    n = {cls: len(hs) for cls, hs in d.classes.items()}
    held = {cls: {len(d.members[h]) for h in hs} for cls, hs in d.classes.items()}
    for m in (1, 2, 7, 8, 9, 10, 63, 64, 65, R - 1, R):
        assert n[f"list{m}"] == 12 and held[f"list{m}"] == {m}
    for m in (200, N - 1, N):
        assert n[f"dense{m}"] == 16 and held[f"dense{m}"] == {m}
    assert n[f"dense{R + 1}"] == 16 + n_dense - 64 and held[f"dense{R + 1}"] == {R + 1}
    assert held["rest"] <= {1, 2, 3, 4, 5} and n["rest"] > 4000
    assert sum(len(m) > R for m in d.members.values()) == n_dense
    if n_dense == 900:
        assert n_dense > 191 * stride // 64               # more than build_static_dense takes for a species
    else:
        assert n_dense <= 191 * stride // 64
    # the lineages: 40 consecutive genomes across genome 256, across genome 512 and inside a tile
    assert [(int(L[0]) // hc.TILE, int(L[-1]) // hc.TILE) for L, _ in d.lineages] == [(0, 1), (1, 2), (2, 2)]
    assert [(int(L[0]) // hc.GROUP, int(L[-1]) // hc.GROUP) for L, _ in d.lineages] == [(0, 0), (0, 1), (1, 1)]
    for li, (L, lists) in enumerate(d.lineages):
        assert len(L) == 40 and n[f"lineage{li}_exact"] == 12
        for h, e, form in lists:
            got = d.members[h]
            gone, new = np.setdiff1d(L, got), np.setdiff1d(got, L)
            assert len(gone) + len(new) == e
            if form == "remove":
                assert len(new) == 0
            if form == "add":
                assert len(gone) == 0
            if form == "mix" and e > 1:
                assert len(gone) and len(new)
        sizes = collections.Counter((e, form) for _, e, form in lists)
        assert all(sizes[(e, form)] == 2 for e in hc.EXC_SIZES for form in hc.EXC_FORMS) and sizes[(0, "exact")] == 12


@pytest.mark.parametrize("n_dense,rare", [(64, R), (65, R), (900, R), (64, 1024), (65, 1024)])
def test_signature_groups_make_the_pattern_count_exact(n_dense, rare):
    """Restates build_patterns from the design: signature = smallest mix32 on the list; a group of four or more long lists gets a
    pattern, its most frequent exact list.  Exactly the three lineages form such groups, their pattern is the lineage's exact list,
    and every lineage list is in its lineage's group -- so the lists within 14 genomes of it are the pattern lists, as expected_index
    says."""
    d = design(n_dense)
    long_lists = {h: m for h, m in d.members.items() if hc.SHORT_LIST < len(m) <= rare}
    groups = collections.defaultdict(list)
    for h, m in long_lists.items():
        groups[hc.signature(m)].append(h)
    big = {s: hs for s, hs in groups.items() if len(hs) >= hc.PAT_GROUP_MIN}
    assert sorted(big) == sorted(hc.signature(L) for L, _ in d.lineages)
    n_pat_lists = 0
    for L, lists in d.lineages:
        hs = big[hc.signature(L)]
        assert {h for h, _, _ in lists} <= set(hs)
        exact = collections.Counter(d.members[h].tobytes() for h in hs)
        (best, count), = exact.most_common(1)
        assert best == L.astype(np.int64).tobytes() and count == 12 and sorted(exact.values())[-2] < 12
        n_pat_lists += sum(len(np.setxor1d(d.members[h], L)) <= hc.PAT_EXC_MAX for h in hs)
    exp = hc.expected_index(d, rare)
    assert exp["patterns"] == dict(long_lists=len(long_lists), patterns=3, pattern_lists=n_pat_lists)
    assert n_pat_lists == 3 * (12 + 2 * 3 * 5)
    assert exp["patterns"]["pattern_lists"] * 10 < exp["patterns"]["long_lists"] * 9     # the transposed bit rows are built by default
    assert exp["patterns"]["pattern_lists"] * 8 >= exp["patterns"]["long_lists"]          # ... and the patterns are kept


def test_expected_index_figures():
    d = design(64)
    e = hc.expected_index(d, R)
    assert e["rare_index"]["keys"] == len(d.members) and e["rare_index"]["rare_keys"] == len(d.members) - 64
    assert e["rare_index"]["postings"] == sum(len(m) for m in d.members.values() if len(m) <= R)
    assert e["static_dense"] == (True, 64) and hc.expected_index(design(65), R)["static_dense"] == (True, 65)
    assert hc.expected_index(design(900), R)["static_dense"] == (False, 0)
    assert hc.expected_index(d, 1024)["static_dense"] == (True, 32)      # only the hashes of N - 1 and N genomes stay dense
    assert hc.expected_index(d, 0)["rare_index"]["keys"] == 0
    for which, n_lifted in (("ff", 1), ("fe", 1), ("both", 2)):
        big, small = hc.expected_index(hc.lifted_design(600, which), R), hc.expected_index(hc.lifted_design(20, which), R)
        assert big["n_dense"] == 15 and big["static_dense"] == (True, 64 + n_lifted)
        assert small["n_dense"] == 0 and small["static_dense"] == (True, n_lifted)
    sp = hc.species_design()
    e = hc.expected_index(sp, R)
    assert e["n_dense"] == 12 and e["static_dense"] == (True, 64 + 1) and e["patterns"]["long_lists"] == 36 < hc.PAT_MIN_LONG
    assert e["rare_index"]["rare_keys"] == e["rare_index"]["keys"] - 12
    forced = [h for cls in sp.classes if cls.startswith("forced") for h in sp.classes[cls]]
    assert len(forced) == 24 and all(len(sp.members[h]) > R for h in forced)


def test_design_counts_are_the_oracles_single_species():
    d = design(64)
    refs, col_lens = hc.build_reference(d)
    names, q, qlen = hc.class_queries(d)
    assert len(names) == len(d.classes) + 1 + 4 + 1 + 3 + 2
    counts = hc.design_counts(d, q, qlen)
    np.testing.assert_array_equal(counts, hc.oracle_counts(refs, col_lens, q, qlen))
    by = dict(zip(names, counts))
    assert by[f"dense{N}"].min() == 16 and by["absent"].max() == 0 and by["empty"].max() == 0
    assert by["column0"][0] == col_lens[0][0] and by["lineages"][236:276].min() > 30 > np.median(by["lineages"])
    assert all(by[cls].max() > 0 for cls in d.classes)


@pytest.mark.parametrize("n_genomes", (600, 20))
@pytest.mark.parametrize("which", ("ff", "fe", "both"))
def test_design_counts_are_the_oracles_lifted(which, n_genomes):
    d = hc.lifted_design(n_genomes, which)
    refs, col_lens = hc.build_reference(d)
    _ascending(refs, col_lens)
    names, q, qlen = hc.lifted_queries(d)
    counts = hc.design_counts(d, q, qlen)
    np.testing.assert_array_equal(counts, hc.oracle_counts(refs, col_lens, q, qlen))
    by = dict(zip(names, counts))
    assert by["FD"].max() == 0
    assert by["FF"].sum() == (0 if which == "fe" else 3) and by["FE"].sum() == (0 if which == "ff" else 3)
    assert by["FE+FF"].max() == (2 if which == "both" else 1)
    if n_genomes == 600 and which != "fe":
        holders = np.nonzero(by["FF"])[0]
        assert len(set(holders // hc.TILE)) == 3 and len(set(holders // hc.GROUP)) == 2


def test_design_counts_are_the_oracles_species():
    d = hc.species_design()
    refs, col_lens = hc.build_reference(d)
    _ascending(refs, col_lens)
    assert [len(r) for r in refs] == [70, 600, 3] and 100 <= refs[0].shape[1] <= 300
    assert int(refs[2][2, col_lens[2][2] - 1]) == hc.FF and sum(int(r[g, c[g] - 1]) == hc.FF for r, c in zip(refs, col_lens) for g in range(len(r))) == 1
    names, q, qlen = hc.class_queries(d)
    counts = hc.design_counts(d, q, qlen)
    np.testing.assert_array_equal(counts, hc.oracle_counts(refs, col_lens, q, qlen))
    by = dict(zip(names, counts))
    assert by["forced_all"].min() == 12 and by["lifted_ff"].sum() == 1 and by["lifted_ff"][-1] == 1
    assert by["dense200_sp1"][:70].max() == 0 and by["dense200_sp1"][70:670].max() > 0


def test_reads_hit_every_class_and_the_leader_changes():
    """the stream the GPU tests push: 1 200 reads of 300 bases from the design's genome"""
    d = design(64)
    refs, col_lens = hc.build_reference(d)
    bases, offsets = hc.reads(d)
    s = refs[0].shape[1]
    e = orc.stream(16, 0, s, refs[0], col_lens[0], bases, offsets, top_k=1, want_sketches=True)
    seen = set(e["sketches"][np.arange(s)[None, :] < e["sketch_len"][:, None]].tolist())
    hit = collections.defaultdict(bool)
    for cls, hs in d.classes.items():   # (a lineage's classes hold two hashes each: counted per lineage and per kind of exception)
        for key in (cls.split("_") if cls.startswith("lineage") else [cls]):
            hit[key] |= bool(seen & set(hs))
    assert all(hit.values()), [k for k, v in hit.items() if not v]
    assert len(hit) == 11 + 4 + 1 + 3 + 1 + 21
    assert len(set(e["topk_idx"][:, 0].tolist())) > 1
