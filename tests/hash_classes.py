"""References built from a DESIGNED membership {hash: genomes that hold it}, so that every storage class skx_ref_create files a
reference hash into occurs, at its boundaries, in one small reference (tests/test_hash_classes_cpu.py, tests/test_gpu_hash_classes.py).

The hashes are the real canonical 16-mer hashes of one random genome and every hash of that genome is in the design: reads drawn
from the genome hit every class.  The classes (skx_capi.hip, "Rare-hash index"; skx_kernels.hip, "long lists as bit rows" and
"long lists as (pattern, exceptions)"), R being the policy "rare_hash_genomes" the reference is created under:

  list of <= 8 genomes         postings (kShortList)
  list of 9 .. R genomes       a bit row -- or a (pattern, <= 14 exceptions) record (kPatExcMax)
  more than R genomes          dense: a row of the static dictionary, found by the scan
  more than R, several species a list anyway ("multi" in the index build)
  >= 0xFFFFFFFFFFFFFFFE        lifted into the exception list; rows in the static dictionary's tail

What the index must report (ReferenceSketch.rare_index / .patterns / .static_dense) follows from the design alone: expected_index().
A long list joins the signature group of the genome with the smallest mix32 on it (list_sig_kernel), a group of four or more lists
gets a pattern (its most frequent exact list), and a list within 14 genomes of its group's pattern is stored as that pattern plus
exceptions.  The builder therefore keeps every lineage list inside its lineage's group and every other list of 9 .. 1024 genomes in a
group of at most two: exactly one pattern per lineage, and the pattern lists are the lineage lists with at most 14 exceptions."""
import numpy as np

from sketchy_amd import synth

FD, FE, FF = 0xFFFFFFFFFFFFFFFD, 0xFFFFFFFFFFFFFFFE, 0xFFFFFFFFFFFFFFFF
K, SEED = 16, 0
SHORT_LIST, PAT_EXC_MAX, PAT_GROUP_MIN, PAT_MIN_LONG = 8, 14, 4, 64
TILE, GROUP = 256, 512
R_TEST = 100                    # above 65: the lists of 63, 64 and 65 genomes stay lists
N_SINGLE = 1300                 # five tiles, three rank groups
LINEAGE_STARTS = (236, 492, 700)   # 40 consecutive genomes each: across genome 256, across genome 512, inside a tile
LINEAGE_LEN, EXC_SIZES, EXC_FORMS = 40, (1, 2, 7, 13, 14, 15, 16), ("remove", "add", "mix")


def mix32(x):
    """list_sig_kernel's mix32 on (padded) genome indices"""
    x = np.asarray(x, np.uint64) & np.uint64(0xFFFFFFFF)
    m = np.uint64(0xFFFFFFFF)
    x = ((x ^ (x >> np.uint64(16))) * np.uint64(0x7FEB352D)) & m
    x = ((x ^ (x >> np.uint64(15))) * np.uint64(0x846CA68B)) & m
    return (x ^ (x >> np.uint64(16))).astype(np.uint32)


def roundup64(n):
    return (int(n) + 63) // 64 * 64


def genome_hashes(length=6000):
    genome = synth.random_genome(length, np.random.default_rng(0))
    return genome, np.unique(synth.canonical_kmer_hashes(genome, K, SEED))


class Design:
    """members: {hash (int): sorted int64 array of genome indices, the species one after the other}; classes: {name: [hashes]};
    lineages: [(L, [(hash, exceptions, form)])] (one species only)."""

    def __init__(self, species, genome):
        self.species, self.genome = tuple(int(n) for n in species), genome
        self.members, self.classes, self.lineages = {}, {}, []

    @property
    def n_genomes(self):
        return sum(self.species)

    def add(self, cls, h, genomes):
        h = int(h)
        assert h not in self.members
        g = np.unique(np.asarray(genomes, np.int64))
        assert len(g) and g[0] >= 0 and g[-1] < self.n_genomes
        self.members[h] = g
        self.classes.setdefault(cls, []).append(h)

    def species_of(self, g):
        return np.searchsorted(np.cumsum(self.species), g, side="right")


def build_reference(design):
    """-> (refs, col_lens): per species [n, stride] uint64 ascending rows (zero behind col_len) and their lengths; one stride for all"""
    hs = np.fromiter(design.members.keys(), np.uint64, len(design.members))
    lens = np.array([len(design.members[int(h)]) for h in hs])
    g_all = np.concatenate([design.members[int(h)] for h in hs])
    h_all = np.repeat(hs, lens)
    order = np.lexsort((h_all, g_all))
    g_all, h_all = g_all[order], h_all[order]
    col_len = np.bincount(g_all, minlength=design.n_genomes).astype(np.uint32)
    stride = int(col_len.max())
    first = np.concatenate([[0], np.cumsum(col_len, dtype=np.int64)[:-1]]).astype(np.int64)
    ref = np.zeros((design.n_genomes, stride), np.uint64)
    ref[g_all, np.arange(len(g_all)) - first[g_all]] = h_all
    cuts = np.concatenate([[0], np.cumsum(design.species)])
    refs = [np.ascontiguousarray(ref[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
    return refs, [np.ascontiguousarray(col_len[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]


def signature(genomes):
    return int(mix32(genomes).min())


def expected_index(design, R):
    """dict(rare_index=..., patterns=..., static_dense=(flag, rows), n_dense, n_lifted) of a reference created under rare_hash_genomes = R
    with every other policy at its default"""
    if R == 0:
        return dict(rare_index=dict(keys=0, rare_keys=0, postings=0), patterns=dict(long_lists=0, patterns=0, pattern_lists=0),
                    static_dense=(False, 0), n_dense=0, n_lifted=0)
    keys = rare = postings = long_lists = 0
    dense_sp = [0] * len(design.species)
    lifted = 0
    for h, g in design.members.items():
        if h >= FE:
            lifted += 1
            continue
        keys += 1
        sp = np.unique(design.species_of(g))
        if len(g) <= R or (len(sp) > 1 and len(g) <= 1 << 18):
            rare += 1
            postings += len(g)
            long_lists += len(g) > SHORT_LIST
        else:
            dense_sp[int(sp[0])] += 1
    pat = dict(long_lists=int(long_lists), patterns=0, pattern_lists=0)
    if long_lists >= PAT_MIN_LONG and design.lineages:
        n = sum(len(np.setxor1d(design.members[h], L)) <= PAT_EXC_MAX for L, lists in design.lineages for h, _, _ in lists)
        if n * 8 >= long_lists:
            pat.update(patterns=len(design.lineages), pattern_lists=int(n))
    # build_static_dense: one sorted segment per species, each from a multiple of 64 on; the lifted hashes behind the last one
    cap_sp = 191 * build_reference(design)[0][0].shape[1] // 64
    static = all(d <= cap_sp for d in dense_sp)
    row = last = 0
    for d in dense_sp:
        last = row + d
        row = roundup64(row + d)
    rows = (row + lifted if lifted else last) if static else 0
    return dict(rare_index=dict(keys=keys, rare_keys=rare, postings=postings), patterns=pat, static_dense=(static, rows),
                n_dense=sum(dense_sp), n_lifted=lifted)


def _draw_grouped(rng, n, n_genomes, used, barred):
    """n random genomes whose signature no lineage has and at most one earlier list shares"""
    for _ in range(100000):
        g = np.sort(rng.choice(n_genomes, n, replace=False))
        s = signature(g)
        if s not in barred and used.get(s, 0) < 2:
            used[s] = used.get(s, 0) + 1
            return g
    raise AssertionError("no list of %d genomes with a free signature" % n)


def single_species(n_dense=64, R=R_TEST, n_genomes=N_SINGLE, per=12):
    """The single-species design.  n_dense: 64, 65 (the static dictionary's tail from row 64 / 128) or any larger number (more than
    build_static_dense takes: per-pass dictionaries).  The variants differ in the number of dense hashes only."""
    genome, hashes = genome_hashes()
    N = n_genomes
    d = Design([N], genome)
    d.R = R
    pool = [int(h) for h in np.random.default_rng(1).permutation(hashes)]
    at = 0

    def take(n):
        nonlocal at
        assert at + n <= len(pool)
        at += n
        return pool[at - n:at]

    # pattern lineages: the exact list 12 times, then L xor E -- a list stays in the lineage's signature group when it keeps the genome
    # of L with the smallest mix32 and adds none with a smaller one
    rng = np.random.default_rng(2)
    barred = set()
    for li, a in enumerate(LINEAGE_STARTS):
        L = np.arange(a, a + LINEAGE_LEN)
        mx = mix32(L)
        keep = L[np.argmin(mx)]
        barred.add(int(mx.min()))
        inside = L[L != keep]
        everyone = np.arange(N)
        outside = everyone[(mix32(everyone) > mx.min()) & ((everyone < a) | (everyone >= a + LINEAGE_LEN))]
        lists = []
        for h in take(per):
            d.add(f"lineage{li}_exact", h, L)
            lists.append((h, 0, "exact"))
        for e in EXC_SIZES:
            for form in EXC_FORMS:
                for h in take(2):
                    n_rm = e if form == "remove" else 0 if form == "add" else e // 2   # (mix of one exception: one outsider)
                    rm = rng.choice(inside, n_rm, replace=False)
                    ad = rng.choice(outside, e - n_rm, replace=False)
                    d.add(f"lineage{li}_{form}{e}", h, np.concatenate([np.setdiff1d(L, rm), ad]))
                    lists.append((h, e, form))
        d.lineages.append((L, lists))
    # dense hashes (more than R genomes) and plain lists, the longest first: they take the genomes with the smallest mix32 as signatures
    rng = np.random.default_rng(3)
    used = {}
    h_dense = {n: take(16) for n in (N, N - 1, 200, R + 1)}
    for h in h_dense[N]:
        d.add(f"dense{N}", h, np.arange(N))
    for h in h_dense[N - 1]:
        d.add(f"dense{N - 1}", h, np.delete(np.arange(N), rng.integers(N)))
    for n in (200, R + 1):
        for h in h_dense[n]:
            d.add(f"dense{n}", h, _draw_grouped(rng, n, N, used, barred))
    for n in (R, R - 1, 65, 64, 63, 10, 9):
        for h in take(per):
            d.add(f"list{n}", h, _draw_grouped(rng, n, N, used, barred))
    for n in (8, 7, 2, 1):
        for h in take(per):
            d.add(f"list{n}", h, rng.choice(N, n, replace=False))
    # everything else of the genome: lists of 1 to 5 genomes -- but for the last n_dense - 64 hashes, which are dense too
    rest = pool[at:]
    extra = n_dense - 64
    assert 0 <= extra < len(rest) - 1000
    rng_rest, rng_extra = np.random.default_rng(4), np.random.default_rng(5)
    for i, h in enumerate(rest):
        small = rng_rest.choice(N, int(rng_rest.integers(1, 6)), replace=False)
        if i < len(rest) - extra:
            d.add("rest", h, small)
        elif i == len(rest) - extra:
            d.add(f"dense{R + 1}", h, _draw_grouped(rng_extra, R + 1, N, used, barred))   # (the 65th: a list under the default policy)
        else:
            d.add(f"dense{R + 1}", h, rng_extra.choice(N, R + 1, replace=False))
    assert len(d.members) == len(hashes) and max(d.members) < FE
    return d


def add_lifted(design, ff=(), fe=()):
    """0xFF..FF / 0xFF..FE into the columns of the given genomes"""
    if len(ff):
        design.add("lifted_ff", FF, ff)
    if len(fe):
        design.add("lifted_fe", FE, fe)
    return design


def lifted_design(n_genomes, which, R=R_TEST):
    """One species; ordinary lists, a few dense hashes when n_genomes > R (a dense segment in front of the static dictionary's tail),
    and the lifted values: which = "ff" (held by genomes of three tiles and two rank groups), "fe", or "both" (different genomes
    and one common one)."""
    genome, hashes = genome_hashes(1500)
    N = n_genomes
    d = Design([N], genome)
    d.R = R
    rng = np.random.default_rng(6)
    for i, h in enumerate(hashes):
        if i % 100 == 0:
            d.add("dense", h, rng.choice(N, min(N, R + 1 + i // 100), replace=False))
        else:
            d.add("rest", h, rng.choice(N, int(rng.integers(1, SHORT_LIST + 1)), replace=False))
    spread = np.array([3, N // 2, N - 2])      # N = 600: tiles 0, 1, 2; rank groups 0, 0, 1
    other = np.array([N // 3, N - 2, N - 1])
    if which == "ff":
        add_lifted(d, ff=spread)
    elif which == "fe":
        add_lifted(d, fe=spread)
    else:
        add_lifted(d, ff=spread, fe=other)
    return d


def species_design(sizes=(70, 600, 3), R=R_TEST):
    """Several species that share one genome's hashes: a hash of 30 + 40 genomes of species 0 and 1 (more than R in all: a list
    anyway), hashes of every genome of every species, hashes of 200 genomes of species 1 alone (dense, in that species' segment),
    ordinary lists inside each species and across them, and 0xFF..FF in one genome of the last species."""
    genome, hashes = genome_hashes(3000)
    d = Design(sizes, genome)
    d.R = R
    first = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    n0, n1 = sizes[0], sizes[1]
    assert n0 >= 30 and n1 >= 200 and 30 + 40 <= R
    rng = np.random.default_rng(7)
    pool = [int(h) for h in rng.permutation(hashes)]
    for h in pool[:12]:
        d.add("forced30+%d" % (R - 29), h, np.concatenate([rng.choice(n0, 30, replace=False), first[1] + rng.choice(n1, R - 29, replace=False)]))
    for h in pool[12:24]:
        d.add("forced_all", h, np.arange(sum(sizes)))
    for h in pool[24:36]:
        d.add("dense200_sp1", h, first[1] + rng.choice(n1, 200, replace=False))
    for h in pool[36:48]:
        d.add("two_species_short", h, np.concatenate([rng.choice(n0, 30, replace=False), first[1] + rng.choice(n1, 40, replace=False)]))
    for i, h in enumerate(pool[48:]):
        sp = len(sizes) - 1 if i % 20 == 0 else 0 if i % 20 <= 4 else 1   # (few for the small last species: its columns stay short)
        n = int(rng.integers(1, min(sizes[sp], SHORT_LIST) + 1))   # (short lists only: fewer than 64 long lists, so no patterns)
        d.add("list_sp%d" % sp, h, first[sp] + rng.choice(sizes[sp], n, replace=False))
    add_lifted(d, ff=[first[-1] + sizes[-1] - 1])
    return d


def design_counts(design, q, qlen):
    """count[i, g] = |{h in query i : g in design[h]}|, from the design alone"""
    out = np.zeros((len(q), design.n_genomes), np.uint32)
    for i in range(len(q)):
        hit = [design.members[int(h)] for h in q[i, :qlen[i]] if int(h) in design.members]
        if hit:
            out[i] = np.bincount(np.concatenate(hit), minlength=design.n_genomes)
    return out


def oracle_counts(refs, col_lens, q, qlen):
    """the same counts from orc.common_hashes, genome by genome (the species one after the other)"""
    from oracle import oracle as orc
    ref, col_len = np.concatenate(refs), np.concatenate(col_lens)
    return np.array([[orc.common_hashes(ref[g, :col_len[g]], q[i, :qlen[i]]) for g in range(len(ref))] for i in range(len(q))],
                    np.uint32).reshape(len(q), len(ref))


def oracle_rows(counts, species, top):
    """[n_query, n_species, top] (idx, shared): the oracle's stable rank per species, indices local to the species"""
    from oracle import oracle as orc
    idx, val = np.zeros((len(counts), len(species), top), np.uint32), np.zeros((len(counts), len(species), top), np.uint32)
    g0 = 0
    for sp, n in enumerate(species):
        for i in range(len(counts)):
            c = counts[i, g0:g0 + n]
            order = orc.stable_rank(c.astype(np.uint64))[:top]
            idx[i, sp], val[i, sp] = order, c[order]
        g0 += n
    return idx, val


def pack_queries(rows):
    q, qlen = np.zeros((len(rows), max(1, max(len(r) for r in rows))), np.uint64), np.array([len(r) for r in rows], np.uint32)
    for i, r in enumerate(rows):
        q[i, :len(r)] = np.sort(np.asarray(r, np.uint64))
    return q, qlen


def class_queries(design, cap=400):
    """(names, q, qlen): one query per class (its hashes only, at most `cap` of them), the classes of every lineage together, mixed
    queries over every class, three genomes' own columns, hashes no genome holds (below the largest reference hash) and an empty one"""
    rng = np.random.default_rng(8)
    names, rows = [], []

    def some(hs):
        hs = np.array(sorted(hs), np.uint64)
        return hs if len(hs) <= cap else np.sort(rng.choice(hs, cap, replace=False))
    for cls, hs in design.classes.items():
        names.append(cls); rows.append(some(hs))
    lin = [h for cls, hs in design.classes.items() if cls.startswith("lineage") for h in hs]
    if lin:
        names.append("lineages"); rows.append(some(lin))
    ordinary = np.array(sorted(h for h in design.members if h < FE), np.uint64)
    top = int(ordinary[-1])
    absent = np.setdiff1d(rng.integers(1, top, size=300, dtype=np.uint64), ordinary)
    for i in range(4):   # every class, a fifth of the hashes nobody's
        names.append(f"mixed{i}")
        rows.append(np.concatenate([rng.choice(ordinary, cap - 80, replace=False), absent[80 * i // 2:80 * i // 2 + 80]]))
    per_class = [h for hs in design.classes.values() for h in hs[:3]]
    names.append("three_of_each"); rows.append(some(per_class))
    for g in (0, design.n_genomes // 2, design.n_genomes - 1):
        names.append(f"column{g}"); rows.append(np.array([h for h, m in design.members.items() if g in m], np.uint64))
    names.append("absent"); rows.append(absent)
    names.append("empty"); rows.append(np.zeros(0, np.uint64))
    q, qlen = pack_queries(rows)
    return names, q, qlen


def lifted_queries(design):
    """queries that end in [FE], [FF], [FE, FF], [FD] behind a genome's ordinary hashes, and those values alone"""
    base = np.array(sorted(h for h, m in design.members.items() if h < FE and 3 in m), np.uint64)
    tails = ([FE], [FF], [FE, FF], [FD])
    names = ["column3+" + "+".join("%X" % (t & 0xFF) for t in tail) for tail in tails] + ["FE", "FF", "FD", "FE+FF"]
    rows = [np.concatenate([base, np.array(t, np.uint64)]) for t in tails] + [np.array(t, np.uint64) for t in ([FE], [FF], [FD], [FE, FF])]
    q, qlen = pack_queries(rows)
    return names, q, qlen


def reads(design, n_reads=1200, read_len=300, err=0.02, rng_seed=9):
    return synth.make_reads(design.genome, n_reads, read_len, err=err, rng_seed=rng_seed)


# ---------------------------------------------------------------------------------------------------------------- device side
# (shared by tests/test_gpu_hash_classes.py and its child tests/hash_classes_worker.py; sketchy_amd.api is imported on use)
def create_reference(design, rare):
    """(ReferenceSketch, refs, col_lens) with the policy rare_hash_genomes = rare while the reference is created"""
    from sketchy_amd import api
    refs, col_lens = build_reference(design)
    before = api.get_option("rare_hash_genomes")
    api.set_option("rare_hash_genomes", rare)
    try:
        R = api.ReferenceSketch(refs[0], col_lens[0]) if len(refs) == 1 else api.ReferenceSketch(refs, col_lens)
    finally:
        api.set_option("rare_hash_genomes", before)
    return R, refs, col_lens


def index_figures(R):
    ri, pt = R.rare_index, R.patterns
    return dict(rare_index={k: ri[k] for k in ("keys", "rare_keys", "postings")},
                patterns={k: pt[k] for k in ("long_lists", "patterns", "pattern_lists")}, static_dense=R.static_dense)


def assert_index(R, design, rare):
    got, exp = index_figures(R), expected_index(design, rare)
    print("index figures (rare_hash_genomes = %d):" % rare, got)
    for k in ("rare_index", "patterns", "static_dense"):
        assert got[k] == exp[k], (k, got[k], exp[k])
    return got


def check_operators(R, species, q, qlen, counts, tops, what=""):
    """skx_common_hashes and skx_rank_sketches (rows, and the counts they were taken from) against `counts`"""
    np.testing.assert_array_equal(R.common_hashes(q, qlen), counts, err_msg=f"{what} common_hashes")
    for top in tops:
        idx, val = oracle_rows(counts, species, top)
        got = R.rank_sketches(q, qlen, top=top, want_common=True)
        np.testing.assert_array_equal(got[2], counts, err_msg=f"{what} rank_sketches top={top} counts")
        np.testing.assert_array_equal(got[1], val, err_msg=f"{what} rank_sketches top={top} shared")
        np.testing.assert_array_equal(got[0], idx, err_msg=f"{what} rank_sketches top={top} idx")


def check_pushes(R, exp, bases, offsets, top, cuts, what=""):
    """synchronous pushes with the per-read x per-genome counts: rows, counts and the table against the oracle's (exp: one
    orc.stream result per species); returns the stream's stats"""
    from sketchy_amd import api
    n = len(offsets) - 1
    S = api.SumOfSharedHashes(R, top=top, max_batch_reads=n, max_batch_bases=max(1, len(bases)))
    try:
        parts = [S.push(bases, offsets[a:b + 1], want_shared=True) for a, b in zip(cuts[:-1], cuts[1:])]
        ti = np.concatenate([p["topk_idx"] for p in parts]).reshape(n, len(exp), top)
        ts = np.concatenate([p["topk_sum"] for p in parts]).reshape(n, len(exp), top)
        np.testing.assert_array_equal(np.concatenate([p["shared"] for p in parts]), np.concatenate([e["shared"] for e in exp], axis=1),
                                      err_msg=f"{what} per-read shared")
        for i, e in enumerate(exp):
            np.testing.assert_array_equal(ts[:, i], e["topk_sum"], err_msg=f"{what} species {i} sums")
            np.testing.assert_array_equal(ti[:, i], e["topk_idx"], err_msg=f"{what} species {i} rows")
        np.testing.assert_array_equal(S.table(), np.concatenate([e["cum"] for e in exp]), err_msg=f"{what} table")
        return S.stats()
    finally:
        S.close()


def check_enqueued(R, exp, bases, offsets, top, cuts, what=""):
    """the same reads as device batches through enqueue_device (they share passes); rows and table; returns the stats"""
    from sketchy_amd import api
    n, n_sp = len(offsets) - 1, len(exp)
    # (room for all the reads' pairs: a pass holds max_batch_reads x 64 of them -- these reads bring ~80 each --, and a group of batches
    # beyond that is taken apart again and shares nothing)
    S = api.SumOfSharedHashes(R, top=top, max_batch_reads=2 * n, max_batch_bases=int(max(offsets[b] - offsets[a] for a, b in zip(cuts[:-1], cuts[1:]))))
    keep = [api.DeviceBuffer.from_numpy(bases)]
    try:
        rows = []
        for a, b in zip(cuts[:-1], cuts[1:]):
            d_o = api.DeviceBuffer.from_numpy(np.ascontiguousarray(offsets[a:b + 1]))
            d_i, d_s = api.DeviceBuffer((b - a) * n_sp * top * 4), api.DeviceBuffer((b - a) * n_sp * top * 8)
            keep += [d_o, d_i, d_s]
            rows.append((b - a, d_i, d_s))
            S.enqueue_device(keep[0].ptr, d_o.ptr, b - a, int(offsets[b] - offsets[a]), d_i.ptr, d_s.ptr)
        S.sync()
        ti = np.concatenate([d_i.to_numpy(np.uint32, (m, n_sp, top)) for m, d_i, _ in rows])
        ts = np.concatenate([d_s.to_numpy(np.uint64, (m, n_sp, top)) for m, _, d_s in rows])
        for i, e in enumerate(exp):
            np.testing.assert_array_equal(ts[:, i], e["topk_sum"], err_msg=f"{what} species {i} sums")
            np.testing.assert_array_equal(ti[:, i], e["topk_idx"], err_msg=f"{what} species {i} rows")
        np.testing.assert_array_equal(S.table(), np.concatenate([e["cum"] for e in exp]), err_msg=f"{what} table")
        return S.stats()
    finally:
        for d in keep:
            d.free()
        S.close()


def oracle_stream(refs, col_lens, bases, offsets, top):
    """one orc.stream per species over the same reads (reads are sketched with s = the stride, as ReferenceSketch does by default)"""
    from oracle import oracle as orc
    return [orc.stream(K, SEED, r.shape[1], r, c, bases, offsets, top_k=top, want_shared=True) for r, c in zip(refs, col_lens)]
