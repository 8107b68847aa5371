"""Expectations for the composition of a stream (skx_stream_enable_composition), from the oracle alone, and the design and builders
the composition tests share (tests/test_composition_cpu.py, tests/test_gpu_composition.py, tests/composition_worker.py).

    hits[r][sp] = |{h in K_r : some genome of species sp holds h inside its col_len}|,  K_r = orc.sketch(read r, K, SEED, s)
    best = max hits[r];  best < min_hits -> unclassified;  one species attains best -> that species;  several -> ambiguous
    reads[n_species + 2] = reads per species, ambiguous, unclassified;  pairs[sp] = sum over the reads of hits[r][sp]

The hash -> species-mask dict comes from refs / col_lens; nothing of the library is involved.

The design.  hc.species_design() with its 300-base reads is vacuous here: every read holds one of the hashes all genomes share and
more of species 1's than of anybody's, so all of them fall to species 1 at every min_hits.  balanced_design() gives three species
(70, 600, 3 genomes) comparable shares of one genome's hashes and reads of 40 bases (25 k-mers) carry a handful of them: every class
holds reads, ties are common, and min_hits = 3 moves reads out of every species."""
import functools

import numpy as np

import hash_classes as hc
from helpers import unpack_reads
from sketchy_amd import synth

K, SEED = hc.K, hc.SEED
SIZES = (70, 600, 3)
CUTS = (0, 250, 251)   # ... and the end of the batch
N_DESIGN, N_OTHER, N_SHORT = 600, 50, 5


def balanced_design(sizes=SIZES, R=hc.R_TEST):
    """12 hashes in every genome, 12 in 200 genomes of species 1 (dense), the others by i % 12: 0-2 a short list inside species 0, 3-5
    inside species 1, 6-7 inside species 2, 8 a list in species 0 plus one in species 1, 9 a list in species 1 plus one in species 2,
    10-11 nobody's (they are not in the reference at all)."""
    genome, hashes = hc.genome_hashes(3000)
    d = hc.Design(sizes, genome)
    d.R = R
    first = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    rng = np.random.default_rng(17)
    pool = [int(h) for h in rng.permutation(hashes)]

    def short(sp):
        n = int(rng.integers(1, min(sizes[sp], hc.SHORT_LIST) + 1))
        return first[sp] + rng.choice(sizes[sp], n, replace=False)
    for h in pool[:12]:
        d.add("everybody", h, np.arange(sum(sizes)))
    for h in pool[12:24]:
        d.add("dense200_sp1", h, first[1] + rng.choice(sizes[1], 200, replace=False))
    d.nobody = []
    for i, h in enumerate(pool[24:]):
        c = i % 12
        if c <= 2:
            d.add("list_sp0", h, short(0))
        elif c <= 5:
            d.add("list_sp1", h, short(1))
        elif c <= 7:
            d.add("list_sp2", h, short(2))
        elif c == 8:
            d.add("list_sp0+1", h, np.concatenate([short(0), short(1)]))
        elif c == 9:
            d.add("list_sp1+2", h, np.concatenate([short(1), short(2)]))
        else:
            d.nobody.append(h)
    return d


def many_species_design(n_species=40, R=hc.R_TEST, block=36):
    """n_species species of two genomes over one genome's k-mers, by POSITION (a read of 40 bases then lies in one or two blocks):
    block b = position // 36 is species b % (n_species + 1)'s -- the last residue: held by species j = (b // (n_species + 1)) % n_species
    and by species (j + 1) % n_species"""
    genome = synth.random_genome(3000, np.random.default_rng(0))
    d = hc.Design([2] * n_species, genome)
    d.R = R
    for pos, h in enumerate(synth.canonical_kmer_hashes(genome, K, SEED).tolist()):
        if h in d.members:
            continue
        b = pos // block
        c = b % (n_species + 1)
        if c < n_species:
            d.add("one", h, [2 * c + pos % 2])
        else:
            j = (b // (n_species + 1)) % n_species
            d.add("two", h, [2 * j, 2 * ((j + 1) % n_species) + 1])
    return d


def species_masks(refs, col_lens):
    """{hash: bit sp set when a genome of species sp holds it inside its col_len}; the lifted values count for nobody"""
    masks = {}
    for sp, (ref, col_len) in enumerate(zip(refs, col_lens)):
        valid = np.arange(ref.shape[1])[None, :] < np.asarray(col_len)[:, None]
        for h in np.unique(ref[valid]).tolist():
            if h < hc.FE:
                masks[h] = masks.get(h, 0) | (1 << sp)
    return masks


def sketch_hits(masks, n_species, sketches):
    """hits [n_reads, n_species] int64 of reads given as their sketches (iterables of hashes)"""
    hits = np.zeros((len(sketches), n_species), np.int64)
    for r, sk in enumerate(sketches):
        for h in sk:
            m = masks.get(int(h), 0)
            for sp in range(n_species):
                hits[r, sp] += (m >> sp) & 1
    return hits


def read_hits(masks, n_species, bases, offsets, s):
    """the same, read by read from the oracle's sketch"""
    from oracle import oracle as orc
    return sketch_hits(masks, n_species, [orc.sketch(seq, K, SEED, s) for seq in unpack_reads(bases, offsets)])


def classes(hits, min_hits):
    """class per read: the species, n_species = ambiguous, n_species + 1 = unclassified"""
    n_sp = hits.shape[1]
    best = hits.max(axis=1)
    ties = (hits == best[:, None]).sum(axis=1)
    return np.where(best < min_hits, n_sp + 1, np.where(ties == 1, hits.argmax(axis=1), n_sp))


def composition(hits, min_hits, a=0, b=None):
    """(reads [n_species + 2], pairs [n_species]) uint64 of the reads [a, b)"""
    h = hits[a:b]
    n_sp = hits.shape[1]
    return (np.bincount(classes(h, min_hits), minlength=n_sp + 2).astype(np.uint64), h.sum(axis=0).astype(np.uint64))


@functools.lru_cache(maxsize=None)
def balanced():
    """(design, refs, col_lens, bases, offsets, hits): the design's 600 reads of 40 bases, 50 reads of 300 bases of an unrelated genome
    (all unclassified) and 5 reads of 15 bases (no k-mer); hits at the reference's own s"""
    d = balanced_design()
    refs, col_lens = hc.build_reference(d)
    b0, o0 = synth.make_reads(d.genome, N_DESIGN, 40, err=0.02, rng_seed=11)
    b1, o1 = synth.make_reads(synth.random_genome(3000, np.random.default_rng(5)), N_OTHER, 300, err=0.0, rng_seed=12)
    b2, o2 = synth.make_reads(d.genome, N_SHORT, 15, err=0.0, rng_seed=13)
    bases = np.concatenate([b0, b1, b2])
    offsets = np.concatenate([o0, o0[-1] + o1[1:], o0[-1] + o1[-1] + o2[1:]]).astype(np.uint64)
    hits = read_hits(species_masks(refs, col_lens), len(SIZES), bases, offsets, refs[0].shape[1])
    for x in (*refs, *col_lens, bases, offsets, hits):
        x.setflags(write=False)
    return d, refs, col_lens, bases, offsets, hits


def reads_from_hashes(genome, wanted, n_max=200):
    """one 16-base read (one k-mer) per position of `genome` whose canonical hash is in `wanted`: reads built only from those hashes"""
    hs = synth.canonical_kmer_hashes(genome, K, SEED)
    pos = [i for i, h in enumerate(hs.tolist()) if h in wanted][:n_max]
    bases = np.concatenate([genome[i:i + K] for i in pos])
    return np.ascontiguousarray(bases), (np.arange(len(pos) + 1) * K).astype(np.uint64)


def stream(R, bases, n, top=0):
    from sketchy_amd import api
    return api.SumOfSharedHashes(R, top=top, max_batch_reads=max(1, n), max_batch_bases=max(1, len(bases)))


def check(S, exp, what=""):
    reads, pairs = S.composition()
    assert reads.dtype == np.uint64 and pairs.dtype == np.uint64
    np.testing.assert_array_equal(reads, exp[0], err_msg=f"{what} reads")
    np.testing.assert_array_equal(pairs, exp[1], err_msg=f"{what} pairs")


def check_pushes(R, bases, offsets, hits, min_hits, cuts, top=1, what=""):
    """synchronous pushes cut at `cuts` on a stream with composition, the query after every cut; returns (rows per push, table)"""
    n = len(offsets) - 1
    S = stream(R, bases, n, top=top)
    try:
        S.enable_composition(min_hits)
        S.enable_composition(min_hits)   # (a second call with the same value changes nothing)
        parts = []
        for a, b in zip(cuts[:-1], cuts[1:]):
            parts.append(S.push(bases, offsets[a:b + 1]))
            check(S, composition(hits, min_hits, 0, b), what=f"{what} min_hits={min_hits} after {b} reads")
        return parts, S.table()
    finally:
        S.close()


def cli_lines(names, exp):
    reads, pairs = exp
    total = int(reads.sum())
    lines = [f"{nm}\t{int(reads[i])}\t{(int(reads[i]) / total if total else 0.0):.6f}\t{int(pairs[i])}" for i, nm in enumerate(names)]
    for nm, v in (("ambiguous", reads[-2]), ("unclassified", reads[-1])):
        lines.append(f"{nm}\t{int(v)}\t{(int(v) / total if total else 0.0):.6f}\t-")
    return lines
