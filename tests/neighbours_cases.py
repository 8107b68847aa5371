"""What tests/test_neighbours_cpu.py and tests/test_gpu_neighbours.py share: the 40-genome sketch file of the CLI tests and the text
`sketchy-hip neighbours` has to print for it, computed from the oracle alone -- counts from orc.common_hashes over all pairs, rows from
orc.stable_rank of a genome's counts with its own entry deleted (indices above it shifted back), the vote with ties to the smallest string."""
import collections
import functools

import numpy as np

from mshio import write_msh
from oracle import oracle as orc

N_CLI = 40
COLUMNS = ("mlst", "res")


def pair_counts(cols):
    """[n, n] uint32: |cols[g] & cols[h]| by the oracle, every pair"""
    n = len(cols)
    out = np.zeros((n, n), np.uint32)
    for g in range(n):
        for h in range(g, n):
            out[g, h] = out[h, g] = orc.common_hashes(cols[g], cols[h])
    return out


def loo_rows(counts, top, first=0, count=None):
    """(idx, shared) [count, top] of the leave-one-out ranking inside one species' square count matrix"""
    n = len(counts)
    count = n - first if count is None else count
    idx, val = np.zeros((count, top), np.uint32), np.zeros((count, top), np.uint32)
    for i, g in enumerate(range(first, first + count)):
        c = np.delete(counts[g], g)
        order = orc.stable_rank(c.astype(np.uint64))[:top].astype(np.int64)
        val[i] = c[order]
        idx[i] = order + (order >= g)
    return idx, val


@functools.lru_cache(maxsize=None)
def cli_genomes():
    """40 sketches of at most 30 hashes in five clusters (a few hashes swapped per genome, so ties are common); 23 is a copy of 7, 11 is
    empty, 13 is the first 12 hashes of 2; two genotype columns, the second all distinct in places so that votes tie."""
    rng = np.random.default_rng(97)
    bases = [np.sort(rng.choice(2 ** 40, size=30, replace=False).astype(np.uint64)) for _ in range(5)]
    hs = []
    for i in range(N_CLI):
        h = bases[i % 5].copy()
        swap = rng.choice(30, size=int(rng.integers(0, 4)), replace=False)
        h[swap] = rng.choice(2 ** 40, size=len(swap), replace=False).astype(np.uint64)
        hs.append(np.unique(h))
    hs[23] = hs[7].copy()
    hs[11] = np.zeros(0, np.uint64)
    hs[13] = hs[2][:12].copy()
    names = [f"genome{i:02d}.fa" for i in range(N_CLI)]
    geno = [(f"ST{(i % 5) if i % 9 else 7}", f"R{i % 3}") for i in range(N_CLI)]
    return names, hs, geno


def write_cli_files(d):
    names, hs, geno = cli_genomes()
    msh, tsv = str(d / "ref.msh"), str(d / "geno.tsv")
    write_msh(msh, names, hs, kmer=16, seed=0, lengths=[1000] * len(names))
    with open(tsv, "w") as f:
        f.write("id\t" + "\t".join(COLUMNS) + "\n" + "".join(f"{nm}\t" + "\t".join(g) + "\n" for nm, g in zip(names, geno)))
    return msh, tsv


@functools.lru_cache(maxsize=None)
def cli_counts():
    return pair_counts(cli_genomes()[1])


def _vote(geno, row):
    call = []
    for j in range(len(COLUMNS)):
        votes = collections.Counter(geno[g][j] for g in row)
        best = max(votes.values())
        call.append(min(v for v, c in votes.items() if c == best))   # ties: the smallest string
    return call


def expected_rows(top, with_geno):
    names, _, geno = cli_genomes()
    idx, val = loo_rows(cli_counts(), top)
    return "".join(f"{names[g]}\t{names[h]}\t{c}" + ("\t" + "\t".join(geno[h]) if with_geno else "") + "\n"
                   for g in range(N_CLI) for h, c in zip(idx[g], val[g]))


def expected_consensus(top):
    names, _, geno = cli_genomes()
    idx, _ = loo_rows(cli_counts(), top)
    return "".join(f"{names[g]}\t-\t-\t" + "\t".join(_vote(geno, idx[g])) + "\n" for g in range(N_CLI))


def expected_summary(top):
    _, _, geno = cli_genomes()
    idx, _ = loo_rows(cli_counts(), top)
    calls = [_vote(geno, idx[g]) for g in range(N_CLI)]
    return "".join(f"{col}\t{sum(calls[g][j] == geno[g][j] for g in range(N_CLI))}\t{N_CLI}\n" for j, col in enumerate(COLUMNS))
