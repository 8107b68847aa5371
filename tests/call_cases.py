"""The species call restated on the CPU (include/sketchy_hip.h, skx_stream_bind_call): what tests/test_call_cpu.py pins against a literal
per-read loop and what tests/test_gpu_call_rows.py and tests/test_gpu_call.py hold the device to.

  call_ref(idx, sums, codes=None)          per read the lowest species with the largest leader sums[r, sp, 0], and its rows
  call_changes_ref(species, part)          the reads at which the call changes: read 0, a new species, or a new compared part
  call_loop / call_changes_loop            the same, read by read in plain Python
  planted_rows(...)                        random rows with the ties the tie rule is about planted in them"""
import numpy as np


def call_ref(idx, sums, codes=None):
    """idx uint32 / sums uint64 [n, n_species, top], codes [n, n_species, F] or None ->
    dict(call_species [n], call_idx [n, top], call_sum [n, top], call_codes [n, F] or None)"""
    idx, sums = np.asarray(idx, np.uint32), np.asarray(sums, np.uint64)
    n = idx.shape[0]
    lead = sums[:, :, 0]
    sp = np.argmax(lead, axis=1).astype(np.uint32) if n else np.zeros(0, np.uint32)  # (argmax: the FIRST maximum)
    rows = np.arange(n)
    return dict(call_species=sp, call_idx=idx[rows, sp], call_sum=sums[rows, sp],
                call_codes=None if codes is None else np.asarray(codes, np.uint32)[rows, sp])


def call_changes_ref(species, part):
    """species [n], part [n, w] (the index rows, or the codes in codes mode) -> ascending reads r with r == 0, species[r] != species[r-1]
    or part[r] != part[r-1] in any element"""
    species, part = np.asarray(species), np.asarray(part)
    n = species.shape[0]
    if n == 0:
        return np.zeros(0, np.int64)
    flag = np.ones(n, bool)
    if n > 1:  # (reshape(0, -1) cannot size an empty array)
        flag[1:] = (species[1:] != species[:-1]) | (part[1:] != part[:-1]).reshape(n - 1, -1).any(axis=1)
    return np.flatnonzero(flag)


def call_loop(idx, sums, codes=None):
    n, n_sp, top = idx.shape
    sp_out, idx_out, sum_out, codes_out = [], [], [], []
    for r in range(n):
        best, c = -1, 0
        for sp in range(n_sp):
            lead = int(sums[r][sp][0])
            if lead > best:  # (strictly greater: the lowest species keeps a tie)
                best, c = lead, sp
        sp_out.append(c)
        idx_out.append([int(v) for v in idx[r][c]])
        sum_out.append([int(v) for v in sums[r][c]])
        if codes is not None:
            codes_out.append([int(v) for v in codes[r][c]])
    return sp_out, idx_out, sum_out, (codes_out if codes is not None else None)


def call_changes_loop(species, part):
    ev = []
    for r in range(len(species)):
        if r == 0 or int(species[r]) != int(species[r - 1]) or [int(v) for v in part[r]] != [int(v) for v in part[r - 1]]:
            ev.append(r)
    return ev


def planted_rows(n, n_sp, top, n_feat=0, seed=0):
    """Random rows [n, n_sp, top] whose sums descend along a row and reach from 0 across 2^32 up to 2^54 - 1, with planted: equal
    leads in two, three and all species (at the maximum, so that the tie decides), all-zero leads, runs of repeated reads (so that
    change points are neither everywhere nor nowhere), and a lone change in the last element of a row.  Returns (idx, sums, codes|None)."""
    rng = np.random.default_rng(seed)
    scale = rng.choice(np.array([1 << 8, 1 << 31, 1 << 33, 1 << 54], np.uint64), size=(n, 1, 1))
    sums = (rng.integers(0, 1 << 62, size=(n, n_sp, top), dtype=np.uint64) % scale).astype(np.uint64)
    sums = -np.sort(-sums.astype(np.int64), axis=2)  # descending along the row, as a ranking leaves them
    sums = sums.astype(np.uint64)
    idx = rng.integers(0, 1 << 20, size=(n, n_sp, top), dtype=np.uint32)
    codes = rng.integers(0, 5, size=(n, n_sp, n_feat), dtype=np.uint32) if n_feat else None
    for r in range(n):
        kind = r % 8
        hi = sums[r, :, 0].max()
        if kind == 1 and n_sp >= 2:      # two species share the largest lead
            a, b = rng.choice(n_sp, 2, replace=False)
            sums[r, a, 0] = sums[r, b, 0] = hi
        elif kind == 2 and n_sp >= 3:    # three
            for sp in rng.choice(n_sp, 3, replace=False):
                sums[r, sp, 0] = hi
        elif kind == 3:                  # all
            sums[r, :, 0] = hi
        elif kind == 4:                  # a table of zeros
            sums[r] = 0
        elif kind == 5:                  # the largest sum a table may hold, past 2^32, in the LAST species and one below it elsewhere
            sums[r, :, 0] = (1 << 54) - 2
            sums[r, n_sp - 1, 0] = (1 << 54) - 1
        elif kind == 6:                  # leads that differ only above bit 32 / only below it
            sums[r, :, 0] = (3 << 32) + 5
            sums[r, n_sp // 2, 0] = (4 << 32) + 1
            sums[r, 0, 0] = (4 << 32)
    for r in range(1, n):                # runs: a read that repeats the one before it, and one that differs in one place only
        if r % 5 in (1, 2):
            idx[r], sums[r] = idx[r - 1], sums[r - 1]
            if codes is not None:
                codes[r] = codes[r - 1]
        if r % 10 == 2:
            idx[r, :, top - 1] ^= 1      # (the last element of every species' row: the called one's among them)
            if codes is not None:
                codes[r, :, n_feat - 1] ^= 1
    return idx, sums, codes
