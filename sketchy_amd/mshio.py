"""Mash `.msh` writer for large collections (un-packed Cap'n Proto, one segment): what bench.py / tools hand the C++ host when
they need a species-scale reference on disk -- 40 000 sketches x 10 000 hashes are 3.2 GB, and a writer that goes through
Python integers (tests/mshio.py, the tests' independent one) takes minutes for that.  Same layout as
sketchy_amd/host/formats.hpp::write_mash_file and tests/mshio.py ([UPSTREAM-RECALL] Mash's MinHash.capnp): root struct 3 data
words + 4 pointers, hashSeed at byte 20 stored XOR 42, referenceList = pointer 3, Reference = 3 data words + 7 pointers
(name 2, comment 3, hashes64 5, counts32 6).  Words are laid out as: header, reference table, then per reference its name, its (empty)
comment, its hashes and -- when given -- its counts (4-byte elements, two per word); every position is computed up front, the hashes go
out with ndarray.tofile.  read_msh is the matching reader (one segment, near pointers: what these writers and the host's produce)."""
import struct

import numpy as np


def _sptr(off, dw, pw):
    return ((off << 2) & 0xFFFFFFFF) | (dw << 32) | (pw << 48)


def _lptr(off, code, count):
    return (((off << 2) & 0xFFFFFFFF) | 1) | (code << 32) | (count << 35)


def write_msh(path, names, hashes, col_len=None, kmer=16, seed=0, lengths=None, counts=None, num_valid_kmers=None):
    """names: list[str]; hashes: [n, s] uint64 array (row g = sketch g, ascending; the first col_len[g] entries count).
    counts: [n, s] uint32 (or None): the hashes' abundances, written as every reference's counts32 (same lengths as the hashes)."""
    hashes = np.ascontiguousarray(hashes, np.uint64)
    n, s = hashes.shape
    if counts is not None:
        counts = np.ascontiguousarray(counts, np.uint32)
        if counts.shape != hashes.shape:
            raise ValueError("counts must have the shape of hashes")
    if len(names) != n:
        raise ValueError("one name per sketch")
    lens = np.full(n, s, np.int64) if col_len is None else np.asarray(col_len, np.int64)
    enc = [nm.encode() for nm in names]
    name_words = np.array([(len(b) + 1 + 7) // 8 for b in enc], np.int64)
    esz, head = 10, 1 + 3 + 4 + 1            # root pointer + root struct + ReferenceList struct
    tag = head
    body0 = tag + 1 + n * esz
    cnt_words = (lens + 1) // 2 if counts is not None else np.zeros(n, np.int64)
    per = name_words + 1 + lens + cnt_words  # name, one word of empty comment text, hashes, counts
    start = body0 + np.concatenate(([0], np.cumsum(per)[:-1]))
    total = int(body0 + per.sum())
    if total - 1 >= (1 << 29):
        raise ValueError("collection too large for one Cap'n Proto segment")
    w = np.zeros(body0, np.uint64)
    w[0] = _sptr(0, 3, 4)
    w[1] = kmer
    w[3] = ((seed ^ 42) & 0xFFFFFFFF) << 32
    rl = 1 + 3 + 4
    w[1 + 3 + 3] = _sptr(rl - (1 + 3 + 3) - 1, 0, 1)
    w[rl] = _lptr(tag - rl - 1, 7, n * esz)
    w[tag] = (n << 2) | (3 << 32) | (7 << 48)
    e = tag + 1 + np.arange(n, dtype=np.int64) * esz
    ln = np.zeros(n, np.int64) if lengths is None else np.asarray(lengths, np.int64)
    w[e + 0] = np.minimum(ln, 0xFFFFFFFF).astype(np.uint64)
    w[e + 1] = ln.astype(np.uint64)
    if num_valid_kmers is not None:
        w[e + 2] = np.asarray(num_valid_kmers, np.uint64)

    def lptr_vec(at, slot, code, count):
        off = (at - slot - 1).astype(np.int64)
        return ((off << 2) & 0xFFFFFFFF).astype(np.uint64) | np.uint64(1) | (np.uint64(code) << np.uint64(32)) | (count.astype(np.uint64) << np.uint64(35))

    name_cnt = np.array([len(b) + 1 for b in enc], np.int64)
    w[e + 3 + 2] = lptr_vec(start, e + 3 + 2, 2, name_cnt)
    w[e + 3 + 3] = lptr_vec(start + name_words, e + 3 + 3, 2, np.ones(n, np.int64))
    w[e + 3 + 5] = lptr_vec(start + name_words + 1, e + 3 + 5, 5, lens)
    if counts is not None:
        w[e + 3 + 6] = lptr_vec(start + name_words + 1 + lens, e + 3 + 6, 4, lens)
    zero = np.zeros(1, np.uint64)
    with open(path, "wb") as f:
        f.write(struct.pack("<II", 0, total))
        w.tofile(f)
        for g in range(n):
            b = enc[g]
            f.write(b + b"\0" * (int(name_words[g]) * 8 - len(b)))
            zero.tofile(f)
            hashes[g, :int(lens[g])].tofile(f)
            if counts is not None:
                c = np.zeros(int(cnt_words[g]) * 2, np.uint32)
                c[:int(lens[g])] = counts[g, :int(lens[g])]
                c.tofile(f)


def read_msh(path):
    """(kmer, seed, [dict(name, length, num_valid_kmers, hashes uint64, counts uint32)]): counts is empty when the reference has no
    counts32 list.  One segment, near pointers."""
    raw = np.fromfile(path, np.uint8)
    nseg, seg_words = struct.unpack_from("<II", raw, 0)
    if nseg != 0 or 8 + 8 * seg_words > len(raw):
        raise ValueError("not a single-segment Cap'n Proto message: " + path)
    w = raw[8:8 + 8 * seg_words].view(np.uint64)

    def follow(at):
        """pointer word at `at` -> (kind, first content word, a, b): struct (0, pos, data words, pointer words), list (1, pos, element
        code, count), or None"""
        p = int(w[at])
        if p == 0:
            return None
        off = (p & 0xFFFFFFFF) >> 2
        off -= (1 << 30) if off >= (1 << 29) else 0
        pos = at + 1 + off
        if p & 3 == 0:
            return 0, pos, (p >> 32) & 0xFFFF, (p >> 48) & 0xFFFF
        if p & 3 == 1:
            return 1, pos, (p >> 32) & 7, p >> 35
        raise ValueError("far pointers are not supported")

    def scalars(at, code, dtype):
        l = follow(at)
        if l is None or l[0] != 1 or l[2] != code:
            return np.zeros(0, dtype)
        _, pos, _, count = l
        size = np.dtype(dtype).itemsize
        if pos < 0 or pos * 8 + count * size > len(w) * 8:
            raise ValueError("list exceeds the segment")
        return w[pos:pos + (count * size + 7) // 8].view(dtype)[:count].copy()

    root = follow(0)
    if root is None or root[0] != 0:
        raise ValueError("not a Mash sketch file: " + path)
    _, rpos, rdw, rpw = root
    kmer = int(w[rpos]) & 0xFFFFFFFF
    seed = ((int(w[rpos + 2]) >> 32) & 0xFFFFFFFF) ^ 42
    refs = []
    rl = follow(rpos + rdw + 3) if rpw > 3 else None
    lst = follow(rl[1] + rl[2]) if rl is not None and rl[0] == 0 and rl[3] > 0 else None
    if lst is not None:
        if lst[0] != 1 or lst[2] != 7:
            raise ValueError("reference list is not a struct list")
        tag = int(w[lst[1]])
        n, dw, pw = (tag >> 2) & 0x3FFFFFFF, (tag >> 32) & 0xFFFF, (tag >> 48) & 0xFFFF
        for i in range(n):
            e = lst[1] + 1 + i * (dw + pw)
            length = int(w[e + 1]) or int(w[e]) & 0xFFFFFFFF
            refs.append(dict(name=scalars(e + dw + 2, 2, np.uint8)[:-1].tobytes().decode(), length=length, num_valid_kmers=int(w[e + 2]),
                             hashes=scalars(e + dw + 5, 5, np.uint64), counts=scalars(e + dw + 6, 4, np.uint32) if pw > 6 else np.zeros(0, np.uint32)))
    return kmer, seed, refs
