"""4-bit packed input at every supported k and seed, through every sketcher tier.

`sketchy-hip predict -s` feeds the device packed bases only, whatever the reference's k and seed; tests/test_gpu_packed.py
holds that format to the oracle at k = 16, seed 0.  Here the same reads go three ways -- to the oracle, to a stream as
ASCII, to a stream as packed input starting on nibble 0 and on nibble 1 -- at the (k, seed) pairs
test_other_kmer_sizes_and_seeds trusts the oracle for: the generic-k hashing loop behind wave_normalise_packed, the packed
carry in front of a segment, packed_code in the block sketcher, the 2048-slot retry and the offset rebasing of packed
batches.  The ASCII leg localises a failure: ASCII right and packed wrong means the packed code is at fault.  Every
comparison is exact integer equality.

The case builders (_short_case, _border_case, _segment_case, _dense_case, _prefilter_case, _species_case, _remap_invalid)
touch no device: they carry the oracle-side preconditions that say a case really exercises its edge."""
import functools

import numpy as np
import pytest

from helpers import pack_reads, workload, workload_species
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

PAIRS = [(16, 42), (21, 0), (11, 7), (32, 1), (15, 3), (17, 9), (8, 0)]
CHUNK = 2048          # raw bases a wave normalises at a time (kSketchCap)
SPLIT = 4 * CHUNK     # reads beyond this are cut into one segment per chunk in production mode (kLongSplit)
SEG_SLOTS = 64        # in-range hashes a segment may leave (kSegSlots)


# ---- plumbing ---------------------------------------------------------------------------------------------------------------
def _oracle(ref, k, seed, bases, offsets, top, sketches=False):
    n, s = ref["ref"].shape
    return orc.stream(k, seed, s, ref["ref"], np.full(n, s, np.uint32), bases, offsets, top_k=top, want_shared=True,
                      want_sketches=sketches)


def _stream(R, top, n_reads, data, off, packed):
    from sketchy_amd import api
    S = api.SumOfSharedHashes(R, top=top, max_batch_reads=max(1, n_reads), max_batch_bases=max(int(off[-1]), len(data)) + 2)
    S.set_packed_input(packed)
    return S


def _push(S, data, off, sketches=False, cuts=()):
    """one push, or one per piece when `cuts` (read indices) are given; the pieces' outputs one after the other + the table"""
    edges = [0, *cuts, len(off) - 1]
    parts = [S.push(data, off[a:b + 1], want_shared=True, want_sketches=sketches) for a, b in zip(edges[:-1], edges[1:])]
    got = {key: np.concatenate([p[key] for p in parts]) for key in ("topk_idx", "topk_sum", "shared")}
    if sketches:
        got.update({key: np.concatenate([p[key] for p in parts]) for key in ("sketches", "sketch_len")})
    got["cum"] = S.table()
    return got


def _same(got, exp, what, sketches=False):
    if sketches:
        np.testing.assert_array_equal(got["sketch_len"], exp["sketch_len"], err_msg=f"{what}: sketch_len")
        np.testing.assert_array_equal(got["sketches"], exp["sketches"], err_msg=f"{what}: sketches")
    np.testing.assert_array_equal(got["shared"], exp["shared"], err_msg=f"{what}: per-read shared")
    np.testing.assert_array_equal(got["topk_sum"], exp["topk_sum"], err_msg=f"{what}: topk_sum")
    np.testing.assert_array_equal(got["topk_idx"], exp["topk_idx"], err_msg=f"{what}: topk_idx")
    np.testing.assert_array_equal(got["cum"], exp["cum"], err_msg=f"{what}: table")


def _odd_cut(poff, lo=1):
    """the read nearest the middle of the batch that starts on an odd nibble: a batch cut there falls inside a byte"""
    n = len(poff) - 1
    odd = [r for r in range(lo, n) if int(poff[r]) & 1 and poff[r] > poff[0]]
    assert odd, "no read of the batch starts on an odd nibble"
    return min(odd, key=lambda r: abs(r - n // 2))


def _packings(bases, offsets):
    from sketchy_amd import api
    n_kept = sum(len(bytes(bases[int(a):int(b)]).translate(None, b" \t\r\n")) for a, b in zip(offsets[:-1], offsets[1:]))
    for first in (0, 1):
        packed, poff = api.pack_reads(bases, offsets, first_nibble=first)
        assert int(poff[0]) == first and int(poff[-1]) - first == n_kept
        yield first, packed, poff


def _with_n(read, positions):
    b = bytearray(read)
    for p in positions:
        b[p] = ord("N")
    return bytes(b)


def _border_positions(k, border=CHUNK):
    """raw positions of an N around the chunk border at `border` and the carry in front of it: the last code of a chunk, the
    first of the next, the oldest code carried over (border - (k - 1)), one before it (just outside the carry) -- and the
    later borders and the read's end.  (border - 1 - (k - 1) names border - k a second time.)"""
    ps = [border - 1, border, border - k, border - k + 1, border - 1 - (k - 1), border + CHUNK - 1, border + CHUNK,
          border + 2 * CHUNK - 1, border + 3 * CHUNK - 1]
    return list(dict.fromkeys(ps))


def _in_range_hashes(ref, read, k, seed):
    """hashes of the read's windows that the production sketchers keep (<= the reference's largest hash), in window order;
    the read holds bases only, so entry p belongs to the window starting at p"""
    h, _ = orc.kmer_hashes(read, k, seed)
    assert len(h) == max(0, len(read) - k + 1)
    return h <= ref["ref"].max()


def _anchored_start(ref, k, seed, border, length, lo=0):
    """Start of a read of `length` bases in the reference's genome whose window over the border at `border` counts: the
    window that begins with the OLDEST code carried over the border (read position border - (k - 1)) is a k-mer some
    reference sketch holds, no other window of the read has its hash, it survives the read's truncation to s, and its first
    base is an A (what code 4 looks like to a hash loop that was not told about it).  A production sketcher that loses the
    oldest carried code, or misses an N there, then reports another per-read count than the oracle -- with any other read the
    window is one of thousands whose hash no reference holds, and nothing would show."""
    g = ref["genome"]
    assert set(np.unique(g).tolist()) <= set(b"ACGT")
    h, _ = orc.kmer_hashes(g.tobytes(), k, seed)  # (bases only: entry p is the window starting at p)
    s = ref["ref"].shape[1]
    w = border - (k - 1)
    q = np.nonzero(np.isin(h, ref["ref"]) & (g[:len(h)] == ord("A")))[0]
    for a in (q - w)[(q - w >= lo) & (q - w + length <= len(g))]:
        hr = h[a:a + length - k + 1]
        if np.count_nonzero(hr == hr[w]) == 1 and np.count_nonzero(np.unique(hr) < hr[w]) < s:
            return int(a)
    raise AssertionError("no window of the genome qualifies")


# ---- a. short reads and the load shapes of wave_normalise_packed ----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _short_case(k, seed):
    ref, _, _ = workload(30, 300, 1, read_len=300, k=k, seed=seed, genome_len=120000, rng_seed=600 + k)
    g = ref["genome"].tobytes()
    rng = np.random.default_rng(17 + k)
    lengths = [0, 1, k - 1, k, k + 1, 2 * k - 1] + list(range(1, 41)) + list(range(252, 261)) + \
              [1023, 1025, 2047, 2048, 2049, CHUNK + k - 2, CHUNK + k - 1, CHUNK + k]
    reads = []
    for n in lengths:
        a = int(rng.integers(0, len(g) - n - 1))
        reads.append(g[a:a + n])
    reads += [g[1000:1400].lower(), g[4000:4300].replace(b"T", b"U"), b"RYKMSWBDHVN" * 20,
              g[2000:2200] + b"N" + g[2201:2500], g[7000:7300] + b"-" + g[7301:7600],
              g[9000:10100] + b"RYKMSWBDHVN" + g[10111:11200] + b"n" + g[11201:11301]]  # full sketch: the block sketcher's
    bases, offsets = pack_reads(reads)
    # reads start on both parities within one batch, whatever the first nibble is
    starts = np.cumsum([0] + [len(r) for r in reads])[:-1]
    long_enough = [s for s, r in zip(starts, reads) if len(r) >= k]
    assert {int(s) & 1 for s in long_enough} == {0, 1}
    exp = _oracle(ref, k, seed, bases, offsets, 2, sketches=True)
    assert exp["shared"].max() > 0
    return ref, reads, bases, offsets, exp


@pytest.mark.parametrize("k,seed", PAIRS)
def test_short_reads_every_load_shape(gpu, k, seed):
    """Reads of 0 .. 40 bases, around the 256-base groups and the 2048-base chunk (2048 + k - 1 is the longest full sketch a
    wave takes; one more goes to the block sketcher), lower case, U, IUPAC codes: full sketches in one push, then the
    production path in two pushes whose cut falls inside a byte."""
    from sketchy_amd import api
    ref, reads, bases, offsets, exp = _short_case(k, seed)
    n = len(reads)
    R = api.ReferenceSketch(ref["ref"], k=k, seed=seed)
    A = _stream(R, 2, n, bases, offsets, False)
    _same(_push(A, bases, offsets, sketches=True), exp, "ASCII, debug path", sketches=True)
    A.reset()
    _same(_push(A, bases, offsets, cuts=(n // 2,)), exp, "ASCII, production path")
    for first, packed, poff in _packings(bases, offsets):
        S = _stream(R, 2, n, packed, poff, True)
        _same(_push(S, packed, poff, sketches=True), exp, f"packed from nibble {first}, debug path", sketches=True)
        S.reset()
        h = _odd_cut(poff)
        _same(_push(S, packed, poff, cuts=(h,)), exp, f"packed from nibble {first}, production path cut at read {h}")
        S.close()
    A.close(); R.close()


# ---- b. N at the chunk and carry borders, one read on one wave ------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _border_case(k, seed):
    ref, _, _ = workload(30, 600, 1, read_len=300, k=k, seed=seed, genome_len=120000, rng_seed=640 + k)
    g = ref["genome"].tobytes()
    a = _anchored_start(ref, k, seed, CHUNK, SPLIT, lo=3001)
    clean = g[a:a + SPLIT]
    positions = _border_positions(k)
    reads = [clean] + [_with_n(clean, [p]) for p in positions]
    bases, offsets = pack_reads(reads)
    exp = _oracle(ref, k, seed, bases, offsets, 2, sketches=True)
    oldest = 1 + positions.index(CHUNK - k + 1)
    assert exp["shared"][oldest].sum() < exp["shared"][0].sum()  # an N on the oldest carried code takes a counted window away
    differ = [r for r in range(1, len(reads)) if not np.array_equal(exp["shared"][r], exp["shared"][0])
              or exp["sketch_len"][r] != exp["sketch_len"][0] or not np.array_equal(exp["sketches"][r], exp["sketches"][0])]
    assert len(differ) >= 2, f"an N changes the oracle's output for reads {differ} only: the case tests nothing"
    return ref, reads, bases, offsets, exp


@pytest.mark.parametrize("k,seed", PAIRS)
def test_n_at_chunk_and_carry_borders_on_one_wave(gpu, k, seed):
    """An 8192-base read stays on one wave in production mode (four chunks, k - 1 codes carried from each to the next); an N
    that is the last code of a chunk, the first of the next, the oldest carried code or the one in front of it must break
    exactly the windows it breaks in the serial loop.  Production path and full sketches (the block sketcher)."""
    from sketchy_amd import api
    ref, reads, bases, offsets, exp = _border_case(k, seed)
    n = len(reads)
    R = api.ReferenceSketch(ref["ref"], k=k, seed=seed)
    A = _stream(R, 2, n, bases, offsets, False)
    _same(_push(A, bases, offsets), exp, "ASCII, production path")
    A.close()
    for first, packed, poff in _packings(bases, offsets):
        S = _stream(R, 2, n, packed, poff, True)
        _same(_push(S, packed, poff), exp, f"packed from nibble {first}, production path")
        st = S.stats()
        assert st["reads_split_over_waves"] == 0 and st["reads_block_sketcher"] == 0, st
        S.reset()
        _same(_push(S, packed, poff, sketches=True), exp, f"packed from nibble {first}, debug path", sketches=True)
        S.close()
    R.close()


# ---- c. segments: reads split over waves ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _segment_case(k, seed):
    ref, _, _ = workload(40, 300, 1, read_len=300, k=k, seed=seed, genome_len=400000, rng_seed=680 + k)
    g = ref["genome"].tobytes()
    a = _anchored_start(ref, k, seed, 3 * CHUNK, 20000, lo=100001)
    r20 = g[a:a + 20000]  # (the window that begins with the oldest code carried into its fourth segment counts)
    clean = [g[0:SPLIT], g[101:101 + SPLIT + 1], g[9000:9000 + SPLIT + k - 2], g[20000:20000 + SPLIT + k - 1],
             g[30001:30001 + SPLIT + k], g[40000:40000 + 10240], r20, g[200000:200000 + 60001]]
    reads = clean + [_with_n(r20, [p]) for p in _border_positions(k, 3 * CHUNK)]
    reads.append(_with_n(r20, range(3 * CHUNK - k // 2, 3 * CHUNK - k // 2 + k)))  # a run of k Ns across a border
    bases, offsets = pack_reads(reads)
    exp = _oracle(ref, k, seed, bases, offsets, 2)
    assert exp["shared"][7].max() > 5  # the 60 kb read really shares hashes
    oldest = len(clean) + _border_positions(k, 3 * CHUNK).index(3 * CHUNK - k + 1)
    assert exp["shared"][oldest].sum() < exp["shared"][6].sum()  # an N on the oldest carried code takes a counted window away
    # no segment of a clean read leaves more hashes than its slot takes (an N only removes windows): every long read is
    # merged from its segments, none falls through to the block sketcher
    for r in clean:
        inr = _in_range_hashes(ref, r, k, seed)
        ends = np.arange(len(inr)) + k - 1
        assert np.bincount(ends[inr] // CHUNK, minlength=1).max() < SEG_SLOTS
    return ref, reads, bases, offsets, exp


def _check_segment_stats(S, reads):
    st = S.stats()
    assert st["reads_split_over_waves"] == sum(1 for r in reads if len(r) > SPLIT), st
    assert st["read_segments"] == sum((len(r) + CHUNK - 1) // CHUNK for r in reads if len(r) > SPLIT), st
    assert st["reads_block_sketcher"] == 0, st


@pytest.mark.parametrize("k,seed", PAIRS)
def test_reads_split_over_waves(gpu, k, seed):
    """Reads at and beyond the 8192-base split, one wave per 2048-base segment: a segment takes the k - 1 nibbles in front of
    its chunk as its carry.  Last segments of 1, k - 2, k - 1 and k bases, an N on either side of a border and at both ends
    of the carry, a run of k Ns across a border.  Production path; then full sketches (the block sketcher), same counts."""
    from sketchy_amd import api
    ref, reads, bases, offsets, exp = _segment_case(k, seed)
    n = len(reads)
    R = api.ReferenceSketch(ref["ref"], k=k, seed=seed)
    A = _stream(R, 2, n, bases, offsets, False)
    _same(_push(A, bases, offsets), exp, "ASCII, production path")
    _check_segment_stats(A, reads)
    A.close()
    for first, packed, poff in _packings(bases, offsets):
        S = _stream(R, 2, n, packed, poff, True)
        _same(_push(S, packed, poff), exp, f"packed from nibble {first}, production path")
        _check_segment_stats(S, reads)
        S.reset()
        full = S.push(packed, poff, want_shared=True, want_sketches=True)
        np.testing.assert_array_equal(full["shared"], exp["shared"], err_msg=f"packed from nibble {first}, debug path")
        S.close()
    R.close()


# ---- d. the tiers behind the fast variant, on a dense reference -----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _dense_case(k, seed):
    ref, _, _ = workload(12, 6000, 1, read_len=300, genome_len=40000, k=k, seed=seed, rng_seed=720 + k)
    g = ref["genome"].tobytes()
    reads = [g[101:401], g[100:1600], g[5001:8001], g[9000:13000], g[0:20000], g[15000:39000]]
    bases, offsets = pack_reads(reads)
    exp = _oracle(ref, k, seed, bases, offsets, 1, sketches=True)
    kept = int(_in_range_hashes(ref, reads[2], k, seed).sum())
    assert 256 < kept < 2048, kept  # the 3 kb read: more than the fast variant's slots, within the retry's
    # a segment of each long read overflows its slot: they fall through to the block sketcher
    for r in reads[4:]:
        inr = _in_range_hashes(ref, r, k, seed)
        ends = np.arange(len(inr)) + k - 1
        assert np.bincount(ends[inr] // CHUNK).max() > SEG_SLOTS
    return ref, reads, bases, offsets, exp


@pytest.mark.parametrize("k,seed", [(16, 42), (21, 0), (32, 1), (8, 0)])
def test_dense_reference_retry_and_block_sketcher(gpu, k, seed):
    """About 15 % of the hash space is in range: the 3 and 4 kb reads overflow the fast variant's 256 hash slots (2048-slot
    retry), the 20 and 24 kb reads overflow their segments' 64-entry slots (block sketcher)."""
    from sketchy_amd import api
    ref, reads, bases, offsets, exp = _dense_case(k, seed)
    n = len(reads)
    R = api.ReferenceSketch(ref["ref"], k=k, seed=seed)
    A = _stream(R, 1, n, bases, offsets, False)
    _same(_push(A, bases, offsets), exp, "ASCII, production path")
    A.close()
    for first, packed, poff in _packings(bases, offsets):
        S = _stream(R, 1, n, packed, poff, True)
        _same(_push(S, packed, poff), exp, f"packed from nibble {first}, production path")
        st = S.stats()
        assert st["reads_block_sketcher"] >= 2 and st["reads_split_over_waves"] >= 2, st
        S.reset()
        _same(_push(S, packed, poff, sketches=True), exp, f"packed from nibble {first}, debug path", sketches=True)
        S.close()
    R.close()


# ---- e. every nibble value above 3 is N ---------------------------------------------------------------------------------------
def _remap_invalid(packed, rng):
    """the buffer with every nibble equal to 4 replaced by a value of 5 .. 15, each of the eleven used at least once"""
    nib = np.empty(2 * len(packed), np.uint8)
    nib[0::2], nib[1::2] = packed & 15, packed >> 4
    assert nib.max() <= 4  # the project's packers write 0 .. 4 only
    at = np.nonzero(nib == 4)[0]
    assert len(at) >= 11
    vals = np.concatenate([np.arange(5, 16), rng.integers(5, 16, len(at) - 11)]).astype(np.uint8)
    nib[at] = rng.permutation(vals)
    assert set(nib[at].tolist()) == set(range(5, 16)) and not (nib == 4).any()
    return (nib[0::2] | (nib[1::2] << 4)).astype(np.uint8)


@pytest.mark.parametrize("case", ["short", "segments"])
@pytest.mark.parametrize("k,seed", [(16, 42), (21, 0)])
def test_every_nibble_above_three_is_n(gpu, k, seed, case):
    """include/sketchy_hip.h: "codes 0..3 = A C G T(U), any other value = a retained non-ACGT byte".  The packers write 4;
    5 .. 15 in its place must change nothing, in the wave sketchers (a bit test on whole words), in the carry of a segment
    and in the block sketcher (a compare per nibble)."""
    from sketchy_amd import api
    ref, reads, bases, offsets, exp = (_short_case if case == "short" else _segment_case)(k, seed)
    n = len(reads)
    R = api.ReferenceSketch(ref["ref"], k=k, seed=seed)
    rng = np.random.default_rng(99)
    for first, packed, poff in _packings(bases, offsets):
        other = _remap_invalid(packed, rng)
        S = _stream(R, 2, n, packed, poff, True)
        cuts = (_odd_cut(poff),) if case == "short" else ()
        plain = _push(S, packed, poff, cuts=cuts)
        S.reset()
        got = _push(S, other, poff, cuts=cuts)
        _same(got, plain, f"nibbles 5..15 against nibble 4, from nibble {first}, production path")
        _same(got, exp, f"nibbles 5..15 against the oracle, from nibble {first}, production path")
        S.reset()
        plain = _push(S, packed, poff, sketches=True)
        S.reset()
        got = _push(S, other, poff, sketches=True)
        _same(got, plain, f"nibbles 5..15 against nibble 4, from nibble {first}, debug path", sketches=True)
        np.testing.assert_array_equal(got["shared"], exp["shared"])
        S.close()
    R.close()


# ---- f. the k-mer prefilter with packed input ---------------------------------------------------------------------------------
def _wrap(seq: bytes, width=60) -> bytes:
    return b"\n".join(seq[i:i + width] for i in range(0, len(seq), width)) + b"\n"


@functools.lru_cache(maxsize=None)
def _prefilter_case(seed):
    s = 2000  # the prefilter takes reads of at most s + 15 = 2015 bases
    ref, _, _ = workload(60, s, 1, read_len=300, seed=seed, genome_len=300000, rng_seed=7300 + seed)
    g = ref["genome"].tobytes()
    rng = np.random.default_rng(12)
    reads = [g[a:a + n] for a, n in ((int(rng.integers(0, 280000)), int(n)) for n in
                                     [15, 16, 17, 64, 300, 1500, 1500, 2014, 2015, 2016, 2047, 2048, 2049, 2063, 2064, 4000, 8192,
                                      8193, 9000, 12000])]
    reads += [g[1000:2500].lower(), g[3000:3700] + b"N" + g[3701:4500], _wrap(g[5000:13000]), g[20000:21500].replace(b"T", b"U"),
              b"ACGT" * 500, b"", g[50000:50040] + b"\n\n" + g[50040:50300]]
    bases, offsets = pack_reads(reads)
    exp = _oracle(ref, 16, seed, bases, offsets, 2)
    assert exp["shared"].max() > 3
    kept = [len(r.translate(None, b" \t\r\n")) for r in reads]
    assert {s + 14, s + 15, s + 16} <= set(kept) and any(SPLIT < n for n in kept)
    assert sum(1 for n in kept if 16 <= n <= s + 15) >= 10  # reads the prefilter takes
    return ref, reads, bases, offsets, exp


@pytest.mark.parametrize("seed", [0, 42])
def test_kmer_prefilter_with_packed_input(gpu, seed):
    """The prefilter (k = 16, production mode, reads of at most s + 15 bases) has its own window loop behind the normalised
    codes: packed input at both parities around the s + 15 boundary, with reads beyond the split beside it."""
    from sketchy_amd import api
    ref, reads, bases, offsets, exp = _prefilter_case(seed)
    n = len(reads)
    try:
        api.set_option("kmer_prefilter", 1)
        R = api.ReferenceSketch(ref["ref"], seed=seed)
        assert R.kmer_filter[0] > 0
        A = _stream(R, 2, n, bases, offsets, False)
        _same(_push(A, bases, offsets), exp, "ASCII, prefilter on")
        A.close()
        for first, packed, poff in _packings(bases, offsets):
            S = _stream(R, 2, n, packed, poff, True)
            _same(_push(S, packed, poff), exp, f"packed from nibble {first}, prefilter on")
            assert S.stats()["reads_split_over_waves"] == sum(1 for r in reads if len(r.translate(None, b" \t\r\n")) > SPLIT)
            S.reset()
            _same(_push(S, packed, poff, cuts=(_odd_cut(poff),)), exp, f"packed from nibble {first}, prefilter on, two pushes")
            S.close()
        R.close()
    finally:
        api.set_option("kmer_prefilter", 0)


# ---- g. device-resident and host-fed entry points at generic k ----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _species_case():
    k, seed, top = 21, 5, 3
    refs, bases, offsets = workload_species([40, 25, 33], 300, 300, read_len=600, k=k, seed=seed, genome_len=60000, rng_seed=760)
    exp = [orc.stream(k, seed, 300, r["ref"], r["col_len"], bases, offsets, top_k=top, want_shared=True) for r in refs]
    assert all(e["shared"].max() > 0 for e in exp)
    return k, seed, top, refs, bases, offsets, exp


def test_device_resident_and_host_fed_generic_k(gpu):
    """k = 21, seed 5, three species, top 3: packed batches through enqueue_device (offsets into one resident buffer) and
    through submit / drain (offsets rebased to the batch's first byte), every batch cut on an odd nibble."""
    from sketchy_amd import api
    k, seed, top, refs, bases, offsets, exp = _species_case()
    n, ns = len(offsets) - 1, len(refs)
    want_idx = np.stack([e["topk_idx"] for e in exp], axis=1)
    want_sum = np.stack([e["topk_sum"] for e in exp], axis=1)
    want_cum = np.concatenate([e["cum"] for e in exp])
    packed, poff = api.pack_reads(bases, offsets, first_nibble=1)
    R = api.ReferenceSketch([r["ref"] for r in refs], [r["col_len"] for r in refs], k=k, seed=seed)
    A = api.SumOfSharedHashes(R, top=top, max_batch_reads=n, max_batch_bases=len(bases))
    ga = A.push(bases, offsets, want_shared=True)
    np.testing.assert_array_equal(ga["topk_sum"], want_sum, err_msg="ASCII")
    np.testing.assert_array_equal(ga["topk_idx"], want_idx, err_msg="ASCII")
    np.testing.assert_array_equal(ga["shared"], np.concatenate([e["shared"] for e in exp], axis=1), err_msg="ASCII")
    A.close()
    odd = [r for r in range(1, n) if int(poff[r]) & 1]
    c1, c2 = min(odd, key=lambda r: abs(r - n // 3)), min(odd, key=lambda r: abs(r - 7 * n // 9))
    assert 0 < c1 and c1 + 1 < c2 < n
    batches = ((0, c1), (c1, c1 + 1), (c1 + 1, c2), (c2, n))  # (the one-read batch ends on either parity)
    assert all(int(poff[a]) & 1 for a in (0, c1, c2))
    S = api.SumOfSharedHashes(R, top=top, max_batch_reads=n, max_batch_bases=int(poff[-1]) + 2)
    S.set_packed_input(True)
    d_b = api.DeviceBuffer.from_numpy(packed)
    keep, rows = [d_b], []
    for a, b in batches:
        d_o = api.DeviceBuffer.from_numpy(np.ascontiguousarray(poff[a:b + 1]))
        d_i, d_s = api.DeviceBuffer((b - a) * ns * top * 4), api.DeviceBuffer((b - a) * ns * top * 8)
        keep += [d_o, d_i, d_s]
        rows.append((b - a, d_i, d_s))
        S.enqueue_device(d_b.ptr, d_o.ptr, b - a, int(poff[b] - poff[a]), d_i.ptr, d_s.ptr)
    S.sync()
    np.testing.assert_array_equal(np.concatenate([d.to_numpy(np.uint32, (m, ns, top)) for m, d, _ in rows]), want_idx)
    np.testing.assert_array_equal(np.concatenate([d.to_numpy(np.uint64, (m, ns, top)) for m, _, d in rows]), want_sum)
    np.testing.assert_array_equal(S.table(), want_cum)
    for d in keep:
        d.free()
    # host-fed: page-locked packed batches through submit / drain
    S.reset()
    hb = api.HostBuffer(len(packed))
    hb.view(np.uint8)[:] = packed
    outs = []
    for a, b in batches:
        ho = api.HostBuffer((b - a + 1) * 8)
        ho.view(np.uint64)[:] = poff[a:b + 1]
        hi, hs = api.HostBuffer((b - a) * ns * top * 4), api.HostBuffer((b - a) * ns * top * 8)
        S.submit(hb.ptr, ho.ptr, b - a, hi.ptr, hs.ptr)
        outs.append((b - a, ho, hi, hs))
    S.drain()
    np.testing.assert_array_equal(np.concatenate([hi.view(np.uint32)[:m * ns * top] for m, _, hi, _ in outs]).reshape(n, ns, top), want_idx)
    np.testing.assert_array_equal(np.concatenate([hs.view(np.uint64)[:m * ns * top] for m, _, _, hs in outs]).reshape(n, ns, top), want_sum)
    np.testing.assert_array_equal(S.table(), want_cum)
    for _, ho, hi, hs in outs:
        ho.free(); hi.free(); hs.free()
    hb.free()
    S.close(); R.close()
