"""Thin Python handles over the C ABI (numpy in, numpy out; no torch, no CPU fallback).

Names follow the reference's own vocabulary for this path:
  ReferenceSketch              the `Vec<Sketch>` returned by Sketchy::_read_sketch (src/sketchy.rs:497-536)
  SumOfSharedHashes            the state and loop body of Sketchy::_sum_of_shared_hashes (src/sketchy.rs:317-356)
  common_hashes / sketch_reads Sketchy::_common_hashes (:419-459) and finch's process/to_vec (:331-335)
"""
import ctypes as C

import numpy as np

from . import _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def pack_reads(bases, offsets, first_nibble=0):
    """ASCII reads (bases, offsets as for push()) -> (packed uint8 array, uint64 offsets in bases): two bases per byte, low
    nibble first, whitespace dropped, everything not ACGTU -> 4 (skx_pack_bases).  first_nibble: start the stream at that
    nibble (tests: reads on odd nibbles)."""
    L = _lib.load()
    bases = np.ascontiguousarray(bases, np.uint8)
    offsets = np.ascontiguousarray(offsets, np.uint64)
    n = len(offsets) - 1
    packed = np.zeros((first_nibble + len(bases) + 1) // 2 + 1, np.uint8)
    out = np.zeros(n + 1, np.uint64)
    pos = int(first_nibble)
    out[0] = pos
    for r in range(n):
        a, b = int(offsets[r]), int(offsets[r + 1])
        if b > a:
            pos = int(L.skx_pack_bases(bases[a:b].ctypes.data_as(C.c_void_p), b - a, _p(packed), pos))
        out[r + 1] = pos
    return packed[: (pos + 1) // 2 + 1], out


def set_option(name: str, value: int):
    """Process-wide policy for references / streams created from now on (skx_set_option), e.g. "kmer_prefilter"."""
    _lib.check(_lib.load().skx_set_option(name.encode(), int(value)))


def get_option(name: str) -> int:
    v = C.c_uint64(0)
    _lib.check(_lib.load().skx_get_option(name.encode(), C.byref(v)))
    return v.value


def device_count() -> int:
    return _lib.load().skx_device_count()


def device_info(device=0):
    L = _lib.load()
    name = C.create_string_buffer(256)
    cu, mem = C.c_int(0), C.c_uint64(0)
    _lib.check(L.skx_device_info(device, name, 256, C.byref(cu), C.byref(mem)))
    return dict(name=name.value.decode(), compute_units=cu.value, total_mem=mem.value)


def device_mem(device=0):
    """(free, total) bytes of device memory"""
    f, t = C.c_uint64(0), C.c_uint64(0)
    _lib.check(_lib.load().skx_dev_mem_info(device, C.byref(f), C.byref(t)))
    return f.value, t.value


def encode_genotypes(columns):
    """Genotype table as integer codes for ReferenceSketch.set_genotypes: columns = one row of strings (or bytes) per genome, all
    of the same length F.  Returns (codes uint32 [n_genomes, F], values): values[f] lists column f's distinct strings in byte-wise
    sorted order and the code of a string is its rank there -- so "ties go to the smallest code" is "ties go to the
    lexicographically smallest string", and values[f][code] turns a consensus code back into its string."""
    rows = [list(r) for r in columns]
    n_feat = len(rows[0]) if rows else 0
    if any(len(r) != n_feat for r in rows):
        raise ValueError("every genome needs the same number of genotype columns")
    key = lambda v: v if isinstance(v, bytes) else str(v).encode()
    codes = np.zeros((len(rows), n_feat), np.uint32)
    values = []
    for f in range(n_feat):
        col = [r[f] for r in rows]
        distinct = sorted(set(col), key=key)
        rank = {v: i for i, v in enumerate(distinct)}
        codes[:, f] = [rank[v] for v in col]
        values.append(distinct)
    return codes, values


class ReferenceSketch:
    """Reference sketch collection(s) resident in HBM.  hashes: [n_genomes, s] uint64, row g = genome g's ascending
    distinct hashes, first col_len[g] valid -- or a LIST of such matrices, one per species (same s, k, seed): they are
    scanned together in one pass per batch, every species keeps its own table and ranking (one `sketchy predict` run
    per species over the same reads, src/sketchy.rs:81-82).  s: the size reads are sketched with; default = the matrix
    width.  The reference uses the length of the collection's FIRST sketch (src/sketchy.rs:82, :520-527) -- pass
    s=col_len[0] to mirror a collection whose sketches differ in length."""

    def __init__(self, hashes, col_len=None, k=16, seed=0, device=0, s=None):
        L = _lib.load()
        many = isinstance(hashes, (list, tuple))
        mats = [np.ascontiguousarray(h, np.uint64) for h in (hashes if many else [hashes])]
        if any(m.ndim != 2 for m in mats) or len({m.shape[1] for m in mats}) != 1:
            raise ValueError("hashes must be [n_genomes, s] (one matrix per species, all with the same s)")
        lens = col_len if many else [col_len]
        lens = [None] * len(mats) if lens is None else list(lens)
        lens = [np.full(m.shape[0], m.shape[1], np.uint32) if c is None else np.ascontiguousarray(c, np.uint32)
                for m, c in zip(mats, lens)]
        self.species = [int(m.shape[0]) for m in mats]
        self.n_species = len(mats)
        self.n_genomes, self.stride = sum(self.species), int(mats[0].shape[1])
        self.s = self.stride if s is None else int(s)
        self.k, self.seed, self.device = int(k), int(seed), int(device)
        h = C.c_void_p()
        if self.n_species == 1:
            _lib.check(L.skx_ref_create(C.byref(h), device, self.k, self.seed, self.s, self.stride, self.n_genomes, _p(mats[0]), _p(lens[0])))
        else:
            ng = (C.c_uint32 * self.n_species)(*self.species)
            hp = (C.c_void_p * self.n_species)(*[m.ctypes.data for m in mats])
            cp = (C.c_void_p * self.n_species)(*[c.ctypes.data for c in lens])
            _lib.check(L.skx_ref_create_multi(C.byref(h), device, self.k, self.seed, self.s, self.stride, self.n_species, ng, hp, cp))
        self._h = h

    @property
    def kmer_filter(self):
        """(keys, table bytes) of the reference's k-mer prefilter; (0, 0) when none was built"""
        n, b = C.c_uint64(0), C.c_uint64(0)
        _lib.check(_lib.load().skx_ref_kmer_filter(self._h, C.byref(n), C.byref(b)))
        return n.value, b.value

    @property
    def rare_index(self):
        """dict(keys, rare_keys, postings, bytes) of the reference's rare-hash index (all 0: none was built)"""
        v = [C.c_uint64(0) for _ in range(4)]
        _lib.check(_lib.load().skx_ref_rare_index(self._h, *[C.byref(x) for x in v]))
        return dict(zip(("keys", "rare_keys", "postings", "bytes"), [x.value for x in v]))

    @property
    def patterns(self):
        """dict(long_lists, patterns, pattern_lists, bytes): the long genome lists of the rare-hash index and how many of them are stored
        as a shared pattern + exceptions (all 0: none)"""
        v = [C.c_uint64(0) for _ in range(4)]
        _lib.check(_lib.load().skx_ref_patterns(self._h, *[C.byref(x) for x in v]))
        return dict(zip(("long_lists", "patterns", "pattern_lists", "bytes"), [x.value for x in v]))

    @property
    def static_dense(self):
        """(is_static, n_hashes): does the reference have a static dense dictionary, and how many hashes the scan can be asked for"""
        f, n = C.c_int(0), C.c_uint64(0)
        _lib.check(_lib.load().skx_ref_static_dense(self._h, C.byref(f), C.byref(n)))
        return bool(f.value), n.value

    @property
    def pass_bytes(self) -> int:
        b = C.c_uint64(0)
        _lib.check(_lib.load().skx_ref_pass_bytes(self._h, C.byref(b)))
        return b.value

    def common_hashes(self, query, query_len=None) -> np.ndarray:
        """[n_query, n_genomes] uint32 intersection sizes (Sketchy::_common_hashes for every pair)."""
        query = np.ascontiguousarray(query, np.uint64)
        nq, stride = query.shape
        query_len = np.full(nq, stride, np.uint32) if query_len is None else np.ascontiguousarray(query_len, np.uint32)
        out = np.zeros((nq, self.n_genomes), np.uint32)
        _lib.check(_lib.load().skx_common_hashes(self._h, _p(query), _p(query_len), nq, stride, _p(out)))
        return out

    def rank_sketches(self, query, query_len=None, top=1, want_common=False):
        """Sketchy::_shared_hashes' tail for many query sketches in one call: per query and species the first `top` genomes of
        (shared desc, index asc), counted and selected on the device.  query: [n_query, stride] uint64 ascending rows.
        Returns (idx, shared[, common]): [n_query, n_species, top] uint32 each (indices local to the species)
        [, [n_query, n_genomes] uint32: the counts the rows were taken from]."""
        query = np.ascontiguousarray(query, np.uint64)
        if query.ndim != 2:
            raise ValueError("query must be [n_query, stride]")
        nq, stride = query.shape
        query_len = np.full(nq, stride, np.uint32) if query_len is None else np.ascontiguousarray(query_len, np.uint32)
        if query_len.shape != (nq,):
            raise ValueError("query_len must hold one length per query row")
        top = int(top)
        idx = np.zeros((nq, self.n_species, max(top, 0)), np.uint32)
        shared = np.zeros_like(idx)
        common = np.zeros((nq, self.n_genomes), np.uint32) if want_common else None
        if stride == 0:  # rows without a slot: nq empty queries (the library copies rows of at least one slot)
            if query_len.any():
                raise ValueError("query_len exceeds the stride of the query rows")
            query, stride = np.zeros((max(nq, 1), 1), np.uint64), 1
        _lib.check(_lib.load().skx_rank_sketches(self._h, _p(query), _p(query_len), nq, stride, top, _p(idx), _p(shared),
                                                 _p(common) if want_common else None))
        return (idx, shared, common) if want_common else (idx, shared)

    def predict_groups(self, bases, offsets, group_first, top=1, want_sketches=False, want_valid_kmers=False):
        """Offline `predict` for many samples in one call: records -> one pooled sketch per group (as sketch_groups, with this
        reference's k, seed and s) -> the first `top` rows per group and species.  Returns (idx, shared) [n_groups, n_species, top]
        uint32, then -- want_sketches -- the pooled sketches and their lengths, then -- want_valid_kmers -- the groups' valid
        k-mer windows."""
        bases = np.ascontiguousarray(bases, np.uint8)
        offsets = np.ascontiguousarray(offsets, np.uint64)
        group_first = np.ascontiguousarray(group_first, np.uint32)
        if offsets.ndim != 1 or len(offsets) < 1 or group_first.ndim != 1 or len(group_first) < 1:
            raise ValueError("offsets and group_first are 1-D with at least one entry")
        n, ng = len(offsets) - 1, len(group_first) - 1
        top = int(top)
        idx = np.zeros((ng, self.n_species, max(top, 0)), np.uint32)
        shared = np.zeros_like(idx)
        sk = np.zeros((ng, self.s), np.uint64) if want_sketches else None
        sl = np.zeros(ng, np.uint32) if want_sketches else None
        vk = np.zeros(ng, np.uint64) if want_valid_kmers else None
        b = bases if len(bases) else np.zeros(1, np.uint8)
        _lib.check(_lib.load().skx_predict_groups(self._h, _p(b), _p(offsets), n, _p(group_first), ng, top, _p(idx), _p(shared),
                                                  _p(sk) if want_sketches else None, _p(sl) if want_sketches else None,
                                                  _p(vk) if want_valid_kmers else None))
        out = (idx, shared)
        if want_sketches:
            out += (sk, sl)
        if want_valid_kmers:
            out += (vk,)
        return out

    def set_genotypes(self, codes):
        """Make a genotype table part of the resident reference: codes [n_genomes, F] uint32 (species one after the other), equal
        codes in a column = equal genotype (encode_genotypes).  Once per reference."""
        codes = np.ascontiguousarray(codes, np.uint32)
        if codes.ndim != 2 or codes.shape[0] != self.n_genomes:
            raise ValueError("codes must be [n_genomes, n_features]")
        _lib.check(_lib.load().skx_ref_set_genotypes(self._h, codes.shape[1], _p(codes)))

    @property
    def n_features(self) -> int:
        """columns of the reference's genotype table (0: none was set)"""
        n = C.c_uint32(0)
        _lib.check(_lib.load().skx_ref_n_features(self._h, C.byref(n)))
        return n.value

    def consensus_rows(self, idx) -> np.ndarray:
        """Consensus code per genotype column of ranked rows: idx [..., top] (one species) or [..., n_species, top] genome indices
        local to the species, as every ranking entry point returns them -> [..., F] / [..., n_species, F] uint32: the code most of
        a row's genomes carry, ties to the smallest code."""
        idx = np.ascontiguousarray(idx, np.uint32)
        tail = 1 if self.n_species == 1 else 2
        if idx.ndim < tail or (tail == 2 and idx.shape[-2] != self.n_species):
            raise ValueError("idx must be [..., top] for one species and [..., n_species, top] for several")
        top = idx.shape[-1]
        lead = idx.shape[: idx.ndim - tail]
        n_rows = int(np.prod(lead, dtype=np.int64))
        out = np.zeros(lead + idx.shape[idx.ndim - tail:-1] + (self.n_features,), np.uint32)
        _lib.check(_lib.load().skx_consensus_rows(self._h, _p(idx), n_rows, top, _p(out)))
        return out

    def neighbours(self, first=0, count=None, top=1, species=0, want_codes=False):
        """Leave-one-out neighbours: for every genome of [first, first + count) of `species` (count None: to the species' end) the
        first `top` OTHER genomes of that species in (shared hashes desc, index asc) order, rebuilt, counted and selected on the
        device from the resident reference.  Returns (idx, shared[, codes]): [count, top] uint32 each (indices local to the species)
        [, [count, n_features] uint32: the consensus of each row's neighbours, ties to the smallest code]."""
        species, first, top = int(species), int(first), int(top)
        if not 0 <= species < self.n_species:
            raise ValueError(f"species {species} outside 0..{self.n_species - 1}")
        n = self.species[species]
        count = n - first if count is None else int(count)
        if first < 0 or count < 0 or first + count > n:
            raise ValueError(f"first={first} + count={count} exceeds the species' {n} genomes")
        if not 1 <= top <= min(n - 1, _lib.MAX_TOP):
            raise ValueError(f"top={top} outside 1..min(genomes of the species - 1, {_lib.MAX_TOP}) = {min(n - 1, _lib.MAX_TOP)}")
        idx = np.zeros((count, top), np.uint32)
        shared = np.zeros_like(idx)
        codes = None
        if want_codes:
            nf = self.n_features
            if nf == 0:
                raise ValueError("want_codes needs a genotype table (set_genotypes)")
            codes = np.zeros((count, nf), np.uint32)
        _lib.check(_lib.load().skx_ref_neighbours(self._h, species, first, count, top, _p(idx), _p(shared), _p(codes) if want_codes else None))
        return (idx, shared, codes) if want_codes else (idx, shared)

    def close(self):
        if getattr(self, "_h", None):
            _lib.load().skx_ref_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class SumOfSharedHashes:
    """Streaming predictor: running sum-of-shared-hashes table + per-read top rows."""

    def __init__(self, ref: ReferenceSketch, top=1, max_batch_reads=4096, max_batch_bases=None):
        L = _lib.load()
        self.ref, self.top = ref, int(top)
        self.max_batch_reads = int(max_batch_reads)
        self.max_batch_bases = int(max_batch_bases if max_batch_bases is not None else max_batch_reads * 2063)
        h = C.c_void_p()
        _lib.check(L.skx_stream_create(C.byref(h), ref._h, self.top, self.max_batch_reads, self.max_batch_bases))
        self._h = h

    def bind_consensus(self, codes_out):
        """Bind a consensus output (pointer / address; [n_reads, n_species, F] uint32) for the NEXT batch call, which consumes it."""
        _lib.check(_lib.load().skx_stream_bind_consensus(self._h, codes_out))

    def bind_changes(self, cap, n_events, ev_read, ev_idx=None, ev_sum=None, ev_codes=None):
        """Bind an event list (pointers / addresses; skx_stream_bind_changes) for the NEXT batch call, which consumes it: n_events [1],
        ev_read [cap], ev_idx / ev_sum [cap, n_species, top], ev_codes [cap, n_species, F] (not None: codes mode)."""
        _lib.check(_lib.load().skx_stream_bind_changes(self._h, cap, n_events, ev_read, ev_idx, ev_sum, ev_codes))

    def bind_call(self, call_species, call_idx=None, call_sum=None, call_codes=None):
        """Bind a species call (pointers / addresses; skx_stream_bind_call) for the NEXT batch call, which consumes it:
        call_species [n_reads], call_idx / call_sum [n_reads, top], call_codes [n_reads, F]."""
        _lib.check(_lib.load().skx_stream_bind_call(self._h, call_species, call_idx, call_sum, call_codes))

    def bind_call_changes(self, cap, n_events, ev_read, ev_species, ev_idx=None, ev_sum=None, ev_codes=None):
        """Bind the call's event list (pointers / addresses; skx_stream_bind_call_changes) for the NEXT batch call, which consumes it:
        n_events [1], ev_read / ev_species [cap], ev_idx / ev_sum [cap, top], ev_codes [cap, F] (not None: codes mode)."""
        _lib.check(_lib.load().skx_stream_bind_call_changes(self._h, cap, n_events, ev_read, ev_species, ev_idx, ev_sum, ev_codes))

    def _bind(self, consensus, changes, call=None, call_changes=None):
        if consensus is not None:
            self.bind_consensus(consensus)
        if changes is not None:
            self.bind_changes(*changes)
        if call is not None:
            self.bind_call(*call)
        if call_changes is not None:
            self.bind_call_changes(*call_changes)

    def push(self, bases, offsets, want_shared=False, want_sketches=False, want_consensus=False, want_changes=None, changes_codes=False,
             want_call=False, want_call_changes=0, call_changes_codes=False):
        """Consume a packed batch; returns dict(topk_idx, topk_sum[, shared, sketches, sketch_len, consensus, changes, call_*]).
        want_call: also the species call of every read (skx_stream_bind_call) -- out["call_species"] [n_reads]: the lowest species
        whose leader has the largest sum; out["call_idx"], out["call_sum"] [n_reads, top]: that species' rows; out["call_codes"]
        [n_reads, F]: its consensus codes (None without a genotype table).  want_call_changes=cap (0: none): the reads at which the
        call changes -- species or index row (call_changes_codes: species or codes), read 0 always among them -- as out["call_events"]
        = dict(n_events, read, species, idx, sum[, codes]): n_events not capped, the arrays the first min(n_events, cap) entries.
        want_changes=cap: also the batch's change points -- the reads whose index row (changes_codes: whose consensus codes) differs
        from the previous read's, read 0 always among them -- as out["changes"] = dict(n, read, idx, sum[, codes]): n their number
        (not capped), the arrays the first min(n, cap) of them.  Rows are
        [n_reads, top] for a single reference and [n_reads, n_species, top] (genome indices local to the species)
        for a multi-species one; shared / table() hold the species one after the other.  want_consensus: the consensus codes of
        every read's rows, [n_reads, F] / [n_reads, n_species, F] (the reference needs a genotype table)."""
        L = _lib.load()
        bases = np.ascontiguousarray(bases, np.uint8)
        offsets = np.ascontiguousarray(offsets, np.uint64)
        n = len(offsets) - 1
        out = {}
        shape = (n, self.top) if self.ref.n_species == 1 else (n, self.ref.n_species, self.top)  # rows per species
        ti = np.zeros(shape, np.uint32) if self.top else None
        ts = np.zeros(shape, np.uint64) if self.top else None
        sh = np.zeros((n, self.ref.n_genomes), np.uint32) if want_shared else None
        sk = np.zeros((n, self.ref.s), np.uint64) if want_sketches else None
        sl = np.zeros(n, np.uint32) if want_sketches else None
        b = bases if len(bases) else np.zeros(1, np.uint8)
        cons = None
        if want_consensus:
            cons = np.zeros(shape[:-1] + (self.ref.n_features,), np.uint32)
            self.bind_consensus(_p(cons))
        if want_changes is not None:
            cap = int(want_changes)
            ev_n, ev_read = np.zeros(1, np.uint32), np.zeros(cap, np.uint32)
            ev_idx, ev_sum = np.zeros((cap,) + shape[1:], np.uint32), np.zeros((cap,) + shape[1:], np.uint64)
            ev_codes = np.zeros((cap,) + shape[1:-1] + (self.ref.n_features,), np.uint32) if changes_codes else None
            self.bind_changes(cap, _p(ev_n), _p(ev_read), _p(ev_idx), _p(ev_sum), _p(ev_codes))
        nf = self.ref.n_features if (want_call or want_call_changes) else 0
        if want_call:
            c_sp, c_idx, c_sum = np.zeros(n, np.uint32), np.zeros((n, self.top), np.uint32), np.zeros((n, self.top), np.uint64)
            c_codes = np.zeros((n, nf), np.uint32) if nf else None
            self.bind_call(_p(c_sp), _p(c_idx), _p(c_sum), _p(c_codes))
        if want_call_changes:
            ccap = int(want_call_changes)
            cev_n, cev_read, cev_sp = np.zeros(1, np.uint32), np.zeros(ccap, np.uint32), np.zeros(ccap, np.uint32)
            cev_idx, cev_sum = np.zeros((ccap, self.top), np.uint32), np.zeros((ccap, self.top), np.uint64)
            cev_codes = np.zeros((ccap, nf), np.uint32) if call_changes_codes else None
            self.bind_call_changes(ccap, _p(cev_n), _p(cev_read), _p(cev_sp), _p(cev_idx), _p(cev_sum), _p(cev_codes))
        _lib.check(L.skx_stream_push(self._h, _p(b), _p(offsets), n, _p(ti), _p(ts), _p(sh), _p(sk), _p(sl)))
        out.update(topk_idx=ti, topk_sum=ts, shared=sh, sketches=sk, sketch_len=sl)
        if want_call:
            out.update(call_species=c_sp, call_idx=c_idx, call_sum=c_sum, call_codes=c_codes)
        if want_call_changes:
            m = min(int(cev_n[0]), ccap)
            out["call_events"] = dict(n_events=int(cev_n[0]), read=cev_read[:m], species=cev_sp[:m], idx=cev_idx[:m], sum=cev_sum[:m])
            if call_changes_codes:
                out["call_events"]["codes"] = cev_codes[:m]
        if want_consensus:
            out["consensus"] = cons
        if want_changes is not None:
            m = min(int(ev_n[0]), cap)
            out["changes"] = dict(n=int(ev_n[0]), read=ev_read[:m], idx=ev_idx[:m], sum=ev_sum[:m])
            if changes_codes:
                out["changes"]["codes"] = ev_codes[:m]
        return out

    def push_device(self, d_bases, d_offsets, n_reads, n_bases, d_topk_idx=None, d_topk_sum=None, consensus=None, changes=None,
                    call=None, call_changes=None):
        """consensus: device pointer for the batch's consensus codes, bound right before the call (needs d_topk_idx);
        changes: (cap, n_events, ev_read[, ev_idx, ev_sum, ev_codes]) device pointers of an event list (bind_changes), likewise;
        call: (call_species[, call_idx, call_sum, call_codes]) device pointers of a species call (bind_call), and call_changes:
        (cap, n_events, ev_read, ev_species[, ev_idx, ev_sum, ev_codes]) of its event list (bind_call_changes), likewise (both need
        d_topk_idx and d_topk_sum)"""
        self._bind(consensus, changes, call, call_changes)
        _lib.check(_lib.load().skx_stream_push_device(self._h, d_bases, d_offsets, n_reads, n_bases, d_topk_idx, d_topk_sum))

    def enqueue_device(self, d_bases, d_offsets, n_reads, n_bases, d_topk_idx=None, d_topk_sum=None, consensus=None, changes=None,
                       call=None, call_changes=None):
        """push_device with the host wait of batch i overlapped by the sketch of batch i + 1: the passes (and any
        error) of a batch are queued by the NEXT enqueue / flush / sync.  Same rows, same table."""
        self._bind(consensus, changes, call, call_changes)
        _lib.check(_lib.load().skx_stream_enqueue_device(self._h, d_bases, d_offsets, n_reads, n_bases, d_topk_idx, d_topk_sum))

    def flush(self):
        _lib.check(_lib.load().skx_stream_flush(self._h))

    def set_packed_input(self, on=True):
        """From now on `bases` of every entry point are 4-bit packed (pack_reads()), offsets count bases."""
        _lib.check(_lib.load().skx_stream_set_packed_input(self._h, int(bool(on))))

    def sync(self):
        _lib.check(_lib.load().skx_stream_sync(self._h))

    def submit(self, h_bases, h_offsets, n_reads, h_topk_idx=None, h_topk_sum=None, consensus=None, changes=None,
               call=None, call_changes=None) -> int:
        """Queue a batch held in page-locked host memory (HostBuffer pointers / addresses); returns its ticket.  The
        copy overlaps the previous batch's kernels; rows are valid after wait(ticket) or drain().  consensus: page-locked
        pointer for the batch's consensus codes, bound right before the call; the row pointers may then be None.  changes:
        (cap, n_events, ev_read[, ev_idx, ev_sum, ev_codes]) page-locked pointers of an event list (bind_changes), likewise.
        call: (call_species[, call_idx, call_sum, call_codes]) and call_changes: (cap, n_events, ev_read, ev_species[, ev_idx, ev_sum,
        ev_codes]) page-locked pointers of a species call and its event list (bind_call, bind_call_changes), likewise."""
        self._bind(consensus, changes, call, call_changes)
        t = C.c_uint64(0)
        _lib.check(_lib.load().skx_stream_submit(self._h, h_bases, h_offsets, n_reads, h_topk_idx, h_topk_sum, C.byref(t)))
        return t.value

    def wait(self, ticket):
        _lib.check(_lib.load().skx_stream_wait(self._h, ticket))

    def drain(self):
        _lib.check(_lib.load().skx_stream_drain(self._h))

    def table(self) -> np.ndarray:
        cum = np.zeros(self.ref.n_genomes, np.uint64)
        _lib.check(_lib.load().skx_stream_table(self._h, _p(cum)))
        return cum

    def table_add(self, add):
        add = np.ascontiguousarray(add, np.uint64)
        assert len(add) == self.ref.n_genomes
        _lib.check(_lib.load().skx_stream_table_add(self._h, _p(add)))

    def reset(self):
        _lib.check(_lib.load().skx_stream_reset(self._h))

    @property
    def reads(self) -> int:
        n = C.c_uint64(0)
        _lib.check(_lib.load().skx_stream_reads(self._h, C.byref(n)))
        return n.value

    def rank(self, top=None):
        top = self.top if top is None else int(top)
        shape = (top,) if self.ref.n_species == 1 else (self.ref.n_species, top)
        idx, sm = np.zeros(shape, np.uint32), np.zeros(shape, np.uint64)
        _lib.check(_lib.load().skx_stream_rank(self._h, top, _p(idx), _p(sm)))
        return idx, sm

    def enable_coverage(self):
        """Give the stream its seen set (skx_stream_enable_coverage): before the first read, or after reset()."""
        _lib.check(_lib.load().skx_stream_enable_coverage(self._h))

    def coverage(self) -> np.ndarray:
        """covered[g] = hashes of genome g's column that some read so far has shared; uint32 [n_genomes], species one after the other."""
        cov = np.zeros(self.ref.n_genomes, np.uint32)
        _lib.check(_lib.load().skx_stream_coverage(self._h, _p(cov)))
        return cov

    def coverage_rows(self, genomes) -> np.ndarray:
        """The same for a list of global genome indices (any order, repeats allowed)."""
        genomes = np.ascontiguousarray(genomes, np.uint32).reshape(-1)
        cov = np.zeros(len(genomes), np.uint32)
        _lib.check(_lib.load().skx_stream_coverage_rows(self._h, _p(genomes), len(genomes), _p(cov)))
        return cov

    def coverage_rank(self, top):
        """Per species the first `top` genomes of (covered desc, index asc): (idx, covered), each [n_species, top], indices local to the species."""
        top = int(top)
        shape = (self.ref.n_species, max(top, 0))
        idx, cov = np.zeros(shape, np.uint32), np.zeros(shape, np.uint32)
        _lib.check(_lib.load().skx_stream_coverage_rank(self._h, top, _p(idx), _p(cov)))
        return idx, cov

    def winners(self):
        """(covered, won), each uint32 [n_genomes]: won[g] = seen hashes of g's column credited to g alone -- every seen hash goes to the
        first of its holders in the global order (containment, then covered, then index): skx_stream_winners, `mash screen -w`."""
        n = self.ref.n_genomes
        cov, won = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        _lib.check(_lib.load().skx_stream_winners(self._h, _p(cov), _p(won)))
        return cov, won

    def winners_rows(self, genomes):
        """The same for a list of global genome indices (any order, repeats allowed)."""
        genomes = np.ascontiguousarray(genomes, np.uint32).reshape(-1)
        cov, won = np.zeros(len(genomes), np.uint32), np.zeros(len(genomes), np.uint32)
        _lib.check(_lib.load().skx_stream_winners_rows(self._h, _p(genomes), len(genomes), _p(cov), _p(won)))
        return cov, won

    def winners_rank(self, top):
        """Per species the first `top` genomes of (won desc, index asc): (idx, won), each [n_species, top], indices local to the species."""
        top = int(top)
        shape = (self.ref.n_species, max(top, 0))
        idx, won = np.zeros(shape, np.uint32), np.zeros(shape, np.uint32)
        _lib.check(_lib.load().skx_stream_winners_rank(self._h, top, _p(idx), _p(won)))
        return idx, won

    def enable_depth(self):
        """Give the stream one saturating counter per reference hash (skx_stream_enable_depth; enables coverage too): before the first
        read, or after reset()."""
        _lib.check(_lib.load().skx_stream_enable_depth(self._h))

    def depth(self):
        """(covered, median, total), each [n_genomes]: hashes of genome g's column seen at all (uint32), the lower median of how many reads
        shared each of those (uint32), and the sum of the counters (uint64)."""
        n = self.ref.n_genomes
        cov, med, tot = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint64)
        _lib.check(_lib.load().skx_stream_depth(self._h, _p(cov), _p(med), _p(tot)))
        return cov, med, tot

    def depth_rows(self, genomes):
        """The same for a list of global genome indices (any order, repeats allowed)."""
        genomes = np.ascontiguousarray(genomes, np.uint32).reshape(-1)
        n = len(genomes)
        cov, med, tot = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint64)
        _lib.check(_lib.load().skx_stream_depth_rows(self._h, _p(genomes), n, _p(cov), _p(med), _p(tot)))
        return cov, med, tot

    def depth_count(self) -> int:
        """Distinct reference hashes seen so far (lifted ones included)."""
        n = C.c_uint64(0)
        _lib.check(_lib.load().skx_stream_depth_count(self._h, C.byref(n)))
        return int(n.value)

    def depth_export(self):
        """The counters as (hashes uint64, counts uint32) of the hashes seen, in no particular order: the portable form of the state."""
        cap = self.depth_count()
        hashes, counts = np.zeros(cap, np.uint64), np.zeros(cap, np.uint32)
        n = C.c_uint64(0)
        _lib.check(_lib.load().skx_stream_depth_export(self._h, _p(hashes), _p(counts), cap, C.byref(n)))
        assert int(n.value) == cap, "the stream moved between depth_count and depth_export"
        return hashes, counts

    def depth_import(self, hashes, counts) -> int:
        """Add (hash, count) pairs to the counters (saturating; the hashes become seen); returns how many named no hash of this reference."""
        hashes = np.ascontiguousarray(hashes, np.uint64).reshape(-1)
        counts = np.ascontiguousarray(counts, np.uint32).reshape(-1)
        if len(hashes) != len(counts):
            raise ValueError("hashes and counts differ in length")
        unknown = C.c_uint64(0)
        _lib.check(_lib.load().skx_stream_depth_import(self._h, _p(hashes), _p(counts), len(hashes), C.byref(unknown)))
        return int(unknown.value)

    def enable_composition(self, min_hits=1):
        """Classify every read by its own sketch's hits per species (skx_stream_enable_composition): before the first read, or after
        reset().  A read whose best species has fewer than `min_hits` hits is unclassified."""
        _lib.check(_lib.load().skx_stream_enable_composition(self._h, int(min_hits)))

    def composition(self):
        """(reads, pairs), uint64: reads [n_species + 2] = reads per species, then ambiguous (several species tie for the most hits), then
        unclassified; pairs [n_species] = the reads' hits per species, whatever their class."""
        n = self.ref.n_species
        reads, pairs = np.zeros(n + 2, np.uint64), np.zeros(n, np.uint64)
        _lib.check(_lib.load().skx_stream_composition(self._h, _p(reads), _p(pairs)))
        return reads, pairs

    def consensus(self, top=None) -> np.ndarray:
        """Consensus codes of the CURRENT table: rank(top) followed by the reference's consensus_rows -> [F] / [n_species, F]."""
        idx, _ = self.rank(top)
        return self.ref.consensus_rows(idx)

    def stats(self):
        """Counters of the stream (skx_stream_stats): pairs / passes of the last push, dictionary size, ..."""
        v = (C.c_uint64 * 18)()
        _lib.check(_lib.load().skx_stream_stats(self._h, v, 18))
        names = ("last_pairs", "last_passes", "dictionary_size", "reads_block_sketcher", "passes", "passes_lean_scan",
                 "pair_capacity", "live_rank_groups", "reads_split_over_waves", "read_segments", "row_pool_grown",
                 "passes_shared", "groups_unshared", "query_rows", "query_rows_grown", "dictionary_dense", "batches_compact", "batches_full")
        return dict(zip(names, [int(x) for x in v]))

    def set_profiling(self, on=True):
        """False/0: off; True/1: every stage; 2: only the reference scan (cheapest way to time the roofline kernel)."""
        _lib.check(_lib.load().skx_stream_set_profiling(self._h, int(on)))

    def profile(self):
        ms = (C.c_double * _lib.N_STAGES)()
        n = (C.c_uint64 * _lib.N_STAGES)()
        _lib.check(_lib.load().skx_stream_profile(self._h, ms, n))
        return {name: dict(ms=ms[i], launches=int(n[i])) for i, name in enumerate(_lib.STAGE_NAMES)}

    def scan_alone(self, reps=3) -> float:
        """average milliseconds of `reps` reference scans with nothing beside them (streams on a reference with a static dense dictionary)"""
        ms = C.c_double(0)
        _lib.check(_lib.load().skx_stream_scan_alone(self._h, int(reps), C.byref(ms)))
        return ms.value

    def allreduce(self, comm):
        _lib.check(_lib.load().skx_stream_allreduce(self._h, comm._h))

    def close(self):
        if getattr(self, "_h", None):
            _lib.load().skx_stream_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Comm:
    """RCCL communicator (one process per GPU)."""

    @staticmethod
    def unique_id() -> bytes:
        buf = (C.c_uint8 * _lib.COMM_ID_BYTES)()
        _lib.check(_lib.load().skx_comm_unique_id(buf))
        return bytes(buf)

    def __init__(self, device, rank, n_ranks, uid: bytes):
        buf = (C.c_uint8 * _lib.COMM_ID_BYTES).from_buffer_copy(uid)
        h = C.c_void_p()
        _lib.check(_lib.load().skx_comm_create(C.byref(h), device, rank, n_ranks, buf))
        self._h = h

    @property
    def n_ranks(self) -> int:
        n = C.c_int(0)
        _lib.check(_lib.load().skx_comm_n_ranks(self._h, C.byref(n)))
        return n.value

    def close(self):
        if getattr(self, "_h", None):
            _lib.load().skx_comm_destroy(self._h)
            self._h = None


def changes_rows(rows, cap=None, device=0):
    """Change points of rows held on the host (skx_changes_rows): rows [n, ...] uint32, compared row by row over all trailing axes
    (1..4096 values per row).  Returns (n_events, ev_row): the number of rows that differ from the row before them, row 0 included
    -- not capped --, and the first min(n_events, cap) of their indices (uint64); cap None: room for all."""
    rows = np.ascontiguousarray(rows, np.uint32)
    n = rows.shape[0] if rows.ndim else 0
    width = int(np.prod(rows.shape[1:], dtype=np.int64)) if rows.ndim > 1 else 1
    cap = n if cap is None else int(cap)
    ev = np.zeros(max(cap, 1), np.uint64)
    n_ev = C.c_uint64(0)
    src = rows if rows.size else np.zeros(1, np.uint32)
    _lib.check(_lib.load().skx_changes_rows(device, _p(src), n, width, cap, C.byref(n_ev), _p(ev)))
    return n_ev.value, ev[:min(n_ev.value, cap)]


def call_rows(idx, sums, codes=None, device=0):
    """Species call of rows held on the host (skx_call_rows): idx uint32 / sums uint64 [n, n_species, top], codes uint32
    [n, n_species, F] or None.  Returns dict(call_species [n], call_idx, call_sum [n, top], call_codes [n, F] or None): per row the
    lowest species whose leader sums[r, sp, 0] is the largest, and that species' rows."""
    idx = np.ascontiguousarray(idx, np.uint32)
    sums = np.ascontiguousarray(sums, np.uint64)
    if idx.ndim != 3 or idx.shape != sums.shape:
        raise ValueError("idx and sums must both be [n_rows, n_species, top]")
    n, n_sp, top = idx.shape
    nf = 0
    if codes is not None:
        codes = np.ascontiguousarray(codes, np.uint32)
        if codes.ndim != 3 or codes.shape[:2] != (n, n_sp):
            raise ValueError("codes must be [n_rows, n_species, n_features]")
        nf = codes.shape[2]
    c_sp, c_idx, c_sum = np.zeros(n, np.uint32), np.zeros((n, top), np.uint32), np.zeros((n, top), np.uint64)
    c_codes = np.zeros((n, nf), np.uint32) if codes is not None else None
    pad = lambda a, t: a if a.size else np.zeros(1, t)  # (an empty array has no address worth passing)
    _lib.check(_lib.load().skx_call_rows(device, _p(pad(idx, np.uint32)), _p(pad(sums, np.uint64)),
                                         _p(pad(codes, np.uint32)) if codes is not None else None, n, n_sp, top, nf,
                                         _p(pad(c_sp, np.uint32)), _p(pad(c_idx, np.uint32)), _p(pad(c_sum, np.uint64)),
                                         _p(pad(c_codes, np.uint32)) if codes is not None else None))
    return dict(call_species=c_sp, call_idx=c_idx, call_sum=c_sum, call_codes=c_codes)


def sketch_reads(bases, offsets, k=16, seed=0, s=1000, device=0):
    """finch MashSketcher process/to_vec per read: ([n_reads, s] uint64 ascending, lengths)."""
    bases = np.ascontiguousarray(bases, np.uint8)
    offsets = np.ascontiguousarray(offsets, np.uint64)
    n = len(offsets) - 1
    sk = np.zeros((n, s), np.uint64)
    sl = np.zeros(n, np.uint32)
    b = bases if len(bases) else np.zeros(1, np.uint8)
    _lib.check(_lib.load().skx_sketch_reads(device, k, seed, s, _p(b), _p(offsets), n, _p(sk), _p(sl)))
    return sk, sl


def sketch_groups(bases, offsets, group_first, k=16, seed=0, s=1000, device=0, want_valid_kmers=False, want_counts=False):
    """finch MashSketcher fed several records: ONE bottom-s sketch per group of records, pooled on the device.
    Group g = records [group_first[g], group_first[g + 1]).  Returns ([n_groups, s] uint64 ascending zero-padded, lengths
    [, valid k-mer windows per group][, counts]).  want_counts: the LAST element is [n_groups, s] uint32, counts[g, j] = valid
    k-mer windows of group g whose hash is sketches[g, j] (finch's KmerCount.count, Mash's counts32), zero beyond the length."""
    bases = np.ascontiguousarray(bases, np.uint8)
    offsets = np.ascontiguousarray(offsets, np.uint64)
    group_first = np.ascontiguousarray(group_first, np.uint32)
    n, ng = len(offsets) - 1, len(group_first) - 1
    sk = np.zeros((ng, s), np.uint64)
    sl = np.zeros(ng, np.uint32)
    vk = np.zeros(ng, np.uint64) if want_valid_kmers else None
    b = bases if len(bases) else np.zeros(1, np.uint8)
    if want_counts:
        kc = np.zeros((ng, s), np.uint32)
        _lib.check(_lib.load().skx_sketch_groups_counts(device, k, seed, s, _p(b), _p(offsets), n, _p(group_first), ng, _p(sk), _p(sl),
                                                        _p(vk) if want_valid_kmers else None, _p(kc)))
        return (sk, sl, vk, kc) if want_valid_kmers else (sk, sl, kc)
    _lib.check(_lib.load().skx_sketch_groups(device, k, seed, s, _p(b), _p(offsets), n, _p(group_first), ng, _p(sk), _p(sl),
                                             _p(vk) if want_valid_kmers else None))
    return (sk, sl, vk) if want_valid_kmers else (sk, sl)


class DeviceBuffer:
    """A raw HBM allocation (bench path: inputs resident on the device before timing starts)."""

    def __init__(self, nbytes, device=0):
        self.device, self.nbytes = device, int(nbytes)
        p = C.c_void_p()
        _lib.check(_lib.load().skx_dev_malloc(device, C.byref(p), self.nbytes))
        self.ptr = p

    @classmethod
    def from_numpy(cls, a, device=0):
        a = np.ascontiguousarray(a)
        buf = cls(max(a.nbytes, 1), device)
        if a.nbytes:
            _lib.check(_lib.load().skx_dev_upload(device, buf.ptr, _p(a), a.nbytes))
        return buf

    def to_numpy(self, dtype, shape):
        out = np.zeros(shape, dtype)
        _lib.check(_lib.load().skx_dev_download(self.device, _p(out), self.ptr, out.nbytes))
        return out

    def free(self):
        if self.ptr:
            _lib.load().skx_dev_free(self.device, self.ptr)
            self.ptr = None


class HostBuffer:
    """Page-locked host memory (skx_host_alloc) with a numpy view: batch buffers for SumOfSharedHashes.submit."""

    def __init__(self, nbytes, device=0):
        self.device, self.nbytes = device, int(nbytes)
        p = C.c_void_p()
        _lib.check(_lib.load().skx_host_alloc(device, C.byref(p), max(self.nbytes, 1)))
        self.ptr = p

    def view(self, dtype, count=None, offset=0):
        dt = np.dtype(dtype)
        count = (self.nbytes - offset) // dt.itemsize if count is None else count
        buf = (C.c_uint8 * (count * dt.itemsize)).from_address(self.ptr.value + offset)
        return np.frombuffer(buf, dtype=dt, count=count)

    def free(self):
        if self.ptr:
            _lib.load().skx_host_free(self.device, self.ptr)
            self.ptr = None
