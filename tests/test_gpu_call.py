"""The species call of a multi-species stream (skx_stream_bind_call, skx_stream_bind_call_changes) against call_cases.call_ref /
call_changes_ref applied to the ORACLE's per-species rows: one orc.stream per species over the same reads, as
tests/test_gpu_species.py::_oracle, started from the seeded table where one is seeded.  Every entry point and memory kind, every
ranking path (top 1, 3, 17; compact batches), ties, batches cut by the caller, truncated event lists and the one-shot binding."""
import ctypes as C
import functools

import numpy as np
import pytest

from call_cases import call_changes_ref, call_ref
from helpers import pack_reads, unpack_reads, workload_species
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

K_MER, SEED = 16, 0
SENT = {np.dtype(np.uint32): 0xDEADBEEF, np.dtype(np.uint64): 0xDEADBEEFDEADBEEF}


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


# ---------------------------------------------------------------- expectations
def oracle_rows(refs, bases, offsets, top, cums=None):
    """the rows a multi-species stream returns, [n, n_species, top], from one oracle run per species"""
    outs = [orc.stream(K_MER, SEED, r["ref"].shape[1], r["ref"], r["col_len"], bases, offsets, top_k=top,
                       cum=None if cums is None else cums[i]) for i, r in enumerate(refs)]
    return (np.stack([o["topk_idx"] for o in outs], axis=1).astype(np.uint32), np.stack([o["topk_sum"] for o in outs], axis=1).astype(np.uint64),
            np.concatenate([o["cum"] for o in outs]))


def consensus_ref(idx, codes, sizes):
    """skx_ref_set_genotypes' vote: per (read, species, column) the code most of the `top` rows carry, ties to the smallest code"""
    g0 = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    n, n_sp, top = idx.shape
    out = np.zeros((n, n_sp, codes.shape[1]), np.uint32)
    for r in range(n):
        for sp in range(n_sp):
            rows = codes[g0[sp] + idx[r, sp]]
            for f in range(codes.shape[1]):
                col = rows[:, f].tolist()
                out[r, sp, f] = min(set(col), key=lambda v: (-col.count(v), v))
    return out


def by_origin(refs, bases, offsets, blocks):
    """the reads of a workload_species stream regrouped by the species they were drawn from: blocks = [(species, count), ...] taken
    in that order, whatever is left behind them.  A read's origin is the species in which it shares most hashes with any genome."""
    shared = [orc.stream(K_MER, SEED, r["ref"].shape[1], r["ref"], r["col_len"], bases, offsets, top_k=1, want_shared=True)["shared"].max(axis=1)
              for r in refs]
    origin = np.argmax(np.stack(shared, axis=1), axis=1)
    pools = [list(np.flatnonzero(origin == sp)) for sp in range(len(refs))]
    order = []
    for sp, m in blocks:
        order += pools[sp][:m]   # (reads that hit nothing count for species 0: a pool may be a little short)
        pools[sp] = pools[sp][m:]
    order += sorted(i for p in pools for i in p)
    reads = unpack_reads(bases, offsets)
    return pack_reads([reads[i] for i in order])


# ---------------------------------------------------------------- driving a stream
class Mem:
    """named arrays of one batch in the memory its entry point takes (host / device / pinned), filled with a sentinel"""

    def __init__(self, kind, spec):
        from sketchy_amd import api
        self.kind, self.spec, self.bufs = kind, spec, {}
        for name, (shape, dtype) in spec.items():
            fill = np.full(shape, SENT[np.dtype(dtype)], dtype)
            if kind == "device":
                self.bufs[name] = api.DeviceBuffer.from_numpy(fill)
            elif kind == "pinned":
                hb = api.HostBuffer(max(fill.nbytes, 8))
                hb.view(dtype, fill.size)[:] = fill.ravel()
                self.bufs[name] = hb
            else:
                self.bufs[name] = fill

    def ptr(self, name):
        if name not in self.bufs:
            return None
        return _p(self.bufs[name]) if self.kind == "host" else self.bufs[name].ptr

    def read(self):
        out = {}
        for name, (shape, dtype) in self.spec.items():
            b = self.bufs[name]
            if self.kind == "device":
                out[name] = b.to_numpy(dtype, shape)
            elif self.kind == "pinned":
                out[name] = b.view(dtype, int(np.prod(shape))).reshape(shape).copy()
            else:
                out[name] = b
        return out

    def free(self):
        if self.kind != "host":
            for b in self.bufs.values():
                b.free()


def drive(S, entry, bases, offsets, cuts, top, n_sp, nf=0, call=True, codes=False, cap=0, codes_mode=False, also=False,
          null_rows=False, packed=False, bound=None):
    """every batch [cuts[i], cuts[i + 1]) through one entry point -> one dict of arrays per batch.  call: bind the call (codes: with
    its codes); cap: bind the call's event list of that many entries (codes_mode: compared by codes); also: a consensus output and
    an event list of the full rows as well; bound: the batches that get bindings (default: all)"""
    from sketchy_amd import _lib, api
    L = _lib.load()
    kind = {"push": "host", "submit": "pinned"}.get(entry, "device")
    mems, extra = [], []
    if packed:
        S.set_packed_input(True)
        bases, offsets = api.pack_reads(bases, offsets)
    try:
        if kind == "pinned":
            hb, ho = api.HostBuffer(max(len(bases), 8)), api.HostBuffer(len(offsets) * 8)
            hb.view(np.uint8, len(bases))[:] = bases
            ho.view(np.uint64, len(offsets))[:] = offsets
            extra += [hb, ho]
        elif kind == "device":
            d_b = api.DeviceBuffer.from_numpy(bases)
            extra.append(d_b)
        for i, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
            n = b - a
            on = bound is None or i in bound
            spec = dict(rows_idx=((n, n_sp, top), np.uint32), rows_sum=((n, n_sp, top), np.uint64),
                        call_sp=((n,), np.uint32), call_idx=((n, top), np.uint32), call_sum=((n, top), np.uint64))
            if codes:
                spec["call_codes"] = ((n, nf), np.uint32)
            if cap:
                spec.update(cev_n=((1,), np.uint32), cev_read=((cap,), np.uint32), cev_sp=((cap,), np.uint32),
                            cev_idx=((cap, top), np.uint32), cev_sum=((cap, top), np.uint64))
                if codes_mode:
                    spec["cev_codes"] = ((cap, nf), np.uint32)
            if also:
                spec.update(cons=((n, n_sp, nf), np.uint32), chg_n=((1,), np.uint32), chg_read=((n,), np.uint32),
                            chg_idx=((n, n_sp, top), np.uint32), chg_sum=((n, n_sp, top), np.uint64))
            M = Mem(kind, spec)
            mems.append(M)
            q = M.ptr
            if on and also:
                S.bind_consensus(q("cons"))
                S.bind_changes(n, q("chg_n"), q("chg_read"), q("chg_idx"), q("chg_sum"))
            if on and call:
                S.bind_call(q("call_sp"), q("call_idx"), q("call_sum"), q("call_codes"))
            if on and cap:
                S.bind_call_changes(cap, q("cev_n"), q("cev_read"), q("cev_sp"), q("cev_idx"), q("cev_sum"), q("cev_codes"))
            ri, rs = (None, None) if null_rows else (q("rows_idx"), q("rows_sum"))
            if entry == "push":
                o = np.ascontiguousarray(offsets[a:b + 1], np.uint64)
                _lib.check(L.skx_stream_push(S._h, _p(bases), _p(o), n, ri, rs, None, None, None))
            elif entry == "submit":
                S.submit(hb.ptr, C.c_void_p(ho.ptr.value + a * 8), n, ri, rs)
            else:
                d_o = api.DeviceBuffer.from_numpy(np.ascontiguousarray(offsets[a:b + 1], np.uint64))
                extra.append(d_o)
                fn = S.enqueue_device if entry == "enqueue_device" else S.push_device
                fn(d_b.ptr, d_o.ptr, n, int(offsets[b] - offsets[a]), ri, rs)
        if entry == "submit":
            S.drain()
        elif kind == "device":
            S.sync()
        return [M.read() for M in mems]
    finally:
        for x in extra + mems:
            x.free()


def untouched(got, names):
    return all((got[k] == SENT[got[k].dtype]).all() for k in names if k in got)


def check(got, cuts, idx, sm, codes=None, cap=0, codes_mode=False, rows=True, what=""):
    """got: drive()'s batches; idx / sm / codes: the expected full rows (and voted codes) of all reads"""
    total = 0
    for g, a, b in zip(got, cuts[:-1], cuts[1:]):
        w = f"{what} batch at {a}"
        want = call_ref(idx[a:b], sm[a:b], None if codes is None else codes[a:b])
        if rows:
            np.testing.assert_array_equal(g["rows_sum"], sm[a:b], err_msg=w)
            np.testing.assert_array_equal(g["rows_idx"], idx[a:b], err_msg=w)
        else:
            assert untouched(g, ("rows_idx", "rows_sum")), w
        np.testing.assert_array_equal(g["call_sp"], want["call_species"], err_msg=w)
        np.testing.assert_array_equal(g["call_sum"], want["call_sum"], err_msg=w)
        np.testing.assert_array_equal(g["call_idx"], want["call_idx"], err_msg=w)
        if "call_codes" in g:
            np.testing.assert_array_equal(g["call_codes"], want["call_codes"], err_msg=w)
        if cap:
            ev = call_changes_ref(want["call_species"], want["call_codes"] if codes_mode else want["call_idx"])
            m = min(len(ev), cap)
            total += len(ev)
            assert int(g["cev_n"][0]) == len(ev), w
            np.testing.assert_array_equal(g["cev_read"][:m], ev[:m], err_msg=w)
            np.testing.assert_array_equal(g["cev_sp"][:m], want["call_species"][ev[:m]], err_msg=w)
            np.testing.assert_array_equal(g["cev_idx"][:m], want["call_idx"][ev[:m]], err_msg=w)
            np.testing.assert_array_equal(g["cev_sum"][:m], want["call_sum"][ev[:m]], err_msg=w)
            if codes_mode:
                np.testing.assert_array_equal(g["cev_codes"][:m], want["call_codes"][ev[:m]], err_msg=w)
            for k in ("cev_read", "cev_sp", "cev_idx", "cev_sum", "cev_codes"):
                assert k not in g or (g[k][m:] == SENT[g[k].dtype]).all(), f"{w}: {k} past min(n_events, cap) was written"
    return total


# ---------------------------------------------------------------- three species
SIZES = (130, 700, 513)
N_FEAT = 4


@functools.lru_cache(maxsize=None)
def three():
    """the stream of tests/test_gpu_species.py, its reads regrouped so that the lead passes from species 0 to 1 to 2"""
    refs, bases, offsets = workload_species(list(SIZES), 300, 240, read_len=800, genome_len=90000, rng_seed=201)
    bases, offsets = by_origin(refs, bases, offsets, [(0, 25), (1, 55), (2, 80)])
    codes = np.random.default_rng(17).integers(0, 4, size=(sum(SIZES), N_FEAT), dtype=np.uint32)
    return refs, bases, offsets, codes


@functools.lru_cache(maxsize=None)
def three_expected(top):
    refs, bases, offsets, codes = three()
    idx, sm, cum = oracle_rows(refs, bases, offsets, top)
    sp = call_ref(idx, sm)["call_species"]
    flips = int((sp[1:] != sp[:-1]).sum())
    assert len(set(sp.tolist())) >= 2 and flips >= 2, (top, sp.tolist())  # (a stream that never flips would pass silently)
    return idx, sm, cum, consensus_ref(idx, codes, SIZES)


@pytest.fixture(scope="module")
def three_ref(gpu):
    from sketchy_amd import api
    refs, bases, offsets, codes = three()
    R = api.ReferenceSketch([r["ref"] for r in refs], [r["col_len"] for r in refs])
    R.set_genotypes(codes)
    yield R
    R.close()


def _stream(R, top, n, n_bases, coalesce=None, seed=None):
    from sketchy_amd import api
    before = api.get_option("stream_coalesce")
    try:
        if coalesce:
            api.set_option("stream_coalesce", coalesce)
        S = api.SumOfSharedHashes(R, top=top, max_batch_reads=n, max_batch_bases=max(1, n_bases))
    finally:
        api.set_option("stream_coalesce", before)
    if seed is not None:
        S.table_add(seed)
    return S


@pytest.mark.parametrize("top", [1, 3, 17])
def test_three_species_call_rows_sums_and_codes(three_ref, top):
    """pruned top-1, pruned top-k and the generic ranking; three pushes; species, index rows, sums and codes of the called species,
    and both kinds of event list"""
    refs, bases, offsets, _ = three()
    idx, sm, cum, cons = three_expected(top)
    cuts = [0, 80, 160, 240]
    for codes_mode in (False, True):
        S = _stream(three_ref, top, 240, len(bases))
        got = drive(S, "push", bases, offsets, cuts, top, 3, N_FEAT, codes=True, cap=240, codes_mode=codes_mode)
        total = check(got, cuts, idx, sm, cons, cap=240, codes_mode=codes_mode, what=f"top {top} codes_mode {codes_mode}")
        assert 3 < total < 240
        np.testing.assert_array_equal(S.table(), cum)
        S.close()


def test_python_push_keywords(three_ref):
    refs, bases, offsets, _ = three()
    idx, sm, cum, cons = three_expected(3)
    S = _stream(three_ref, 3, 240, len(bases))
    out = S.push(bases, offsets, want_call=True, want_call_changes=240)
    want = call_ref(idx, sm, cons)
    for k in ("call_species", "call_idx", "call_sum", "call_codes"):
        np.testing.assert_array_equal(out[k], want[k], err_msg=k)
    np.testing.assert_array_equal(out["topk_idx"], idx)
    ev = call_changes_ref(want["call_species"], want["call_idx"])
    e = out["call_events"]
    assert e["n_events"] == len(ev) and e["read"].tolist() == ev.tolist() and e["species"].tolist() == want["call_species"][ev].tolist()
    np.testing.assert_array_equal(e["idx"], want["call_idx"][ev])
    np.testing.assert_array_equal(e["sum"], want["call_sum"][ev])
    S.reset()
    e = S.push(bases, offsets, want_call_changes=5, call_changes_codes=True)["call_events"]
    ev = call_changes_ref(want["call_species"], want["call_codes"])
    assert e["n_events"] == len(ev) > 5 and e["read"].tolist() == ev[:5].tolist()
    np.testing.assert_array_equal(e["codes"], want["call_codes"][ev[:5]])
    assert "call_species" not in S.push(bases, offsets[:3])
    S.close()


# ---------------------------------------------------------------- every entry point
ENTRIES = [("push", False, False), ("push", True, False), ("push_device", False, False), ("enqueue_device", False, False),
           ("submit", False, False), ("submit", True, False), ("submit", True, True)]


@pytest.mark.parametrize("entry,null_rows,packed", ENTRIES,
                         ids=("push", "push_null_rows", "push_device", "enqueue_device", "submit", "submit_null_rows", "submit_packed"))
def test_every_entry_point(three_ref, entry, null_rows, packed):
    """four batches (three enqueued ones share a pass), call and call events bound to the first three only: the call of every entry
    point is the reference's, the rows and the table are an unbound stream's, and the fourth batch writes nothing anywhere"""
    refs, bases, offsets, _ = three()
    idx, sm, cum, cons = three_expected(3)
    cuts = [0, 60, 130, 190, 240]
    S = _stream(three_ref, 3, 80, len(bases), coalesce=3)
    got = drive(S, entry, bases, offsets, cuts, 3, 3, N_FEAT, codes=True, cap=16, null_rows=null_rows, packed=packed, bound=(0, 1, 2))
    check(got[:3], cuts[:4], idx, sm, cons, cap=16, rows=not null_rows, what=entry)
    last = got[3]
    assert untouched(last, ("call_sp", "call_idx", "call_sum", "call_codes", "cev_n", "cev_read", "cev_sp", "cev_idx", "cev_sum")), "one-shot"
    if not null_rows:
        np.testing.assert_array_equal(last["rows_idx"], idx[190:])
        np.testing.assert_array_equal(last["rows_sum"], sm[190:])
    np.testing.assert_array_equal(S.table(), cum)
    if entry == "enqueue_device":
        assert S.stats()["passes_shared"] >= 1, S.stats()
    S.close()


@pytest.mark.parametrize("entry", ("push", "enqueue_device", "submit"))
def test_all_four_bindings_on_one_batch(three_ref, entry):
    from test_changes_cpu import changes_ref
    refs, bases, offsets, _ = three()
    idx, sm, cum, cons = three_expected(3)
    cuts = [0, 90, 170, 240]
    for codes_mode in (False, True):
        S = _stream(three_ref, 3, 90, len(bases), coalesce=3)
        got = drive(S, entry, bases, offsets, cuts, 3, 3, N_FEAT, codes=True, cap=90, codes_mode=codes_mode, also=True)
        check(got, cuts, idx, sm, cons, cap=90, codes_mode=codes_mode, what=entry)
        for g, a, b in zip(got, cuts[:-1], cuts[1:]):
            np.testing.assert_array_equal(g["cons"], cons[a:b])
            ev = changes_ref(idx[a:b])
            assert int(g["chg_n"][0]) == len(ev)
            np.testing.assert_array_equal(g["chg_read"][:len(ev)], ev)
            np.testing.assert_array_equal(g["chg_idx"][:len(ev)], idx[a:b][ev])
            np.testing.assert_array_equal(g["chg_sum"][:len(ev)], sm[a:b][ev])
        S.close()


# ---------------------------------------------------------------- events
def test_events_truncated_and_batches_cut_inside_a_run(three_ref):
    refs, bases, offsets, _ = three()
    idx, sm, cum, cons = three_expected(1)
    want = call_ref(idx, sm, cons)
    ev = call_changes_ref(want["call_species"], want["call_idx"])
    inside = sorted(set(range(20, 220)) - set(ev.tolist()))  # reads that are no change point: a batch beginning there is inside a run
    assert len(inside) >= 2 and len(ev) > 8
    cuts = [0, inside[0], inside[len(inside) // 2], 240]
    assert max(b - a for a, b in zip(cuts[:-1], cuts[1:])) <= 240
    for entry in ("push", "push_device", "submit"):
        S = _stream(three_ref, 1, 240, len(bases))
        got = drive(S, entry, bases, offsets, cuts, 1, 3, N_FEAT, cap=240)
        total = check(got, cuts, idx, sm, cap=240, what=entry)
        assert all(int(g["cev_read"][0]) == 0 for g in got) and total == len(ev) + 2  # every batch starts with an event of its own
        S.close()
    for entry in ("push", "enqueue_device", "submit"):  # cap below n_events
        S = _stream(three_ref, 1, 240, len(bases))
        got = drive(S, entry, bases, offsets, [0, 240], 1, 3, N_FEAT, cap=4, codes=True, codes_mode=True)
        check(got, [0, 240], idx, sm, cons, cap=4, codes_mode=True, what=entry)
        assert int(got[0]["cev_n"][0]) > 4
        S.close()


def test_events_without_the_call_and_without_optional_columns(three_ref):
    """an event list alone (the compact rows live in the lane's scratch), and one that asks for nothing but reads and species"""
    from sketchy_amd import api
    refs, bases, offsets, _ = three()
    idx, sm, cum, cons = three_expected(3)
    S = _stream(three_ref, 3, 240, len(bases))
    got = drive(S, "push_device", bases, offsets, [0, 240], 3, 3, N_FEAT, call=False, cap=240, codes_mode=True)[0]
    want = call_ref(idx, sm, cons)
    ev = call_changes_ref(want["call_species"], want["call_codes"])
    assert int(got["cev_n"][0]) == len(ev) and untouched(got, ("call_sp", "call_idx", "call_sum"))
    np.testing.assert_array_equal(got["cev_read"][:len(ev)], ev)
    np.testing.assert_array_equal(got["cev_sp"][:len(ev)], want["call_species"][ev])
    np.testing.assert_array_equal(got["cev_idx"][:len(ev)], want["call_idx"][ev])
    np.testing.assert_array_equal(got["cev_sum"][:len(ev)], want["call_sum"][ev])
    np.testing.assert_array_equal(got["cev_codes"][:len(ev)], want["call_codes"][ev])
    S.reset()
    n_ev, rd, sp = np.zeros(1, np.uint32), np.full(240, 7, np.uint32), np.full(240, 7, np.uint32)
    only_sp = np.full(240, 7, np.uint32)
    S.bind_call(_p(only_sp))
    S.bind_call_changes(240, _p(n_ev), _p(rd), _p(sp))
    S.push(bases, offsets)
    ev = call_changes_ref(want["call_species"], want["call_idx"])
    assert int(n_ev[0]) == len(ev) and rd[:len(ev)].tolist() == ev.tolist() and sp[:len(ev)].tolist() == want["call_species"][ev].tolist()
    assert (rd[len(ev):] == 7).all() and only_sp.tolist() == want["call_species"].tolist()
    S.close()


# ---------------------------------------------------------------- ties
def test_ties_zero_leads_and_one_species(gpu):
    from sketchy_amd import api
    refs, bases, offsets = workload_species([60, 60], 128, 90, read_len=500, genome_len=40000, rng_seed=211)
    refs[1]["ref"][:] = refs[0]["ref"]            # the same genomes in two species: equal leads at every read
    refs[1]["col_len"][:] = refs[0]["col_len"]
    junk = np.random.default_rng(3).choice(np.frombuffer(b"ACGT", np.uint8), size=(6, 300))
    reads = [j.tobytes() for j in junk] + unpack_reads(bases, offsets)  # six reads that hit nothing open the batch
    bases, offsets = pack_reads(reads)
    idx, sm, cum = oracle_rows(refs, bases, offsets, 1)
    assert (sm[:6] == 0).all() and (sm[6:, 0] == sm[6:, 1]).all() and sm[-1].min() > 0
    R = api.ReferenceSketch([r["ref"] for r in refs], [r["col_len"] for r in refs])
    for entry in ("push", "enqueue_device"):
        S = _stream(R, 1, 96, len(bases))
        got = drive(S, entry, bases, offsets, [0, 96], 1, 2, cap=96)
        check(got, [0, 96], idx, sm, cap=96, what=entry)
        assert (got[0]["call_sp"] == 0).all()
        S.close()
    R.close()
    # one species: species 0 and the plain rows
    R = api.ReferenceSketch(refs[0]["ref"], refs[0]["col_len"])
    S = _stream(R, 3, 96, len(bases))
    idx, sm, cum = oracle_rows(refs[:1], bases, offsets, 3)
    got = drive(S, "push", bases, offsets, [0, 50, 96], 3, 1, cap=96)
    check(got, [0, 50, 96], idx, sm, cap=96, what="one species")
    for g in got:
        assert (g["call_sp"] == 0).all()
        np.testing.assert_array_equal(g["call_idx"], g["rows_idx"][:, 0])
        np.testing.assert_array_equal(g["call_sum"], g["rows_sum"][:, 0])
    S.close()
    R.close()


# ---------------------------------------------------------------- compact ranking
def test_compact_ranking(three_ref):
    """a table seeded (skx_stream_table_add) with five contenders per species, species 1's far ahead: the enqueued batches rank on
    their candidates, whose slots become genome indices (launch_cand_rows_back) before the selection may copy them"""
    refs, bases, offsets, _ = three()
    rng = np.random.default_rng(9)
    cums = []
    for sp, n in enumerate(SIZES):
        c = np.zeros(n, np.uint64)
        c[rng.choice(n, 5, replace=False)] = (1 << 33) * (3 if sp == 1 else 1) + rng.integers(0, 1000, 5).astype(np.uint64)
        cums.append(c)
    idx, sm, cum = oracle_rows(refs, bases, offsets, 3, cums)
    cons = consensus_ref(idx, three()[3], SIZES)
    assert (call_ref(idx, sm)["call_species"] == 1).all()
    cuts = [0, 80, 160, 240]
    S = _stream(three_ref, 3, 80, len(bases), coalesce=3, seed=np.concatenate(cums))
    got = drive(S, "enqueue_device", bases, offsets, cuts, 3, 3, N_FEAT, codes=True, cap=80)
    st = S.stats()
    assert st["batches_compact"] >= 1, st
    check(got, cuts, idx, sm, cons, cap=80, what="compact")
    np.testing.assert_array_equal(S.table(), cum)
    S.close()


def test_genotype_table_set_after_the_first_event_list(gpu):
    """skx_ref_set_genotypes may come after a stream has run bound batches: a rows-mode event list at top 1 sizes the key scratch
    for two words per read, the codes-mode list behind it needs 1 + 64 -- the scratch has to grow with the key"""
    from sketchy_amd import api
    refs, bases, offsets, _ = three()
    nf = 64
    codes = np.random.default_rng(23).integers(0, 3, size=(sum(SIZES), nf), dtype=np.uint32)
    idx, sm, cum = oracle_rows(refs, bases, offsets, 1)
    cons = consensus_ref(idx, codes, SIZES)
    cuts = [0, 120, 240]
    for entry in ("push", "push_device"):
        R = api.ReferenceSketch([r["ref"] for r in refs], [r["col_len"] for r in refs])  # (a reference of its own: no table yet)
        S = _stream(R, 1, 120, len(bases))
        first = drive(S, entry, bases, offsets, cuts[:2], 1, 3, cap=120)
        check(first, cuts[:2], idx, sm, cap=120, what=entry + " rows mode, no table yet")
        R.set_genotypes(codes)
        second = drive(S, entry, bases, offsets, cuts[1:], 1, 3, nf, codes=True, cap=120, codes_mode=True)
        check(second, cuts[1:], idx, sm, cons, cap=120, codes_mode=True, what=entry + " codes mode, table set since")
        np.testing.assert_array_equal(S.table(), cum)
        S.close()
        R.close()


# ---------------------------------------------------------------- errors
def test_errors_consume_the_binding(gpu):
    from sketchy_amd import _lib, api
    L = _lib.load()
    refs, bases, offsets, _ = three()
    R = api.ReferenceSketch([r["ref"] for r in refs], [r["col_len"] for r in refs])  # no genotype table
    n = 40
    o = np.ascontiguousarray(offsets[:n + 1])
    sp, cc = np.full(n, 7, np.uint32), np.full((n, N_FEAT), 7, np.uint32)
    n_ev, rd, esp = np.full(1, 7, np.uint32), np.full(n, 7, np.uint32), np.full(n, 7, np.uint32)
    S = _stream(R, 2, n, int(o[-1]))
    plain = S.push(bases, o)
    for bind in (lambda: S.bind_call(_p(sp), None, None, _p(cc)),
                 lambda: S.bind_call_changes(n, _p(n_ev), _p(rd), _p(esp), None, None, _p(cc))):
        S.reset()
        bind()
        with pytest.raises(_lib.SketchyHipError) as e:
            S.push(bases, o)
        assert e.value.code == _lib.ERR_INVALID and "genotype table" in str(e.value) and S.reads == 0
        again = S.push(bases, o)  # the binding is gone: an ordinary push
        np.testing.assert_array_equal(again["topk_idx"], plain["topk_idx"])
        assert (sp == 7).all() and (cc == 7).all() and n_ev[0] == 7
    d_b, d_o = api.DeviceBuffer.from_numpy(bases), api.DeviceBuffer.from_numpy(o)
    d_i, d_s, d_sp = api.DeviceBuffer(n * 3 * 2 * 4), api.DeviceBuffer(n * 3 * 2 * 8), api.DeviceBuffer.from_numpy(sp)
    try:
        for fn in (L.skx_stream_push_device, L.skx_stream_enqueue_device):
            for ri, rs in ((None, d_s.ptr), (d_i.ptr, None), (None, None)):
                S.bind_call(d_sp.ptr)
                assert fn(S._h, d_b.ptr, d_o.ptr, n, int(o[-1]), ri, rs) == _lib.ERR_INVALID
                assert "d_topk_idx or d_topk_sum" in L.skx_last_error().decode()
        S.reset()
        S.push_device(d_b.ptr, d_o.ptr, n, int(o[-1]), d_i.ptr, d_s.ptr)  # unbound now
        S.sync()
        assert (d_sp.to_numpy(np.uint32, n) == 7).all()
        np.testing.assert_array_equal(d_i.to_numpy(np.uint32, (n, 3, 2)), plain["topk_idx"])
        # an empty batch: no events
        d_n = api.DeviceBuffer.from_numpy(n_ev)
        S.push_device(d_b.ptr, d_o.ptr, 0, 0, d_i.ptr, d_s.ptr, call_changes=(n, d_n.ptr, d_sp.ptr, d_sp.ptr))
        S.sync()
        assert d_n.to_numpy(np.uint32, 1)[0] == 0
        d_n.free()
    finally:
        for d in (d_b, d_o, d_i, d_s, d_sp):
            d.free()
    S.bind_call_changes(n, _p(n_ev), _p(rd), _p(esp))
    S.push(bases, o[:1])
    assert n_ev[0] == 0 and (rd == 7).all()
    S.close()
    S0 = api.SumOfSharedHashes(R, top=0, max_batch_reads=n, max_batch_bases=int(o[-1]))
    S0.bind_call(_p(sp))
    with pytest.raises(_lib.SketchyHipError) as e:
        S0.push(bases, o)
    assert e.value.code == _lib.ERR_INVALID and "top_k" in str(e.value)
    S0.push(bases, o)
    assert S0.reads == n and (sp == 7).all()
    S0.close()
    R.close()


# ---------------------------------------------------------------- the CLI with the real library
import os  # noqa: E402
import subprocess  # noqa: E402

BIN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sketchy_amd", "sketchy-hip")
COLUMNS = ("mlst", "mlst\tmeca", "st\tmec\tpvl")  # the three tables have different columns


def _cli(*args):
    p = subprocess.run([BIN, *args], capture_output=True)
    return p.returncode, p.stdout.decode(), p.stderr.decode()


@pytest.fixture(scope="module")
def cli_files(gpu, tmp_path_factory):
    from mshio import write_msh
    d = tmp_path_factory.mktemp("call_cli")
    refs, bases, offsets, _ = three()
    msh, tsv = [], []
    for i, r in enumerate(refs):
        names = [f"sp{i}_genome{g:03d}.fa" for g in range(r["ref"].shape[0])]
        msh.append(str(d / f"species{i}.msh"))
        tsv.append(str(d / f"species{i}.tsv"))
        write_msh(msh[-1], names, r["ref"], kmer=K_MER, seed=SEED, lengths=[90000] * len(names))
        with open(tsv[-1], "w") as f:
            f.write("id\t" + COLUMNS[i] + "\n")
            for g, nm in enumerate(names):
                f.write(nm + "\t" + "\t".join(f"{c}{(g * (j + 2)) % (3 + j)}" for j, c in enumerate(COLUMNS[i].split("\t"))) + "\n")
    fq = str(d / "reads.fq")
    with open(fq, "w") as f:
        for i, r in enumerate(unpack_reads(bases, offsets)):
            f.write(f"@r{i}\n{r.decode()}\n+\n{'I' * len(r)}\n")
    return msh, tsv, fq


def _blocks(text, top, n_header=0):
    lines = text.splitlines(keepends=True)
    head, lines = lines[:n_header], lines[n_header:]
    assert len(lines) % top == 0
    return head, [lines[i:i + top] for i in range(0, len(lines), top)]


def _without_species(block):
    return [ln.split("\t", 2)[0] + "\t" + ln.split("\t", 2)[2] for ln in block]


def _called(single_rows):
    """per read the lowest species whose first row has the largest shared_hashes column, from the single-reference runs' blocks"""
    lead = np.array([[int(b[0].split("\t")[2]) for b in blocks] for blocks in single_rows])  # [species, read]
    return np.argmax(lead, axis=0)


def filter_call_changes(text, top, n_header):
    """tests/test_changes_cpu.py::filter_changes for the multi-reference format: keyed on everything but the read number and the sum"""
    head, blocks = _blocks(text, top, n_header)
    out, prev = list(head), None
    for b in blocks:
        key = [ln.split("\t")[1:3] + ln.split("\t")[4:] for ln in b]
        if key != prev:
            out += b
        prev = key
    return "".join(out)


@functools.lru_cache(maxsize=None)
def _single_runs(files, stream):
    """one run per reference file, rows and consensus: what a user without the call does"""
    msh, tsv, fq = files
    mode = ("-s", "-b", "50") if stream else ()
    rows, cons, heads = [], [], []
    for m, t in zip(msh, tsv):
        rc, out, err = _cli("predict", "-r", m, "-g", t, "-i", fq, "-t", "3", "-H", *mode)
        assert rc == 0, err
        head, blocks = _blocks(out, 3, 1)
        rows.append(blocks)
        heads.append(head[0])
        rc, out, err = _cli("predict", "-r", m, "-g", t, "-i", fq, "-t", "3", "-c", *mode)
        assert rc == 0, err
        cons.append(_blocks(out, 1)[1])
    return rows, cons, heads


@pytest.fixture(scope="module")
def single_stream(cli_files):
    return _single_runs(tuple(tuple(x) if isinstance(x, list) else x for x in cli_files), True)


@pytest.fixture(scope="module")
def single_offline(cli_files):
    return _single_runs(tuple(tuple(x) if isinstance(x, list) else x for x in cli_files), False)


SPECIES_NAMES = [f"species{i}" for i in range(3)]


def _agree(cli_files, single, mode, n):
    msh, tsv, fq = cli_files
    single_rows, single_cons, heads = single
    assert all(len(b) == n for b in single_rows)
    called = _called(single_rows)
    rc, multi, err = _cli("predict", "-r", *msh, "-g", *tsv, "-i", fq, "-t", "3", "-H", *mode)
    assert rc == 0, err
    head, blocks = _blocks(multi, 3, 3)
    assert head == [h.replace("reads\t", f"reads\t{sp}\t", 1) for h, sp in zip(heads, SPECIES_NAMES)]
    assert len(blocks) == n
    for r, b in enumerate(blocks):
        assert all(ln.split("\t")[1] == SPECIES_NAMES[called[r]] for ln in b), r
        assert _without_species(b) == single_rows[called[r]][r], r
    rc, cons, err = _cli("predict", "-g", *tsv, "-r", *msh, "-i", fq, "-t", "3", "-c", *mode)
    assert rc == 0, err
    _, cblocks = _blocks(cons, 1)
    assert len(cblocks) == n
    for r, b in enumerate(cblocks):
        assert b[0].split("\t")[1] == SPECIES_NAMES[called[r]] and _without_species(b) == single_cons[called[r]][r], r
    return called, multi, cons


def test_cli_stream_prints_the_called_species_run(cli_files, single_stream):
    undefined = subprocess.check_output(["nm", "-D", "--undefined-only", BIN], text=True)
    for name in ("skx_ref_create_multi", "skx_stream_bind_call", "skx_stream_bind_call_changes", "skx_call_rows"):
        assert name in undefined
    called, multi, cons = _agree(cli_files, single_stream, ("-s", "-b", "50"), 240)
    assert len(set(called.tolist())) >= 2 and (called[1:] != called[:-1]).sum() >= 2
    msh, tsv, fq = cli_files
    rc, got, err = _cli("predict", "-r", *msh, "-g", *tsv, "-i", fq, "-t", "3", "-s", "-l", "77", "-b", "50")
    assert rc == 0 and got == "".join(multi.splitlines(keepends=True)[3:3 + 77 * 3]), err


def test_cli_offline_prints_the_called_species_run(cli_files, single_offline):
    _agree(cli_files, single_offline, (), 1)


@pytest.mark.parametrize("args,top,nh", ((("-H",), 3, 3), (("-c",), 1, 0)), ids=("rows", "consensus"))
def test_cli_changes_prints_the_filtered_call(cli_files, args, top, nh):
    msh, tsv, fq = cli_files
    base = ("predict", "-r", *msh, "-g", *tsv, "-i", fq, "-t", "3", "-s", *args)
    rc, text, err = _cli(*base, "-b", "50")
    assert rc == 0, err
    want = filter_call_changes(text, top, nh)
    assert want.count("\n") < text.count("\n")
    for b in ("50", "7", "100000"):  # batches that begin inside runs and at their starts; one batch
        rc, got, err = _cli(*base, "-b", b, "--changes")
        assert rc == 0, err
        assert got == want, (args, b)


def test_cli_several_references_usage_errors(cli_files, tmp_path):
    from mshio import write_msh
    msh, tsv, fq = cli_files
    refs = three()[0]
    rc, out, err = _cli("predict", "-r", *msh, "-g", *tsv[:2], "-i", fq, "-s")
    assert rc == 2 and out == "" and "-g" in err and "-r" in err
    rc, out, err = _cli("predict", "-r", *msh, "-g", *tsv, "-i", fq, "-s", "-t", "131")  # the smallest file holds 130 sketches
    assert rc == 2 and out == "" and "--top" in err
    other = str(tmp_path / "k15.msh")
    names = [f"sp0_genome{g:03d}.fa" for g in range(130)]
    write_msh(other, names, refs[0]["ref"], kmer=15, seed=SEED, lengths=[90000] * 130)
    rc, out, err = _cli("predict", "-r", other, msh[1], "-g", tsv[0], tsv[1], "-i", fq, "-s")
    assert rc == 2 and out == "" and other in err and msh[1] in err
