"""The bound outputs of a batch -- consensus codes, change list, species call and the call's change list -- travel as ONE record
(sketchy_amd/csrc/skx_batch_out.hpp) through every batch entry point.  What one path for all of them could break and the tests of
the single bindings leave out: all four through skx_stream_push_device, all four on a batch cut into passes, bindings that come,
grow and go from ticket to ticket on the staging slots of skx_stream_submit and on the shared passes of skx_stream_enqueue_device,
and a stream that never binds.  Workload, driver and restatements are tests/test_gpu_call.py's; every expected value comes from the
CPU oracle's rows."""
import ctypes as C
import functools

import numpy as np
import pytest

from call_cases import call_changes_ref, call_ref
from helpers import unpack_reads, workload_species
from oracle import oracle as orc
from test_changes_cpu import changes_ref
from test_gpu_call import (K_MER, N_FEAT, SEED, SENT, SIZES, Mem, _stream, check, consensus_ref, drive, oracle_rows, three, three_expected,
                           three_ref, untouched)  # noqa: F401  (three_ref: the module's fixture)

pytestmark = pytest.mark.gpu

TOP, N_SP = 3, 3


def check_all_four(got, cuts, idx, sm, cons, cap, codes_mode, what):
    """drive(..., also=True)'s batches: the call and its list (check), the consensus output and the change list of the full rows"""
    total = check(got, cuts, idx, sm, cons, cap=cap, codes_mode=codes_mode, what=what)
    for g, a, b in zip(got, cuts[:-1], cuts[1:]):
        np.testing.assert_array_equal(g["cons"], cons[a:b], err_msg=what)
        ev = changes_ref(idx[a:b])
        assert int(g["chg_n"][0]) == len(ev), what
        np.testing.assert_array_equal(g["chg_read"][:len(ev)], ev, err_msg=what)
        np.testing.assert_array_equal(g["chg_idx"][:len(ev)], idx[a:b][ev], err_msg=what)
        np.testing.assert_array_equal(g["chg_sum"][:len(ev)], sm[a:b][ev], err_msg=what)
        for k in ("chg_read", "chg_idx", "chg_sum"):
            assert (g[k][len(ev):] == SENT[g[k].dtype]).all(), f"{what}: {k} past n_events was written"
    return total


@pytest.mark.parametrize("codes_mode", (False, True), ids=("rows", "codes"))
def test_all_four_bindings_through_push_device(three_ref, codes_mode):
    refs, bases, offsets, _ = three()
    idx, sm, cum, cons = three_expected(TOP)
    cuts = [0, 90, 170, 240]
    S = _stream(three_ref, TOP, 90, len(bases))
    got = drive(S, "push_device", bases, offsets, cuts, TOP, N_SP, N_FEAT, codes=True, cap=90, codes_mode=codes_mode, also=True)
    assert check_all_four(got, cuts, idx, sm, cons, 90, codes_mode, "push_device") > 3
    np.testing.assert_array_equal(S.table(), cum)
    S.close()


# ---------------------------------------------------------------- one batch, several passes
QUERY_ROWS = 64
# The bit matrices of a pass have max(stream_query_rows, s) rows, rounded up to 64 -- one read alone must fit, and a read's sketch
# has s = 300 hashes -- one row per DISTINCT hash of the pass's reads that some genome holds.  The 240 reads hold 250 such hashes:
# one pass at any value of the option.  This case therefore takes 720 reads of the same generator over the same three references.
PASS_ROWS = (max(QUERY_ROWS, 300) + 63) // 64 * 64
N_MORE = 720


@functools.lru_cache(maxsize=None)
def more_reads():
    refs, _, _, codes = three()
    refs2, bases, offsets = workload_species(list(SIZES), 300, N_MORE, read_len=800, genome_len=90000, rng_seed=201)
    assert all(np.array_equal(a["ref"], b["ref"]) and np.array_equal(a["col_len"], b["col_len"]) for a, b in zip(refs, refs2))
    held = np.unique(np.concatenate([r["ref"].ravel() for r in refs]))
    sketches = np.concatenate([orc.sketch(rd, K_MER, SEED, 300) for rd in unpack_reads(bases, offsets)])
    distinct = len(np.unique(sketches[np.isin(sketches, held)]))
    idx, sm, cum = oracle_rows(refs, bases, offsets, TOP)
    return bases, offsets, distinct, idx, sm, cum, consensus_ref(idx, codes, SIZES)


@pytest.mark.parametrize("entry", ("push", "push_device"))
def test_all_four_bindings_on_a_batch_cut_into_passes(three_ref, entry):
    """every pass votes, selects and flags its own reads (the first read of a later pass against the last of the pass before); the
    scans and the gathers of both lists come once, behind the batch's last pass"""
    from sketchy_amd import api
    bases, offsets, distinct, idx, sm, cum, cons = more_reads()
    assert distinct > PASS_ROWS, distinct  # (the oracle's sketches: more distinct hashes than one pass has rows)
    n = len(offsets) - 1
    before = api.get_option("stream_query_rows")
    try:
        api.set_option("stream_query_rows", QUERY_ROWS)
        S = _stream(three_ref, TOP, n, len(bases))
    finally:
        api.set_option("stream_query_rows", before)
    for codes_mode in (False, True):
        S.reset()
        got = drive(S, entry, bases, offsets, [0, n], TOP, N_SP, N_FEAT, codes=True, cap=n, codes_mode=codes_mode, also=True)
        assert S.stats()["last_passes"] > 1, S.stats()
        assert check_all_four(got, [0, n], idx, sm, cons, n, codes_mode, f"{entry} codes_mode {codes_mode}") > 3
        np.testing.assert_array_equal(S.table(), cum)
    S.close()


# ---------------------------------------------------------------- bindings that change from batch to batch
ALL_ROWS = dict(cons=True, chg=30, call=True, cev=30)
ALL_CODES = dict(cons=True, chg=30, chg_codes=True, call=True, call_codes=True, cev=30, cev_codes=True)
# What one staging slot of a submitting stream sees, ticket after ticket: caps that grow, codes that arrive late, bindings that
# disappear.  Ticket t uses slot t % n_slots, so the plan of a stream is laid out from its slot count (plans_for).
SLOT_SEQ = ((dict(), dict(call=True), dict(cev=4, cev_codes=True)),
            (dict(chg=4), dict(chg=30, chg_codes=True), ALL_CODES),
            (ALL_ROWS, dict(), dict(chg=4, chg_codes=True, cons=True)))


def staging_slots(coalesce):
    """skx_stream_submit's rule: three slots, 2 n + 1 when groups of n <= 4 batches share a pass"""
    return 3 if coalesce < 2 else 2 * min(coalesce, 4) + 1


def plans_for(n_slots, rounds=3):
    return tuple(SLOT_SEQ[(t % n_slots) % len(SLOT_SEQ)][t // n_slots] for t in range(rounds * n_slots))


PLANS = plans_for(3)
GROUPS = dict(cons=("cons",), chg=("chg_n", "chg_read", "chg_idx", "chg_sum", "chg_codes"),
              call=("call_sp", "call_idx", "call_sum", "call_codes"), cev=("cev_n", "cev_read", "cev_sp", "cev_idx", "cev_sum", "cev_codes"))


def run_plans(S, entry, bases, offsets, cuts, plans):
    """drive() with bindings of its own for every batch: each batch gets every array, sentinel-filled and sized for the whole batch,
    and binds what its plan names"""
    from sketchy_amd import api
    kind = "pinned" if entry == "submit" else "device"
    mems, extra = [], []
    try:
        if kind == "pinned":
            hb, ho = api.HostBuffer(max(len(bases), 8)), api.HostBuffer(len(offsets) * 8)
            hb.view(np.uint8, len(bases))[:] = bases
            ho.view(np.uint64, len(offsets))[:] = offsets
            extra += [hb, ho]
        else:
            d_b = api.DeviceBuffer.from_numpy(bases)
            extra.append(d_b)
        for plan, a, b in zip(plans, cuts[:-1], cuts[1:]):
            n = b - a
            spec = dict(rows_idx=((n, N_SP, TOP), np.uint32), rows_sum=((n, N_SP, TOP), np.uint64), cons=((n, N_SP, N_FEAT), np.uint32),
                        chg_n=((1,), np.uint32), chg_read=((n,), np.uint32), chg_idx=((n, N_SP, TOP), np.uint32),
                        chg_sum=((n, N_SP, TOP), np.uint64), chg_codes=((n, N_SP, N_FEAT), np.uint32),
                        call_sp=((n,), np.uint32), call_idx=((n, TOP), np.uint32), call_sum=((n, TOP), np.uint64), call_codes=((n, N_FEAT), np.uint32),
                        cev_n=((1,), np.uint32), cev_read=((n,), np.uint32), cev_sp=((n,), np.uint32), cev_idx=((n, TOP), np.uint32),
                        cev_sum=((n, TOP), np.uint64), cev_codes=((n, N_FEAT), np.uint32))
            M = Mem(kind, spec)
            mems.append(M)
            q = M.ptr
            if plan.get("cons"):
                S.bind_consensus(q("cons"))
            if plan.get("chg"):
                S.bind_changes(plan["chg"], q("chg_n"), q("chg_read"), q("chg_idx"), q("chg_sum"), q("chg_codes") if plan.get("chg_codes") else None)
            if plan.get("call"):
                S.bind_call(q("call_sp"), q("call_idx"), q("call_sum"), q("call_codes") if plan.get("call_codes") else None)
            if plan.get("cev"):
                S.bind_call_changes(plan["cev"], q("cev_n"), q("cev_read"), q("cev_sp"), q("cev_idx"), q("cev_sum"),
                                    q("cev_codes") if plan.get("cev_codes") else None)
            if entry == "submit":
                S.submit(hb.ptr, C.c_void_p(ho.ptr.value + a * 8), n, q("rows_idx"), q("rows_sum"))
            else:
                d_o = api.DeviceBuffer.from_numpy(np.ascontiguousarray(offsets[a:b + 1], np.uint64))
                extra.append(d_o)
                fn = S.enqueue_device if entry == "enqueue_device" else S.push_device
                fn(d_b.ptr, d_o.ptr, n, int(offsets[b] - offsets[a]), q("rows_idx"), q("rows_sum"))
        if entry == "submit":
            S.drain()
        else:
            S.sync()
        return [M.read() for M in mems]
    finally:
        for x in extra + mems:
            x.free()


def check_events(g, pre, cap, ev, cols, w):
    """one event list of a batch: n_events whatever the cap, the first min(n_events, cap) entries of every bound column, and nothing
    past them; cols: name -> the expected per-read rows (None: not bound)"""
    m = min(len(ev), cap)
    assert int(g[pre + "_n"][0]) == len(ev), w
    np.testing.assert_array_equal(g[pre + "_read"][:m], ev[:m], err_msg=w)
    assert (g[pre + "_read"][m:] == SENT[np.dtype(np.uint32)]).all(), f"{w}: {pre}_read past min(n_events, cap) was written"
    for name, rows in cols.items():
        k = f"{pre}_{name}"
        if rows is None:
            assert untouched(g, (k,)), f"{w}: {k} was not bound"
            continue
        np.testing.assert_array_equal(g[k][:m], rows[ev[:m]], err_msg=f"{w}: {k}")
        assert (g[k][m:] == SENT[g[k].dtype]).all(), f"{w}: {k} past min(n_events, cap) was written"


def check_plans(got, plans, cuts, idx, sm, cons, what):
    seen_truncated = False
    for i, (g, plan, a, b) in enumerate(zip(got, plans, cuts[:-1], cuts[1:])):
        w = f"{what} batch {i} {plan}"
        np.testing.assert_array_equal(g["rows_sum"], sm[a:b], err_msg=w)
        np.testing.assert_array_equal(g["rows_idx"], idx[a:b], err_msg=w)
        for name, cols in GROUPS.items():
            if not plan.get(name):
                assert untouched(g, cols), f"{w}: {name} was not bound"
        want = call_ref(idx[a:b], sm[a:b], cons[a:b])
        if plan.get("cons"):
            np.testing.assert_array_equal(g["cons"], cons[a:b], err_msg=w)
        if plan.get("chg"):
            by_codes = bool(plan.get("chg_codes"))
            ev = changes_ref(cons[a:b] if by_codes else idx[a:b])
            seen_truncated = seen_truncated or len(ev) > plan["chg"]
            check_events(g, "chg", plan["chg"], ev, dict(idx=idx[a:b], sum=sm[a:b], codes=cons[a:b] if by_codes else None), w)
        if plan.get("call"):
            np.testing.assert_array_equal(g["call_sp"], want["call_species"], err_msg=w)
            np.testing.assert_array_equal(g["call_idx"], want["call_idx"], err_msg=w)
            np.testing.assert_array_equal(g["call_sum"], want["call_sum"], err_msg=w)
            if plan.get("call_codes"):
                np.testing.assert_array_equal(g["call_codes"], want["call_codes"], err_msg=w)
            else:
                assert untouched(g, ("call_codes",)), w
        if plan.get("cev"):
            by_codes = bool(plan.get("cev_codes"))
            ev = call_changes_ref(want["call_species"], want["call_codes"] if by_codes else want["call_idx"])
            seen_truncated = seen_truncated or len(ev) > plan["cev"]
            check_events(g, "cev", plan["cev"], ev, dict(sp=want["call_species"], idx=want["call_idx"], sum=want["call_sum"],
                                                        codes=want["call_codes"] if by_codes else None), w)
    assert seen_truncated, "no list of the plan was longer than its cap"


CUTS = [int(x) for x in np.linspace(0, 240, len(PLANS) + 1)]  # nine batches of 26 or 27 reads


def test_submit_more_tickets_than_slots_with_changing_bindings(three_ref):
    """three tickets on each staging slot: every slot's device copies serve a ticket after another one's -- event arrays that grow
    from 4 entries to 30, codes that the slot's first list did not have, and bindings gone again"""
    from sketchy_amd import api
    refs, bases, offsets, _ = three()
    idx, sm, cum, cons = three_expected(TOP)
    before = api.get_option("stream_coalesce")
    try:
        api.set_option("stream_coalesce", 1)
        plans = plans_for(staging_slots(api.get_option("stream_coalesce")))  # (the option the stream is created under)
        S = api.SumOfSharedHashes(three_ref, top=TOP, max_batch_reads=30, max_batch_bases=len(bases))
    finally:
        api.set_option("stream_coalesce", before)
    assert plans == PLANS and len(plans) > staging_slots(1)
    got = run_plans(S, "submit", bases, offsets, CUTS, plans)
    check_plans(got, plans, CUTS, idx, sm, cons, "submit")
    np.testing.assert_array_equal(S.table(), cum)
    S.close()


def test_enqueue_device_bound_and_unbound_batches_share_passes(three_ref):
    refs, bases, offsets, _ = three()
    idx, sm, cum, cons = three_expected(TOP)
    S = _stream(three_ref, TOP, 30, len(bases), coalesce=3)
    got = run_plans(S, "enqueue_device", bases, offsets, CUTS, PLANS)
    assert S.stats()["passes_shared"] >= 1, S.stats()
    check_plans(got, PLANS, CUTS, idx, sm, cons, "enqueue_device")
    np.testing.assert_array_equal(S.table(), cum)
    S.close()


# ---------------------------------------------------------------- the change list compared by codes
@pytest.mark.parametrize("cons", (False, True), ids=("lane_scratch", "consensus_output"))
def test_codes_mode_change_list_through_push_device(three_ref, cons):
    """the list of the full rows compared by their voted codes, alone (the vote goes to the ranking lane's scratch) and with a
    consensus output travelling along (the vote is the output's), beside the call with codes"""
    refs, bases, offsets, _ = three()
    idx, sm, cum, codes = three_expected(TOP)
    cuts = [0, 90, 170, 240]
    plans = (dict(chg=90, chg_codes=True, cons=cons), dict(chg=4, chg_codes=True, cons=cons, call=True, call_codes=True),
             dict(chg=90, chg_codes=True, cons=cons, cev=90, cev_codes=True))
    S = _stream(three_ref, TOP, 90, len(bases))
    got = run_plans(S, "push_device", bases, offsets, cuts, plans)
    check_plans(got, plans, cuts, idx, sm, codes, "push_device")
    np.testing.assert_array_equal(S.table(), cum)
    S.close()


@pytest.mark.parametrize("cons", (False, True), ids=("lane_scratch", "consensus_output"))
def test_codes_mode_change_list_on_a_batch_cut_into_passes(three_ref, cons):
    """the first read of a later pass compares its codes with the codes the pass before voted: into the lane's scratch, or into the
    consensus output"""
    from sketchy_amd import api
    bases, offsets, distinct, idx, sm, cum, codes = more_reads()
    assert distinct > PASS_ROWS, distinct
    n = len(offsets) - 1
    before = api.get_option("stream_query_rows")
    try:
        api.set_option("stream_query_rows", QUERY_ROWS)
        S = _stream(three_ref, TOP, n, len(bases))
    finally:
        api.set_option("stream_query_rows", before)
    plans = (dict(chg=n, chg_codes=True, cons=cons),)
    got = run_plans(S, "push_device", bases, offsets, [0, n], plans)
    assert S.stats()["last_passes"] > 1, S.stats()
    ev = changes_ref(codes)
    assert 3 < len(ev) < n and int(got[0]["chg_n"][0]) == len(ev)
    check_events(got[0], "chg", n, ev, dict(idx=idx, sum=sm, codes=codes), "several passes")
    np.testing.assert_array_equal(got[0]["rows_idx"], idx)
    if cons:
        np.testing.assert_array_equal(got[0]["cons"], codes)
    np.testing.assert_array_equal(S.table(), cum)
    S.close()


# ---------------------------------------------------------------- nothing bound
@pytest.mark.parametrize("entry", ("push", "push_device", "enqueue_device", "submit"))
def test_a_stream_that_never_binds(three_ref, entry):
    """the path the benchmark times: the oracle's rows and table, and no bound output written anywhere"""
    refs, bases, offsets, _ = three()
    idx, sm, cum, cons = three_expected(TOP)
    cuts = [0, 90, 170, 240]
    S = _stream(three_ref, TOP, 90, len(bases), coalesce=3)
    got = drive(S, entry, bases, offsets, cuts, TOP, N_SP, N_FEAT, call=False, codes=True, also=True, bound=())
    for g, a, b in zip(got, cuts[:-1], cuts[1:]):
        np.testing.assert_array_equal(g["rows_sum"], sm[a:b], err_msg=entry)
        np.testing.assert_array_equal(g["rows_idx"], idx[a:b], err_msg=entry)
        assert untouched(g, ("cons", "chg_n", "chg_read", "chg_idx", "chg_sum", "call_sp", "call_idx", "call_sum", "call_codes")), entry
    np.testing.assert_array_equal(S.table(), cum)
    S.close()
