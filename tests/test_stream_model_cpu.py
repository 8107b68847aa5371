"""tests/stream_model.py without a device: the model against the restatements it does not use itself, and what the committed walks of
tests/test_gpu_walks.py must contain -- computed from the plans and the model alone."""
import functools

import numpy as np
import pytest

import depth_cases as dc
import stream_model as sm
from call_cases import call_changes_ref, call_ref
from oracle import oracle as orc
from test_changes_cpu import changes_ref
from test_gpu_bound_outputs import PASS_ROWS
from test_gpu_call import consensus_ref

DEPTH_QUERIES = ("depth", "depth_rows", "depth_count", "depth_export")


@functools.lru_cache(maxsize=None)
def committed(world):
    """[(seed, ops, trace)] of the world's committed walks (default seed base)"""
    out = []
    for seed in sm.seeds(world):
        ops = sm.plan(world, seed)
        out.append((seed, ops, sm.trace(world, ops)))
    return out


# ---------------------------------------------------------------------------------------------------------------- the plans
@pytest.mark.parametrize("world", sm.WORLDS)
def test_plans_are_deterministic_literals_within_their_limits(world):
    for seed, ops, _ in committed(world):
        assert ops == sm.plan(world, seed)
        assert eval(repr(ops)) == ops, "a plan must print as a Python literal"
        assert len(ops) <= 40 and sum(op["m"] for op in ops if op["op"] == "batch") <= 1500
        assert [op["op"] for op in ops[-3:]] == ["sync", "table", "reads"] and ops[0]["op"] == "create"


def _applicable(world, seed, ops):
    """the rules of stream_model's docstring, tracked here once more: tickets out, enqueued batches not yet flushed (a refused batch
    flushes nothing, whatever its entry point), what is enabled, reads left"""
    W = sm.world_of(world, ops[0])
    out, dev_pending, pos, stat = 0, False, 0, ops[0]["stat"]
    for i, op in enumerate(ops[1:], 1):
        kind, entry = op["op"], op.get("entry")
        w = f"seed {seed} op {i} {op}"
        if entry == "submit":
            assert not dev_pending, w
        elif kind not in ("wait", "drain", "flush"):
            assert out == 0, w
        if kind == "wait":
            assert out > 0, w
        if kind.startswith("coverage"):
            assert stat in ("coverage", "depth"), w
        if kind.startswith("depth"):
            assert stat == "depth", w
        if kind == "batch":
            pos += op["m"]
            assert op["m"] in sm.SIZES_OF_A_BATCH and pos <= W.n_reads, w
            assert not (op["null_rows"] and op["bind"] and entry in ("enqueue_device", "push_device")), w
        if kind == "batch" and entry == "submit":
            out += 1
        elif kind == "batch" and entry in ("enqueue_device", "push_device"):
            dev_pending = True
        elif kind == "drain":
            out, dev_pending = 0, False
        elif kind not in ("reads", "wait", "refuse"):
            dev_pending = False


@pytest.mark.parametrize("world", sm.WORLDS)
def test_plans_emit_only_applicable_ops(world):
    """the runner executes every op as it stands: whatever an op needs in front of it must be in the plan"""
    for seed, ops, _ in committed(world):
        _applicable(world, seed, ops)


@pytest.mark.parametrize("world", ("classes", "species"))
def test_plans_of_other_seed_bases_emit_only_applicable_ops(world):
    """SKX_TEST_SEED selects other walks: their plans keep the same rules (the two worlds whose plans cost nothing to draw)"""
    met = 0
    for base in range(1, 41):
        for seed in sm.seeds(world, base):
            ops = sm.plan(world, seed)
            assert len(ops) <= 40
            _applicable(world, seed, ops)
            # the sequence a refusal must not break: enqueued batches, a refused push, and the flush in front of the submit behind it
            met += sum(1 for a, b, c, d in zip(ops[1:], ops[2:], ops[3:], ops[4:])
                       if a["op"] == "batch" and a["entry"] == "enqueue_device" and (b["op"], b.get("entry")) == ("refuse", "push")
                       and c["op"] == "flush" and d.get("entry") == "submit")
    assert met > 0, "the scan never met a refused push between enqueued batches and a submit"


# ---------------------------------------------------------------------------------------------------------------- the model
def _unchained(W, top, n):
    outs = [orc.stream(sm.K_MER, sm.SEED, W.s, r, c, W.bases, W.offsets[:n + 1], top_k=top) for r, c in zip(W.refs, W.col_lens)]
    idx = np.stack([o["topk_idx"] for o in outs], axis=1).astype(np.uint32)
    sums = np.stack([o["topk_sum"] for o in outs], axis=1).astype(np.uint64)
    return idx, sums, np.concatenate([o["cum"] for o in outs]), consensus_ref(idx, W.codes, W.sizes)


@pytest.mark.parametrize("world", sm.WORLDS)
def test_model_against_one_unchained_oracle_run(world):
    """two short plans without reset, table_add and depth_import: the model chains the oracle batch by batch; here one oracle run over all
    reads is cut at the batches, and the depth figures come from depth_cases.expected_depth"""
    for seed in (11, 12):
        ops = sm.plan(world, seed, max_ops=16, max_reads=260, exclude=("reset", "table_add", "depth_import"))
        W = sm.world_of(world, ops[0])
        tr = sm.trace(world, ops)
        n = sum(op["m"] for op in ops if op["op"] == "batch")
        assert n > 0
        idx, sums, cum, cons = _unchained(W, ops[0]["top"], n)
        at = sorted({0, n} | {e["first"] + e["m"] for op, e in tr if op["op"] == "batch"})
        depth = dc.expected_depth(W.refs, W.col_lens, W.bases, W.offsets, W.s, at)
        pos = 0
        for op, e in tr:
            w = f"{world} seed {seed} {op}"
            if op["op"] == "batch":
                a, b = pos, pos + op["m"]
                assert e["first"] == a
                np.testing.assert_array_equal(e["rows_idx"], idx[a:b], err_msg=w)
                np.testing.assert_array_equal(e["rows_sum"], sums[a:b], err_msg=w)
                np.testing.assert_array_equal(e["cons"], cons[a:b], err_msg=w)
                want = call_ref(idx[a:b], sums[a:b], cons[a:b])
                for k, k2 in (("call_sp", "call_species"), ("call_idx", "call_idx"), ("call_sum", "call_sum"), ("call_codes", "call_codes")):
                    np.testing.assert_array_equal(e[k], want[k2], err_msg=w)
                np.testing.assert_array_equal(e["chg_ev"]["rows"], changes_ref(idx[a:b]), err_msg=w)
                np.testing.assert_array_equal(e["chg_ev"]["codes"], changes_ref(cons[a:b]), err_msg=w)
                np.testing.assert_array_equal(e["cev_ev"]["rows"], call_changes_ref(want["call_species"], want["call_idx"]), err_msg=w)
                np.testing.assert_array_equal(e["cev_ev"]["codes"], call_changes_ref(want["call_species"], want["call_codes"]), err_msg=w)
                pos = b
            elif op["op"] in ("depth", "depth_rows", "coverage", "coverage_rows"):
                rows = np.asarray(op.get("rows", np.arange(W.n_genomes)), np.int64)
                for name, want in zip(("covered", "median", "total"), depth[pos]):
                    if name in e:
                        np.testing.assert_array_equal(e[name], want[rows], err_msg=f"{w} {name}")
            elif op["op"] == "reads":
                assert e["reads"] == pos
        np.testing.assert_array_equal(tr[-2][1]["table"], cum)
        np.testing.assert_array_equal(depth[n][2], cum)  # (nothing imported, nothing saturated: total is the table)


# ---------------------------------------------------------------------------------------------------------------- the committed walks
def conditions():
    """what the committed walks contain: name -> count"""
    c = dict.fromkeys(("truncated_chg", "truncated_cev", "species_flip_in_bound_batch", "query_behind_enqueue", "bind_with_ticket_out",
                       "reset_then_batches_then_depth_query", "import_behind_reset", "led_by_add", "refused_with_bindings",
                       "bound_batch_of_several_passes", "bound_walk_with_adjacent_enqueues"), 0)
    kinds, carried = {}, set()
    for world in sm.WORLDS:
        for seed, ops, tr in committed(world):
            out, since_reset, bound_walk, adjacent = set(), None, False, False
            for i, (op, e) in enumerate(tr):
                kind, entry, bind = op["op"], op.get("entry"), op.get("bind", {})
                name = f"{kind}:{entry}" if kind == "batch" else kind
                kinds[name] = kinds.get(name, 0) + 1
                prev = ops[i - 1] if i else {}
                if kind == "batch":
                    bound_walk = bound_walk or bool(bind)
                    carried |= {(entry, b) for b in sm.BINDINGS if bind.get(b)}
                    c["truncated_chg"] += bool(bind.get("chg")) and len(e["chg_ev"]["codes" if bind["chg_codes"] else "rows"]) > bind["chg"]
                    c["truncated_cev"] += bool(bind.get("cev")) and len(e["cev_ev"]["codes" if bind["cev_codes"] else "rows"]) > bind["cev"]
                    if world == "species" and (bind.get("call") or bind.get("cev")) and len(set(e["call_sp"].tolist())) > 1:
                        c["species_flip_in_bound_batch"] += 1
                    if world == "species" and bind and op.get("stats") and ops[0]["query_rows"] == 64 and e["distinct_held"] > PASS_ROWS:
                        c["bound_batch_of_several_passes"] += 1
                    if entry == "enqueue_device" and prev.get("op") == "batch" and prev.get("entry") == "enqueue_device" and ops[0]["coalesce"] >= 2:
                        adjacent = True
                    c["led_by_add"] += bool(e.get("led_by_add"))
                    if since_reset == "reset":
                        since_reset = "batches"
                if kind in sm.QUERIES and prev.get("op") == "batch" and prev.get("entry") == "enqueue_device":
                    c["query_behind_enqueue"] += 1
                if kind in ("batch", "refuse") and entry == "submit" and bind and out:   # (tickets issued and neither waited for nor drained)
                    c["bind_with_ticket_out"] += 1
                if kind == "refuse" and bind:
                    c["refused_with_bindings"] += 1
                if kind == "reset":
                    since_reset = "reset"
                if kind in DEPTH_QUERIES and since_reset == "batches":
                    c["reset_then_batches_then_depth_query"] += 1
                    since_reset = None
                if kind == "depth_import" and since_reset == "reset":
                    c["import_behind_reset"] += 1
                if kind == "batch" and entry == "submit":
                    out.add(e["ticket"])
                elif kind == "wait":
                    out.discard(op["ticket"])
                elif kind == "drain":
                    out.clear()
            c["bound_walk_with_adjacent_enqueues"] += bound_walk and adjacent
    return c, kinds, carried


def test_committed_walks_hold_what_the_walks_are_for():
    c, kinds, carried = conditions()
    every = [f"batch:{e}" for e in sm.ENTRIES] + [k for k in sm.WEIGHTS if k != "batch"]
    assert set(every) - {"batch:" + e for e in sm.ENTRIES} == set(sm.QUERIES) | {"refuse", "depth_import", "table_add", "reset", "packed", "flush",
                                                                                "sync", "wait", "drain"}
    assert not [k for k in every if kinds.get(k, 0) < 2], {k: kinds.get(k, 0) for k in every}
    assert not [(e, b) for e in sm.ENTRIES for b in sm.BINDINGS if (e, b) not in carried], sorted(carried)
    assert not [k for k, v in c.items() if v < 1], c
