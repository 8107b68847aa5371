"""Random walks over the WHOLE stream API, as a plan, a CPU model and a runner (tests/test_stream_model_cpu.py, tests/test_gpu_walks.py).

  plan(world, seed)    a list of ops (plain dicts; op 0 creates the stream).  The generator tracks what it needs to emit only ops that
                       are applicable -- reads left, tickets outstanding, enqueued batches not yet flushed, packed or not, what is
                       enabled -- and writes the drains and flushes an op needs in front of it as ops of their own: nothing is skipped
                       or added when the plan is executed.
  Model(world, create) the CPU state that consumes the same ops and yields, per op, everything the device must return.  Only the oracle
                       (orc.sketch once per read, orc.stream chained through `cum` batch by batch) and the restatements the single-feature
                       tests use: consensus_ref, changes_ref, call_ref, call_changes_ref, depth_cases.depth_matrix / summarise /
                       reference_pairs, coverage_cases.expected_rank.
  run / replay         execute a plan on the device against the model.  On a failure the world, the seed, the index of the failing op and
                       the ops so far are printed as a Python literal; replay(world, ops) runs such a literal.

What has to be drained or flushed in front of an op (include/sketchy_hip.h; where it is silent, the rule of tests/test_gpu_fuzz.py):
  * submitted batches are not interleaved with anything but submit / wait / flush without a drain in between (header: push and
    push_device; set_packed_input refuses; the old walk drains in front of every other op as well, queries included);
  * a flush in front of a submit that follows enqueued or device-pushed batches (the old walk);
  * everything else flushes by itself (header, skx_stream_enqueue_device).
Outputs are read where the header says they are there: a push's when it returns, a ticket's after wait(ticket) or drain, a device
batch's after skx_stream_sync.

The library is imported on use only: plan and Model run without a device."""
import functools
import time

import numpy as np

import coverage_cases as cc
import depth_cases as dc
import hash_classes as hc
from call_cases import call_changes_ref, call_ref
from helpers import unpack_reads, workload_snp
from oracle import oracle as orc
from test_changes_cpu import changes_ref
from test_gpu_call import SENT, Mem, consensus_ref, three

K_MER, SEED = 16, 0
N_FEAT = 4
MAX_BATCH_READS = 400
SIZES_OF_A_BATCH = (1, 7, 64, 65, 120, 240, 400)
WORLDS = ("classes", "species", "tree")
U32_MAX = dc.U32_MAX
ENTRIES = ("enqueue_device", "push_device", "push", "submit")
QUERIES = ("table", "rank", "reads", "coverage", "coverage_rows", "coverage_rank", "depth", "depth_rows", "depth_count", "depth_export")
BINDINGS = ("cons", "chg", "call", "cev")
# the fields of one batch's memory that belong to each binding (run: every batch gets every array, sentinel-filled)
GROUPS = dict(cons=("cons",), chg=("chg_n", "chg_read", "chg_idx", "chg_sum", "chg_codes"),
              call=("call_sp", "call_idx", "call_sum", "call_codes"), cev=("cev_n", "cev_read", "cev_sp", "cev_idx", "cev_sum", "cev_codes"))


# the committed walks: seed = multiplier x base + offset, base = SKX_TEST_SEED (default 5, as tests/test_gpu_fuzz.py).  The offsets are
# chosen so that the conditions of tests/test_stream_model_cpu.py hold for the default base.
SEED_BASE = 5
WALKS = dict(classes=(3000, (1, 2, 7, 15)), species=(4000, (1, 8, 10, 12)), tree=(6000, (4, 6, 8, 10)))


def seeds(world, base=SEED_BASE):
    mult, offsets = WALKS[world]
    return [mult * int(base) + o for o in offsets]


# ---------------------------------------------------------------------------------------------------------------- worlds
class World:
    """refs / col_lens: one [n, stride] uint64 matrix and its lengths per species; s: the size reads are sketched with"""

    def __init__(self, name, key, refs, col_lens, s, bases, offsets, codes, design=None):
        self.name, self.key, self.design = name, key, design
        self.refs = [np.ascontiguousarray(r, np.uint64) for r in refs]
        self.col_lens = [np.ascontiguousarray(c, np.uint32) for c in col_lens]
        self.s, self.bases, self.offsets, self.codes = int(s), bases, offsets, codes
        self.sizes = tuple(int(r.shape[0]) for r in self.refs)
        self.n_genomes, self.n_species, self.n_reads = sum(self.sizes), len(self.sizes), len(offsets) - 1
        self.first = np.concatenate([[0], np.cumsum(self.sizes)[:-1]]).astype(np.int64)
        ref, col_len = np.concatenate(self.refs), np.concatenate(self.col_lens)
        self.held = np.unique(ref[np.arange(ref.shape[1])[None, :] < col_len[:, None]])

    @functools.cached_property
    def sketches(self):
        """per read the hashes of its bottom-s sketch that some genome holds (orc.sketch, once per read), as Python ints"""
        out = []
        for seq in unpack_reads(self.bases, self.offsets):
            sk = orc.sketch(seq, K_MER, SEED, self.s)
            out.append([int(h) for h in sk[np.isin(sk, self.held)]])
        return out


@functools.lru_cache(maxsize=None)
def _world(name, n, read_len, rng_seed):
    if name == "classes":
        design, refs, col_lens, bases, offsets = cc.single(64)
        codes = np.random.default_rng(23).integers(0, 4, size=(hc.N_SINGLE, N_FEAT), dtype=np.uint32)
        return World(name, (name,), refs, col_lens, int(col_lens[0][0]), bases, offsets, codes, design=design)
    if name == "species":
        from test_gpu_bound_outputs import more_reads
        refs, _, _, codes = three()
        bases, offsets = more_reads()[:2]
        return World(name, (name,), [r["ref"] for r in refs], [r["col_len"] for r in refs], 300, bases, offsets, codes)
    assert name == "tree", name
    ref, bases, offsets = workload_snp(n, 300, 1500, read_len=read_len, rng_seed=rng_seed, n_lineages=13)
    codes = np.random.default_rng(29 + n).integers(0, 4, size=(n, N_FEAT), dtype=np.uint32)
    return World(name, (name, n, read_len, rng_seed), [ref["ref"]], [ref["col_len"]], 300, bases, offsets, codes)


def world_of(name, create):
    """the world a plan's first op names (the clone tree is drawn with the stream: its size, read length and generator seed)"""
    if name == "tree":
        return _world(name, int(create["n"]), int(create["read_len"]), int(create["rng_seed"]))
    return _world(name, 0, 0, 0)


# ---------------------------------------------------------------------------------------------------------------- plan
# weights of the kinds of op; a kind that is not applicable in the tracked state is left out of the draw
WEIGHTS = dict(batch=15.0, refuse=1.6, table=1.0, rank=1.2, reads=0.8, coverage=0.8, coverage_rows=0.8, coverage_rank=0.9, depth=1.2,
               depth_rows=0.8, depth_count=0.6, depth_export=0.8, depth_import=1.2, table_add=1.3, reset=1.2, packed=1.0, flush=0.8,
               sync=1.5, wait=1.2, drain=0.8)
ENTRY_WEIGHTS = dict(enqueue_device=3.0, push_device=1.0, push=1.2, submit=2.2)
SIZE_WEIGHTS = dict(classes=(2, 2, 2, 2, 2, 1, 1), species=(3, 3, 3, 2, 2, 1, 3), tree=(1, 1, 1, 1, 1, 1, 1))
# ops that may run with tickets outstanding; every other op gets a drain in front of it
WITH_TICKETS = ("submit", "wait", "drain", "flush")


def _choice(rng, items, weights):
    w = np.asarray(weights, float)
    return items[int(rng.choice(len(items), p=w / w.sum()))]


def _draw_create(world, rng):
    op = dict(op="create", coalesce=int(rng.choice([1, 2, 3, 5, 8, 8])), lanes=int(rng.choice([1, 2, 2, 2, 3, 4])), query_rows=0, reuse=0,
              stat="depth")
    if world == "classes":
        op["top"] = int(rng.choice([1, 5]))
    elif world == "species":
        op["top"] = int(rng.choice([1, 3, 3, 17]))
        op["stat"] = str(rng.choice(["coverage", "depth", "depth"]))
        op["query_rows"] = int(rng.choice([0, 64]))
    else:
        op["top"] = int(rng.choice([1, 3]))
        op["reuse"] = int(rng.choice([0, 0, 1]))
        # (two trees in all -- each is made by a child process: read length and generator seed go with the size)
        op["n"] = int(rng.choice([1500, 2600]))
        op.update(read_len=200 if op["n"] == 1500 else 500, rng_seed=3 if op["n"] == 1500 else 4)
    return op


def _draw_bind(rng, m):
    """a random binding plan: any subset of the four bindings, caps from {1, 4, m}, rows or codes mode, the call with or without codes"""
    if rng.random() < 0.25:
        return {}
    on = [b for b in BINDINGS if rng.random() < 0.5] or [str(rng.choice(BINDINGS))]
    bind = {}
    if "cons" in on:
        bind["cons"] = True
    if "chg" in on:
        bind.update(chg=int(rng.choice([1, 4, m])), chg_codes=bool(rng.random() < 0.5))
    if "call" in on:
        bind.update(call=True, call_codes=bool(rng.random() < 0.5))
    if "cev" in on:
        bind.update(cev=int(rng.choice([1, 4, m])), cev_codes=bool(rng.random() < 0.5))
    return bind


def _draw_rows(rng, W):
    """a list of global genome indices with repeats, across the species' edges"""
    edges = [int(v) for f, n in zip(W.first, W.sizes) for v in (f, f + n - 1)]
    rows = [int(v) for v in rng.integers(0, W.n_genomes, size=int(rng.integers(1, 12)))] + [int(v) for v in rng.choice(edges, 2)]
    rows.append(rows[int(rng.integers(0, len(rows)))])
    return [rows[i] for i in rng.permutation(len(rows))]


def _draw_import(rng, W):
    """(hash, count) pairs: hashes the reference holds and hashes it does not, one of them named twice; small counts, now and then 0 or
    2^32 - 1"""
    pairs = [[int(W.held[int(rng.integers(0, len(W.held)))]), 0] for _ in range(int(rng.integers(1, 7)))]
    pairs += [[int(rng.integers(1, 2 ** 63)) * 2 + 1, 0] for _ in range(int(rng.integers(0, 4)))]
    pairs.append(list(pairs[int(rng.integers(0, len(pairs)))]))
    for p in pairs:
        p[1] = int(rng.choice([0, 1, 2, 3, 9, U32_MAX], p=[0.1, 0.25, 0.2, 0.15, 0.15, 0.15]))
    return [pairs[i] for i in rng.permutation(len(pairs))]


def plan(world, seed, max_ops=40, max_reads=1500, exclude=()):
    """the ops of one walk: deterministic in (world, seed), at most max_ops ops and max_reads reads, the last ops a drain (when tickets
    are out), a sync, the table and the read counter.  exclude: kinds of op to leave out."""
    assert world in WORLDS, world
    rng = np.random.default_rng(seed)
    create = _draw_create(world, rng)
    W = world_of(world, create)
    n_reads = min(W.n_reads, max_reads)
    ops = [create]
    pos = 0                # reads handed to the stream so far
    tickets = 0            # tickets issued so far
    out = []               # tickets issued since the last drain (the old walk's `outstanding`)
    waited = set()
    dev_pending = False    # enqueued / device-pushed batches since the last op that flushes
    packed = False
    stat = create["stat"]
    after_reset = streak = False
    room = max_ops - 4     # (the closing ops)

    def emit(op):
        ops.append(op)

    while len(ops) < room:
        left = n_reads - pos
        kinds = []
        for kind in WEIGHTS:
            if kind in exclude:
                continue
            if kind == "batch" and left < 1:
                continue
            if kind in ("coverage", "coverage_rows", "coverage_rank") and stat not in ("coverage", "depth"):
                continue
            if kind.startswith("depth") and stat != "depth":
                continue
            if kind == "wait" and not [t for t in out if t not in waited]:
                continue
            if kind == "drain" and not out:
                continue
            kinds.append(kind)
        # (with tickets out, more of what may follow them: a walk that drains at once never has two tickets in flight)
        kind = _choice(rng, kinds, [WEIGHTS[k] * (15.0 if out and k == "wait" else 5.0 if out and k == "batch" else 1.0) for k in kinds])
        if after_reset and stat == "depth" and "depth_import" not in exclude and rng.random() < 0.5:
            kind = "depth_import"   # (a checkpoint resumed on freshly zeroed counters)
        after_reset = False
        # several passes per batch need a batch of more distinct hashes than a pass has rows: large, and synchronous so that its passes
        # can be read behind it
        several = create["query_rows"] == 64
        ew = [ENTRY_WEIGHTS[e] * (4.0 if out and e == "submit" else 1.0) * (3.0 if several and e in ("push", "push_device") else 1.0) for e in ENTRIES]
        entry = _choice(rng, ENTRIES, ew) if kind in ("batch", "refuse") else None
        if streak and not out and left >= 1 and "batch" not in exclude and rng.random() < 0.45:
            kind, entry = "batch", "enqueue_device"   # (enqueued batches back to back: the ones that share a pass)
        streak = False
        key = entry if entry == "submit" else kind
        need = []
        if out and key not in WITH_TICKETS:
            need.append(dict(op="drain"))
        if key == "submit" and dev_pending:
            need.append(dict(op="flush"))
        if len(ops) + len(need) + 1 > room:
            break
        for op in need:
            emit(op)
            if op["op"] == "drain":
                out, dev_pending = [], False
            else:
                dev_pending = False
        if kind == "batch":
            fits = [(m, w * (8 if several and m == 400 else 1)) for m, w in zip(SIZES_OF_A_BATCH, SIZE_WEIGHTS[world]) if m <= left]
            m = int(_choice(rng, [f[0] for f in fits], [f[1] for f in fits]))
            bind = _draw_bind(rng, m)
            # NULL rows where the header allows them: push and submit always (outputs are optional; with a binding only the bound
            # outputs travel back), the _device entry points only with nothing bound
            null_rows = bool(rng.random() < 0.2) and (entry in ("push", "submit") or not bind)
            op = dict(op="batch", entry=entry, m=m, bind=bind, null_rows=null_rows)
            if entry in ("push", "push_device") and bind:
                op["stats"] = True   # (synchronous entry points: the runner reads last_passes behind them)
            emit(op)
            pos += m
            streak = entry == "enqueue_device"
        elif kind == "refuse":
            # more reads than max_batch_reads -- or, for a _device entry point, bindings without row arrays -- with bindings in front
            why = "null_rows" if entry in ("enqueue_device", "push_device") and rng.random() < 0.4 else "reads"
            bind = _draw_bind(rng, 4) or dict(cons=True)
            emit(dict(op="refuse", entry=entry, why=why, bind=bind))
            # every other refusal is pinned at once by a cheap query of the enabled statistic (the seen set and the counters must be
            # as they were); the others stay where they are, between the batches of a group.  No draw: the parity of the op's index
            pin = "depth_count" if stat == "depth" else "coverage_rows"
            if not out and len(ops) % 2 == 0 and len(ops) < room and pin not in exclude:
                emit(dict(op=pin, rows=_draw_rows(np.random.default_rng(seed + len(ops)), W)) if pin == "coverage_rows" else dict(op=pin))
                dev_pending = False   # (a query flushes)
        elif kind in ("coverage_rows", "depth_rows"):
            emit(dict(op=kind, rows=_draw_rows(rng, W)))
        elif kind == "coverage_rank":
            emit(dict(op=kind, top=int(rng.choice([1, 3, min(W.sizes)]))))
        elif kind == "depth_import":
            emit(dict(op=kind, pairs=_draw_import(rng, W)))
        elif kind == "table_add":
            # [genome, over]: the genome is lifted to its species' largest entry + over -- 400 is more than one read can add (s <= 300)
            emit(dict(op=kind, lift=[[int(rng.integers(0, W.n_genomes)), int(rng.choice([1, 400, 5000]))] for _ in range(int(rng.integers(1, 4)))]))
        elif kind == "packed":
            packed = not packed
            emit(dict(op=kind, on=packed))
        elif kind == "wait":
            t = int(rng.choice([t for t in out if t not in waited]))
            waited.add(t)
            emit(dict(op=kind, ticket=t))
        else:
            emit(dict(op=kind))
        # what the op leaves behind
        if kind == "refuse":
            pass   # (refused before the library flushes anything: enqueued batches stay pending, whatever the entry point)
        elif kind == "batch" and entry == "submit":
            out.append(tickets)
            tickets += 1
        elif kind == "batch" and entry in ("enqueue_device", "push_device"):
            dev_pending = True
        elif kind == "drain":
            out, dev_pending = [], False
        elif kind not in ("reads", "wait"):
            dev_pending = False
        if kind == "reset":
            after_reset = True
    if out:
        emit(dict(op="drain"))
    emit(dict(op="sync"))
    emit(dict(op="table"))
    emit(dict(op="reads"))
    assert len(ops) <= max_ops and pos <= max_reads
    return ops


# ---------------------------------------------------------------------------------------------------------------- model
class Model:
    """the state of one stream on the CPU; apply(op) -> what the device has to return for that op"""

    def __init__(self, W, create):
        self.W, self.top = W, int(create["top"])
        self.stat = create["stat"]
        self.cums = [np.zeros(n, np.uint64) for n in W.sizes]
        self.counter = {}          # held hash -> clamped number of reads (and imported counts)
        self.pos = 0               # next read of the world
        self.reads = 0             # reads since the last reset
        self.tickets = 0
        self.packed = False
        self._figures = None
        self._lifted = None        # (the genomes of the last table_add, the table before it) until the next batch

    # -- rows
    def _rows(self, a, b, cums):
        W = self.W
        outs = [orc.stream(K_MER, SEED, W.s, r, c, W.bases, W.offsets[a:b + 1], top_k=self.top, cum=cum)
                for r, c, cum in zip(W.refs, W.col_lens, cums)]
        return (np.stack([o["topk_idx"] for o in outs], axis=1).astype(np.uint32),
                np.stack([o["topk_sum"] for o in outs], axis=1).astype(np.uint64), [o["cum"] for o in outs])

    def _batch(self, m):
        W, a, b = self.W, self.pos, self.pos + m
        assert b <= W.n_reads
        idx, sm, cums = self._rows(a, b, self.cums)
        codes = consensus_ref(idx, W.codes, W.sizes)
        call = call_ref(idx, sm, codes)
        exp = dict(rows_idx=idx, rows_sum=sm, cons=codes, call_sp=call["call_species"], call_idx=call["call_idx"], call_sum=call["call_sum"],
                   call_codes=call["call_codes"], chg_ev=dict(rows=changes_ref(idx), codes=changes_ref(codes)),
                   cev_ev=dict(rows=call_changes_ref(call["call_species"], call["call_idx"]),
                               codes=call_changes_ref(call["call_species"], call["call_codes"])), first=a, m=m)
        held = [h for sk in W.sketches[a:b] for h in sk]
        exp["distinct_held"] = len(set(held))
        if self._lifted is not None:   # did the first row's leader lead only because of the add?
            lifted, before = self._lifted
            plain = self._rows(a, a + 1, before)[0]
            exp["led_by_add"] = any(int(W.first[sp]) + int(idx[0, sp, 0]) in lifted and int(plain[0, sp, 0]) != int(idx[0, sp, 0])
                                    for sp in range(W.n_species))
            self._lifted = None
        for h in held:
            self.counter[h] = min(self.counter.get(h, 0) + 1, U32_MAX)
        self.cums, self.pos, self.reads, self._figures = cums, b, self.reads + m, None
        return exp

    # -- breadth and depth
    def figures(self):
        """(covered uint32, median uint32, total uint64) per genome"""
        if self._figures is None:
            self._figures = dc.summarise(dc.depth_matrix(self.W.refs, self.W.col_lens, self.counter))
        return self._figures

    def table(self):
        return np.concatenate(self.cums)

    def rank(self, top):
        """(idx uint32, sum uint64) [n_species, top]: (sum desc, index asc) per species"""
        idx, sm = np.zeros((self.W.n_species, top), np.uint32), np.zeros((self.W.n_species, top), np.uint64)
        for sp, cum in enumerate(self.cums):
            order = np.lexsort((np.arange(len(cum)), -cum.astype(np.int64)))[:top]
            idx[sp], sm[sp] = order, cum[order]
        return idx, sm

    def apply(self, op):
        W, kind = self.W, op["op"]
        if kind == "batch":
            exp = self._batch(op["m"])
            if op["entry"] == "submit":
                exp["ticket"] = self.tickets
                self.tickets += 1
            return exp
        if kind in ("refuse", "flush", "sync", "wait", "drain", "create"):
            return {}
        if kind == "packed":
            self.packed = bool(op["on"])
            return {}
        if kind == "table":
            return dict(table=self.table())
        if kind == "rank":
            idx, sm = self.rank(self.top)
            return dict(idx=idx, sum=sm)
        if kind == "reads":
            return dict(reads=self.reads)
        if kind == "coverage":
            return dict(covered=self.figures()[0])
        if kind == "coverage_rows":
            return dict(covered=self.figures()[0][np.asarray(op["rows"], np.int64)])
        if kind == "coverage_rank":
            idx, val = cc.expected_rank(self.figures()[0], W.sizes, op["top"])
            return dict(idx=idx, covered=val)
        if kind == "depth":
            return dict(zip(("covered", "median", "total"), self.figures()))
        if kind == "depth_rows":
            rows = np.asarray(op["rows"], np.int64)
            return dict(zip(("covered", "median", "total"), (f[rows] for f in self.figures())))
        if kind == "depth_count":
            return dict(n=sum(1 for c in self.counter.values() if c > 0))
        if kind == "depth_export":
            hashes, counts = dc.reference_pairs(W.refs, W.col_lens, {h: c for h, c in self.counter.items() if c > 0})
            return dict(hashes=hashes, counts=counts)
        if kind == "depth_import":
            held, unknown = set(int(h) for h in W.held), 0
            for h, c in op["pairs"]:
                if h not in held:
                    unknown += 1
                elif c > 0:
                    self.counter[h] = min(self.counter.get(h, 0) + c, U32_MAX)
            self._figures = None
            return dict(unknown=unknown)
        if kind == "table_add":
            add = np.zeros(W.n_genomes, np.uint64)
            table = self.table()
            for g, over in op["lift"]:
                sp = int(np.searchsorted(W.first, g, side="right")) - 1
                top = int(self.cums[sp].max())
                add[g] = max(int(add[g]), top - int(table[g]) + over)
            before = [c.copy() for c in self.cums]
            self.cums = [c + add[f:f + n] for c, f, n in zip(self.cums, W.first, W.sizes)]
            lifted = set(int(g) for g, _ in op["lift"])
            self._lifted = (lifted, before) if self._lifted is None else (lifted | self._lifted[0], self._lifted[1])
            return dict(add=add)
        if kind == "reset":
            self.cums = [np.zeros(n, np.uint64) for n in W.sizes]
            self.counter, self.reads, self._figures, self._lifted = {}, 0, None, None
            return {}
        raise ValueError(f"unknown op {op!r}")


def trace(world, ops):
    """[(op, expectation)] of a plan on the model alone"""
    model = Model(world_of(world, ops[0]), ops[0])
    return [(op, model.apply(op)) for op in ops]


# ---------------------------------------------------------------------------------------------------------------- checks
def written(got, names):
    """the names of the arrays that no longer hold the sentinel everywhere"""
    return [k for k in names if not (got[k] == SENT[got[k].dtype]).all()]


def _check_events(g, pre, cap, ev, cols, w):
    m = min(len(ev), cap)
    assert int(g[pre + "_n"][0]) == len(ev), f"{w}: {pre} n_events {int(g[pre + '_n'][0])}, expected {len(ev)}"
    np.testing.assert_array_equal(g[pre + "_read"][:m], ev[:m], err_msg=f"{w}: {pre}_read")
    assert (g[pre + "_read"][m:] == SENT[np.dtype(np.uint32)]).all(), f"{w}: {pre}_read past min(n_events, cap) was written"
    for name, rows in cols.items():
        k = f"{pre}_{name}"
        if rows is None:
            assert not written(g, (k,)), f"{w}: {k} was not bound and was written"
            continue
        np.testing.assert_array_equal(g[k][:m], rows[ev[:m]], err_msg=f"{w}: {k}")
        assert (g[k][m:] == SENT[g[k].dtype]).all(), f"{w}: {k} past min(n_events, cap) was written"


def check_batch(g, exp, op, w):
    """one batch's memory against the model: the values, the sentinel in whatever was not bound, the sentinel past min(n_events, cap)"""
    if op["op"] == "refuse":
        assert not written(g, g.keys()), f"{w}: a refused batch wrote {written(g, g.keys())}"
        return
    bind = op["bind"]
    if op["null_rows"]:
        assert not written(g, ("rows_idx", "rows_sum")), f"{w}: rows were not asked for"
    else:
        np.testing.assert_array_equal(g["rows_sum"], exp["rows_sum"], err_msg=f"{w}: rows_sum")
        np.testing.assert_array_equal(g["rows_idx"], exp["rows_idx"], err_msg=f"{w}: rows_idx")
    for name, cols in GROUPS.items():
        if not bind.get(name):
            assert not written(g, cols), f"{w}: {name} was not bound, {written(g, cols)} written"
    if bind.get("cons"):
        np.testing.assert_array_equal(g["cons"], exp["cons"], err_msg=f"{w}: cons")
    if bind.get("chg"):
        by = "codes" if bind["chg_codes"] else "rows"
        _check_events(g, "chg", bind["chg"], exp["chg_ev"][by],
                      dict(idx=exp["rows_idx"], sum=exp["rows_sum"], codes=exp["cons"] if bind["chg_codes"] else None), w)
    if bind.get("call"):
        for k in ("call_sp", "call_idx", "call_sum"):
            np.testing.assert_array_equal(g[k], exp[k], err_msg=f"{w}: {k}")
        if bind["call_codes"]:
            np.testing.assert_array_equal(g["call_codes"], exp["call_codes"], err_msg=f"{w}: call_codes")
        else:
            assert not written(g, ("call_codes",)), f"{w}: call_codes was not bound and was written"
    if bind.get("cev"):
        by = "codes" if bind["cev_codes"] else "rows"
        _check_events(g, "cev", bind["cev"], exp["cev_ev"][by],
                      dict(sp=exp["call_sp"], idx=exp["call_idx"], sum=exp["call_sum"], codes=exp["call_codes"] if bind["cev_codes"] else None), w)


# ---------------------------------------------------------------------------------------------------------------- runner
_REFS = {}


def reference(W):
    """the world's reference on the device with its genotype table: created once per process (the table can be set once)"""
    from sketchy_amd import api
    if W.key not in _REFS:
        if W.name == "classes":
            R = cc.create_reference(W.design, hc.R_TEST)[0]
        elif W.n_species == 1:
            R = api.ReferenceSketch(W.refs[0], W.col_lens[0])
        else:
            R = api.ReferenceSketch(W.refs, W.col_lens)
        R.set_genotypes(W.codes)
        _REFS[W.key] = R
    return _REFS[W.key]


def close_references():
    for R in _REFS.values():
        R.close()
    _REFS.clear()


def _create_stream(R, W, create):
    from sketchy_amd import api
    names = dict(stream_coalesce="coalesce", rank_lanes="lanes", stream_query_rows="query_rows", reuse_membership="reuse")
    before = {k: api.get_option(k) for k in names}
    try:
        for k, field in names.items():
            api.set_option(k, create[field])
        S = api.SumOfSharedHashes(R, top=create["top"], max_batch_reads=MAX_BATCH_READS, max_batch_bases=max(1, len(W.bases)))
    finally:
        for k, v in before.items():
            api.set_option(k, v)
    if create["stat"] == "depth":
        S.enable_depth()
    elif create["stat"] == "coverage":
        S.enable_coverage()
    return S


def _spec(n, n_sp, top):
    return dict(rows_idx=((n, n_sp, top), np.uint32), rows_sum=((n, n_sp, top), np.uint64), cons=((n, n_sp, N_FEAT), np.uint32),
                chg_n=((1,), np.uint32), chg_read=((n,), np.uint32), chg_idx=((n, n_sp, top), np.uint32),
                chg_sum=((n, n_sp, top), np.uint64), chg_codes=((n, n_sp, N_FEAT), np.uint32),
                call_sp=((n,), np.uint32), call_idx=((n, top), np.uint32), call_sum=((n, top), np.uint64), call_codes=((n, N_FEAT), np.uint32),
                cev_n=((1,), np.uint32), cev_read=((n,), np.uint32), cev_sp=((n,), np.uint32), cev_idx=((n, top), np.uint32),
                cev_sum=((n, top), np.uint64), cev_codes=((n, N_FEAT), np.uint32))


def _bind(S, q, bind):
    if bind.get("cons"):
        S.bind_consensus(q("cons"))
    if bind.get("chg"):
        S.bind_changes(bind["chg"], q("chg_n"), q("chg_read"), q("chg_idx"), q("chg_sum"), q("chg_codes") if bind["chg_codes"] else None)
    if bind.get("call"):
        S.bind_call(q("call_sp"), q("call_idx"), q("call_sum"), q("call_codes") if bind["call_codes"] else None)
    if bind.get("cev"):
        S.bind_call_changes(bind["cev"], q("cev_n"), q("cev_read"), q("cev_sp"), q("cev_idx"), q("cev_sum"),
                            q("cev_codes") if bind["cev_codes"] else None)


def run(world, ops, seed=None):
    """execute a plan on the device against the model; -> dict(stats, seconds, reads, bound, bound_passes, executed)"""
    import ctypes as C

    from sketchy_amd import _lib, api
    L = _lib.load()
    t0 = time.perf_counter()
    create = ops[0]
    assert create["op"] == "create"
    W = world_of(world, create)
    model = Model(W, create)
    S = _create_stream(reference(W), W, create)
    n_sp, top = W.n_species, model.top
    packed, poff = api.pack_reads(W.bases, W.offsets)
    text = {False: (W.bases, W.offsets), True: (packed, poff)}
    keep = []                 # device and page-locked buffers, freed at the end (inputs stay untouched until the stream is through)
    dev = {p: api.DeviceBuffer.from_numpy(text[p][0]) for p in (False, True)}
    pin = {}
    for p in (False, True):
        pin[p] = api.HostBuffer(max(len(text[p][0]), 8))
        pin[p].view(np.uint8, len(text[p][0]))[:] = text[p][0]
    keep += list(dev.values()) + list(pin.values())
    pending = []              # (kind, ticket, Mem, expectation, op, index): outputs not yet guaranteed to be there
    refused_host = []         # (Mem, op, index) of refused pushes: host arrays, looked at again behind later batches and at the end
    info = dict(bound=False, bound_passes=0, total=0)
    executed, i = 0, 0

    def resolve(which):
        for item in [p for p in pending if which(p)]:
            kind, ticket, M, exp, op, at = item
            check_batch(M.read(), exp, op, f"op {at} {op}")
            pending.remove(item)
        recheck_refused("at a resolution")

    def recheck_refused(when):
        """the host arrays of refused pushes still hold the sentinel: nothing that came later wrote through a binding made for them"""
        for M, op, at in refused_host:
            check_batch(M.read(), {}, op, f"op {at} {op}, looked at again {when}")

    def batch(op, exp, at):
        refused = op["op"] == "refuse"
        entry, bind = op["entry"], op["bind"]
        if refused:
            m = MAX_BATCH_READS + 1 if op["why"] == "reads" else 7
            a = 0                      # (any reads of the world: none of them is consumed)
        else:
            m, a = op["m"], exp["first"]
        off = np.ascontiguousarray(text[model.packed][1][a:a + m + 1], np.uint64)
        kind = {"push": "host", "submit": "pinned"}.get(entry, "device")
        M = Mem(kind, _spec(m, n_sp, top))
        keep.append(M)
        _bind(S, M.ptr, bind)
        null = op["null_rows"] if not refused else op["why"] == "null_rows"
        ri, rs = (None, None) if null else (M.ptr("rows_idx"), M.ptr("rows_sum"))
        ticket = None

        def call():
            nonlocal ticket
            if entry == "push":
                b = text[model.packed][0]
                _lib.check(L.skx_stream_push(S._h, b.ctypes.data_as(C.c_void_p), off.ctypes.data_as(C.c_void_p), m, ri, rs, None, None, None))
            elif entry == "submit":
                ho = api.HostBuffer((m + 1) * 8)
                keep.append(ho)
                ho.view(np.uint64, m + 1)[:] = off
                ticket = S.submit(pin[model.packed].ptr, ho.ptr, m, ri, rs)
            else:
                d_o = api.DeviceBuffer.from_numpy(off)
                keep.append(d_o)
                fn = S.enqueue_device if entry == "enqueue_device" else S.push_device
                fn(dev[model.packed].ptr, d_o.ptr, m, int(off[-1] - off[0]), ri, rs)
        if refused:
            before = S.reads
            try:
                call()
            except _lib.SketchyHipError as e:
                # include/sketchy_hip.h: SKX_ERR_CAPACITY for a batch beyond the capacity given at skx_stream_create, SKX_ERR_INVALID
                # for a bound _device batch without row arrays
                want = _lib.ERR_CAPACITY if op["why"] == "reads" else _lib.ERR_INVALID
                assert e.code == want, f"op {at}: refused with {e.code}, expected {want}: {e}"
            else:
                raise AssertionError(f"op {at}: the batch was accepted")
            assert S.reads == before, f"op {at}: a refused batch moved the read counter"
        else:
            call()
            info["total"] += m
            if bind:
                info["bound"] = True
        if entry == "submit" and not refused:
            assert ticket == exp["ticket"], (ticket, exp["ticket"])
        if kind == "host":
            check_batch(M.read(), exp, op, f"op {at} {op}")
            if refused:
                refused_host.append((M, op, at))
        else:
            pending.append((kind, ticket, M, exp, op, at))
        recheck_refused(f"behind op {at}")   # (a binding that was not consumed would send this batch's outputs there)
        if op.get("stats"):
            passes = S.stats()["last_passes"]
            if bind:
                info["bound_passes"] = max(info["bound_passes"], passes)

    try:
        for i, op in enumerate(ops):
            kind = op["op"]
            exp = model.apply(op)
            w = f"op {i} {kind}"
            if kind == "create":
                pass
            elif kind in ("batch", "refuse"):
                batch(op, exp, i)
            elif kind == "table":
                np.testing.assert_array_equal(S.table(), exp["table"], err_msg=w)
            elif kind == "rank":
                gi, gs = S.rank(top)
                np.testing.assert_array_equal(gs.reshape(n_sp, top), exp["sum"], err_msg=w)
                np.testing.assert_array_equal(gi.reshape(n_sp, top), exp["idx"], err_msg=w)
            elif kind == "reads":
                assert S.reads == exp["reads"], f"{w}: {S.reads}, expected {exp['reads']}"
            elif kind == "coverage":
                np.testing.assert_array_equal(S.coverage(), exp["covered"], err_msg=w)
            elif kind == "coverage_rows":
                np.testing.assert_array_equal(S.coverage_rows(np.asarray(op["rows"], np.uint32)), exp["covered"], err_msg=w)
            elif kind == "coverage_rank":
                gi, gv = S.coverage_rank(op["top"])
                np.testing.assert_array_equal(gv, exp["covered"], err_msg=w)
                np.testing.assert_array_equal(gi, exp["idx"], err_msg=w)
            elif kind in ("depth", "depth_rows"):
                got = S.depth() if kind == "depth" else S.depth_rows(np.asarray(op["rows"], np.uint32))
                for name, g in zip(("covered", "median", "total"), got):
                    np.testing.assert_array_equal(g, exp[name], err_msg=f"{w} {name}")
            elif kind == "depth_count":
                assert S.depth_count() == exp["n"], f"{w}: {S.depth_count()}, expected {exp['n']}"
            elif kind == "depth_export":
                hashes, counts = S.depth_export()
                order = np.argsort(hashes)
                np.testing.assert_array_equal(hashes[order], exp["hashes"], err_msg=w)
                np.testing.assert_array_equal(counts[order], exp["counts"], err_msg=w)
            elif kind == "depth_import":
                got = S.depth_import(np.array([p[0] for p in op["pairs"]], np.uint64), np.array([p[1] for p in op["pairs"]], np.uint32))
                assert got == exp["unknown"], f"{w}: {got} unknown hashes, expected {exp['unknown']}"
            elif kind == "table_add":
                S.table_add(exp["add"])
            elif kind == "reset":
                S.reset()
            elif kind == "packed":
                S.set_packed_input(op["on"])
            elif kind == "flush":
                S.flush()
            elif kind == "sync":
                S.sync()
                resolve(lambda p: p[0] == "device")
            elif kind == "wait":
                S.wait(op["ticket"])
                resolve(lambda p: p[0] == "pinned" and p[1] == op["ticket"])
            elif kind == "drain":
                S.drain()
                resolve(lambda p: p[0] == "pinned")
            else:
                raise ValueError(f"unknown op {op!r}")
            executed += 1
        recheck_refused("at the end of the walk")
        assert not pending, f"{len(pending)} batches were never resolved: the plan does not end in a drain and a sync"
        assert executed == len(ops)
        info.update(stats=S.stats(), executed=executed, reads=model.reads, stats_reads=S.reads)
    except BaseException:
        print(f"\nwalk failed: world {world!r}, seed {seed!r}, op {i} of {len(ops)}: {ops[i]!r}\nreplay({world!r}, {ops[:i + 1]!r})")
        raise
    finally:
        S.close()
        for x in keep:
            x.free()
    info["seconds"] = time.perf_counter() - t0
    return info


def replay(world, ops):
    """run an op list as a failed walk printed it; ops that end mid-walk are closed with a drain and a sync"""
    ops = [dict(op) for op in ops]
    if ops[-1]["op"] != "sync":
        ops += [dict(op="drain"), dict(op="sync")]
    return run(world, ops)


def walk(world, seed, **kw):
    return run(world, plan(world, seed, **kw), seed=seed)
