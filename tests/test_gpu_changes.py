"""Change points on the device: skx_changes_rows alone, and the event list every stream entry point returns through
skx_stream_bind_changes, against test_changes_cpu.changes_ref.  The events of a batch are a pure function of its rows (or of the
consensus codes of its rows), so the stream cases apply the restatement, batch by batch, to the rows a SECOND stream returns for the
same reads with nothing bound -- and hold the bound stream's own rows to those rows."""
import ctypes as C
import gzip
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from helpers import exp_env, unpack_reads, workload, workload_species
from mshio import write_msh
from test_changes_cpu import changes_ref, filter_changes
from test_consensus_cpu import consensus_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "sketchy_amd", "sketchy-hip")
WORKER = os.path.join(ROOT, "tests", "changes_worker.py")
SENT = 0xDEADBEEF


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


# ---------------------------------------------------------------- the operator alone
WIDTHS = (1, 2, 63, 64, 65, 1024, 4096)
ROWS = (1, 63, 64, 65, 1025, 5000)


def make_rows(kind, n, width, rng):
    if kind == "equal":
        return np.broadcast_to(rng.integers(0, 2 ** 32, width, dtype=np.uint64).astype(np.uint32), (n, width)).copy()
    if kind == "different":  # every row differs from the one before, in one element at a random place
        rows = np.zeros((n, width), np.uint32)
        rows[np.arange(n), rng.integers(0, width, n)] = np.arange(1, n + 1, dtype=np.uint32)
        return rows
    if kind == "three":
        vals = rng.integers(0, 2 ** 32, (3, width), dtype=np.uint64).astype(np.uint32)
        vals[1, :-1] = vals[0, :-1]  # (two of the three differ in the last element only)
        vals[1, -1] = vals[0, -1] ^ 1
        return vals[rng.integers(0, 3, n)]
    rows = np.broadcast_to(rng.integers(0, 2 ** 32, width, dtype=np.uint64).astype(np.uint32), (n, width)).copy()
    rows[:, -1 if kind == "last" else 0] = rng.integers(0, 2, n).astype(np.uint32) * 0x80000000  # runs of equal rows
    return rows


@pytest.mark.parametrize("width", WIDTHS)
def test_operator_against_the_restatement(gpu, width):
    from sketchy_amd import _lib
    L = _lib.load()
    rng = np.random.default_rng(width)
    for kind in ("equal", "different", "three", "last", "first"):
        for n in ROWS:
            rows = make_rows(kind, n, width, rng)
            want = changes_ref(rows)
            if kind == "equal":
                assert len(want) == 1
            if kind == "different":
                assert len(want) == n
            if kind in ("three", "last", "first") and n >= 63:
                assert 1 < len(want) < n
            for cap in sorted({len(want) + 3, max(len(want) - 1, 1), 1}):
                ev = np.full(cap + 5, SENT, np.uint64)
                n_ev = C.c_uint64(SENT)
                assert L.skx_changes_rows(0, _p(rows), n, width, cap, C.byref(n_ev), _p(ev)) == _lib.OK, L.skx_last_error()
                m = min(len(want), cap)
                what = f"{kind} rows {n} width {width} cap {cap}"
                assert n_ev.value == len(want), what
                np.testing.assert_array_equal(ev[:m], want[:m], err_msg=what)
                assert (ev[m:] == SENT).all(), what + ": entries past min(n, cap) were written"


def test_operator_api_and_errors(gpu):
    from sketchy_amd import _lib, api
    L = _lib.load()
    rows = make_rows("three", 300, 5, np.random.default_rng(3)).reshape(300, 1, 5)
    n, ev = api.changes_rows(rows)
    np.testing.assert_array_equal(ev, changes_ref(rows))
    assert n == len(ev) and ev.dtype == np.uint64
    n, ev = api.changes_rows(rows, cap=4)
    assert n == len(changes_ref(rows)) and ev.tolist() == changes_ref(rows)[:4].tolist()
    assert api.changes_rows(np.zeros((0, 5), np.uint32))[0] == 0
    flat = np.zeros(16, np.uint32)
    out, n_ev = np.full(4, SENT, np.uint64), C.c_uint64(SENT)
    for args in ((None, 4, 4, 4, C.byref(n_ev), _p(out)), (_p(flat), 4, 4, 4, None, _p(out)), (_p(flat), 4, 4, 4, C.byref(n_ev), None),
                 (_p(flat), 4, 0, 4, C.byref(n_ev), _p(out)), (_p(flat), 0, 4097, 4, C.byref(n_ev), _p(out))):
        assert L.skx_changes_rows(0, *args) == _lib.ERR_INVALID, args
    assert (out == SENT).all()
    assert L.skx_changes_rows(0, _p(flat), 0, 4, 4, C.byref(n_ev), _p(out)) == _lib.OK and n_ev.value == 0 and (out == SENT).all()


def test_operator_in_chunks_with_a_change_and_a_non_change_at_the_seams(gpu, tmp_path):
    """Chunks of 100 rows (SKX_CHANGES_ROWS, experiments build): row 100 differs from row 99, row 200 equals row 199, row 300 differs in
    its last element only; the last chunk holds 37 rows."""
    rng = np.random.default_rng(12)
    rows = make_rows("three", 437, 65, rng)
    rows[100] = rows[99]
    rows[100, 7] ^= 1
    rows[200] = rows[199]
    rows[300] = rows[299]
    rows[300, -1] ^= 1
    want = changes_ref(rows)
    assert 100 in want and 300 in want and 200 not in want and 1 < len(want) < 437
    caps = [len(want) + 3, len(want) - 1, 1, int(np.searchsorted(want, 100)), int(np.searchsorted(want, 200))]
    src, dst = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    np.savez(src, rows=rows, caps=np.array(caps))
    r = subprocess.run([sys.executable, WORKER, "chunks", src, dst], env=exp_env(SKX_CHANGES_ROWS=100), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    z = np.load(dst)
    for cap in caps:
        assert int(z[f"n{cap}"]) == len(want), cap
        np.testing.assert_array_equal(z[f"ev{cap}"], want[:cap], err_msg=f"cap {cap}")


# ---------------------------------------------------------------- streams
class Events:
    """the event arrays of one batch, in whatever memory the entry point takes, pre-filled with a sentinel"""

    def __init__(self, kind, cap, n_sp, top, n_feat, codes):
        from sketchy_amd import api
        self.kind, self.cap = kind, cap
        self.shapes = [((1,), np.uint32), ((cap,), np.uint32), ((cap, n_sp, top), np.uint32), ((cap, n_sp, top), np.uint64),
                       ((cap, n_sp, n_feat), np.uint32) if codes else None]
        self.bufs = []
        for sh in self.shapes:
            if sh is None:
                self.bufs.append(None)
                continue
            fill = np.full(sh[0], SENT, sh[1])
            if kind == "device":
                self.bufs.append(api.DeviceBuffer.from_numpy(fill))
            elif kind == "pinned":
                hb = api.HostBuffer(fill.nbytes)
                hb.view(sh[1])[:] = fill.ravel()
                self.bufs.append(hb)
            else:
                self.bufs.append(fill)

    def binding(self):
        return (self.cap,) + tuple(None if b is None else (_p(b) if self.kind == "host" else b.ptr) for b in self.bufs)

    def read(self):
        out = []
        for b, sh in zip(self.bufs, self.shapes):
            if b is None:
                out.append(None)
            elif self.kind == "device":
                out.append(b.to_numpy(sh[1], sh[0]))
            elif self.kind == "pinned":
                out.append(b.view(sh[1]).reshape(sh[0]).copy())
            else:
                out.append(b)
        return dict(n=int(out[0][0]), read=out[1], idx=out[2], sum=out[3], codes=out[4])

    def free(self):
        if self.kind != "host":
            for b in self.bufs:
                if b is not None:
                    b.free()


def drive(S, entry, bases, offsets, cuts, top, n_sp, n_feat=0, cap=None, codes=False, bind_cons=False, null_rows=False):
    """every batch [cuts[i], cuts[i + 1]) through one entry point -> (idx [n, n_sp, top] or None, sum likewise, [events of every batch]);
    cap: bind an event list of that many entries to every batch (codes: in codes mode; bind_cons: a consensus output as well)"""
    from sketchy_amd import _lib, api
    n_all = cuts[-1] - cuts[0]
    kind = {"push": "host", "submit": "pinned"}.get(entry, "device")
    evs = [Events(kind, cap, n_sp, top, n_feat, codes) for _ in cuts[1:]] if cap else []
    bufs = []
    try:
        if entry == "push":
            idx, sm = np.zeros((n_all, n_sp, top), np.uint32), np.zeros((n_all, n_sp, top), np.uint64)
            for i, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
                cons = np.zeros((b - a, n_sp, n_feat), np.uint32) if bind_cons else None
                if bind_cons:
                    S.bind_consensus(_p(cons))
                if cap:
                    S.bind_changes(*evs[i].binding())
                o = np.ascontiguousarray(offsets[a:b + 1], np.uint64)
                _lib.check(_lib.load().skx_stream_push(S._h, _p(bases), _p(o), b - a, None if null_rows else _p(idx[a - cuts[0]:]),
                                                       None if null_rows else _p(sm[a - cuts[0]:]), None, None, None))
        elif entry == "submit":
            at = lambda buf, off: C.c_void_p(buf.ptr.value + off)
            hb, ho = api.HostBuffer(len(bases)), api.HostBuffer(len(offsets) * 8)
            hi, hs, hc = api.HostBuffer(n_all * n_sp * top * 4), api.HostBuffer(n_all * n_sp * top * 8), api.HostBuffer(max(n_all * n_sp * n_feat * 4, 4))
            bufs += [hb, ho, hi, hs, hc]
            hb.view(np.uint8)[:] = bases
            ho.view(np.uint64)[:] = offsets
            hi.view(np.uint32)[:] = 0xFFFFFFFF
            for i, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
                r = a - cuts[0]
                S.submit(hb.ptr, at(ho, a * 8), b - a, None if null_rows else at(hi, r * n_sp * top * 4),
                         None if null_rows else at(hs, r * n_sp * top * 8), consensus=at(hc, r * n_sp * n_feat * 4) if bind_cons else None,
                         changes=evs[i].binding() if cap else None)
            S.drain()
            idx = hi.view(np.uint32).reshape(n_all, n_sp, top).copy()
            sm = hs.view(np.uint64).reshape(n_all, n_sp, top).copy()
        else:
            d_b = api.DeviceBuffer.from_numpy(bases)
            bufs.append(d_b)
            rows = []
            for i, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
                n = b - a
                d_o = api.DeviceBuffer.from_numpy(np.ascontiguousarray(offsets[a:b + 1], np.uint64))
                d_i, d_s, d_c = api.DeviceBuffer(n * n_sp * top * 4), api.DeviceBuffer(n * n_sp * top * 8), api.DeviceBuffer(max(n * n_sp * n_feat * 4, 4))
                bufs += [d_o, d_i, d_s, d_c]
                rows.append((n, d_i, d_s))
                fn = S.enqueue_device if entry == "enqueue_device" else S.push_device
                fn(d_b.ptr, d_o.ptr, n, int(offsets[b] - offsets[a]), d_i.ptr, d_s.ptr, consensus=d_c.ptr if bind_cons else None,
                   changes=evs[i].binding() if cap else None)
            S.sync()
            idx = np.concatenate([d_i.to_numpy(np.uint32, (n, n_sp, top)) for n, d_i, _ in rows])
            sm = np.concatenate([d_s.to_numpy(np.uint64, (n, n_sp, top)) for n, _, d_s in rows])
        got = [e.read() for e in evs]
        return (None, None, got) if null_rows else (idx, sm, got)
    finally:
        for b in bufs:
            b.free()
        for e in evs:
            e.free()


def check_events(got, cuts, idx, sm, cap, call=None, what=""):
    """got: the events of every batch; idx / sm: the expected rows of all reads; call: what is compared (default: idx)"""
    call = idx if call is None else call
    for ev, a, b in zip(got, cuts[:-1], cuts[1:]):
        want = changes_ref(call[a:b])
        m = min(len(want), cap)
        w = f"{what} batch at {a}"
        assert ev["n"] == len(want), w
        np.testing.assert_array_equal(ev["read"][:m], want[:m], err_msg=w)
        np.testing.assert_array_equal(ev["idx"][:m], idx[a:b][want[:m]], err_msg=w)
        np.testing.assert_array_equal(ev["sum"][:m], sm[a:b][want[:m]], err_msg=w)
        if ev["codes"] is not None:
            np.testing.assert_array_equal(ev["codes"][:m], call[a:b][want[:m]], err_msg=w)
        for k in ("read", "idx", "sum", "codes"):
            assert ev[k] is None or (ev[k][m:] == SENT).all(), f"{w}: {k} past min(n, cap) was written"


@pytest.fixture(scope="module")
def near(gpu):
    """the near-tie stream: 513 genomes, s = 64, 2 800 reads of 300 bases, four batches of 700; rows of a stream that never binds, per top"""
    from sketchy_amd import api
    ref, bases, offsets = workload(513, 64, 2800, read_len=300, rng_seed=911)
    R = api.ReferenceSketch(ref["ref"], ref["col_len"])
    out = dict(R=R, ref=ref, bases=bases, offsets=offsets, cuts=[0, 700, 1400, 2100, 2800], plain={})
    yield out
    R.close()


def stream(near, top):
    from sketchy_amd import api
    return api.SumOfSharedHashes(near["R"], top=top, max_batch_reads=700, max_batch_bases=700 * 300)


def plain_rows(near, top):
    if top not in near["plain"]:
        S = stream(near, top)
        near["plain"][top] = drive(S, "push", near["bases"], near["offsets"], near["cuts"], top, 1)[:2]
        S.close()
    return near["plain"][top]


ENTRIES = [("push", False), ("push_device", False), ("enqueue_device", False), ("submit", False), ("submit", True)]


@pytest.mark.parametrize("entry,null_rows", ENTRIES, ids=("push", "push_device", "enqueue_device", "submit", "submit_null_rows"))
def test_every_entry_point_returns_the_events_of_its_rows(near, entry, null_rows):
    idx, sm = plain_rows(near, 5)
    per_batch = [len(changes_ref(idx[a:a + 700])) for a in near["cuts"][:-1]]
    assert all(2 <= n <= 350 for n in per_batch), per_batch  # (the CPU oracle: 54 / 67 / 62 / 33 adjacent changes + the forced first reads)
    S = stream(near, 5)
    got_idx, got_sum, ev = drive(S, entry, near["bases"], near["offsets"], near["cuts"], 5, 1, cap=700, null_rows=null_rows)
    if entry == "enqueue_device":
        assert S.stats()["passes_shared"] >= 1  # the four batches shared a pass: their chains ran on both lanes
    S.close()
    if not null_rows:
        np.testing.assert_array_equal(got_idx, idx, err_msg="a binding changed the rows")
        np.testing.assert_array_equal(got_sum, sm, err_msg="a binding changed the sums")
    check_events(ev, near["cuts"], idx, sm, 700, what=entry)


@pytest.mark.parametrize("top,total", [(1, 46), (5, 216), (17, 344), (64, 670)])
def test_ranking_paths(near, top, total):
    """top 1 (rank_seg_top1), 5 (the fast top-k), 17 and 64 (the generic ranking) in front of the flags; `total`: the change points of
    the 2 800 reads as one stream, from the CPU oracle.  At top 1 a run of 995 reads without one: a block of the scan with no flag."""
    idx, sm = plain_rows(near, top)
    ch = changes_ref(idx)
    assert len(ch) == total
    if top == 1:
        assert np.diff(ch).max() == 995
    S = stream(near, top)
    got_idx, got_sum, ev = drive(S, "enqueue_device", near["bases"], near["offsets"], near["cuts"], top, 1, cap=700)
    S.close()
    np.testing.assert_array_equal(got_idx, idx)
    check_events(ev, near["cuts"], idx, sm, 700, what=f"top {top}")
    S = stream(near, top)
    ev = drive(S, "push", near["bases"], near["offsets"], [0, 700], top, 1, cap=700)[2]
    S.close()
    check_events(ev, [0, 700], idx, sm, 700, what=f"top {top} push")


@pytest.mark.parametrize("entry", ("push", "enqueue_device", "submit"))
def test_overflow(near, entry):
    """cap = 64 at top 17: the CPU oracle gives 85 / 113 / 90 / 58 change points per batch, so three of the four lists are truncated"""
    idx, sm = plain_rows(near, 17)
    per_batch = [len(changes_ref(idx[a:a + 700])) for a in near["cuts"][:-1]]
    assert sum(n > 64 for n in per_batch) == 3 and sum(n <= 64 for n in per_batch) == 1, per_batch
    S = stream(near, 17)
    got_idx, _, ev = drive(S, entry, near["bases"], near["offsets"], near["cuts"], 17, 1, cap=64)
    S.close()
    np.testing.assert_array_equal(got_idx, idx)
    assert [e["n"] for e in ev] == per_batch
    check_events(ev, near["cuts"], idx, sm, 64, what=entry)


def test_a_batch_cut_into_several_passes(near, tmp_path):
    """stream_query_rows = 64: the batch is ranked pass by pass, every pass flags its own reads and the first read of a later pass
    compares with the last row of the pass before.  A child process on the experiments build, which names the reads that begin a pass
    (SKX_DEBUG_PASS): among them the expected data must hold a change point and a read that is none."""
    top = 17  # (the passes begin at reads 144, 307, 477 and 624: at top 17 the last two are change points, the first two are not)
    idx, sm = plain_rows(near, top)
    idx, sm = idx[:700, 0], sm[:700, 0]
    src, dst = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    np.savez(src, ref=near["ref"]["ref"], col_len=near["ref"]["col_len"], bases=near["bases"][:int(near["offsets"][700])],
             offsets=near["offsets"][:701], top=top, cap=700)
    r = subprocess.run([sys.executable, WORKER, "passes", src, dst], env=exp_env(SKX_DEBUG_PASS=1), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    z = np.load(dst)
    cuts = [(int(a), int(b)) for a, b in re.findall(r"\[skx pass cut\] reads (\d+) (\d+)", r.stderr)]
    n_pass = len(cuts) // 2  # (the batch went through twice)
    assert cuts[:n_pass] == cuts[n_pass:] and cuts[0][0] == 0 and cuts[n_pass - 1][1] == 700
    assert int(z["push_passes"]) == n_pass > 1 and int(z["dev_passes"]) == n_pass
    want = changes_ref(idx)
    starts = {a for a, _ in cuts[:n_pass] if a > 0}
    assert starts & set(want.tolist()), "no pass begins at a change point: pick another seed"
    assert starts - set(want.tolist()), "every pass begins at a change point: pick another seed"
    for k in ("push", "dev"):
        np.testing.assert_array_equal(z[f"{k}_idx"], idx, err_msg=k)
        np.testing.assert_array_equal(z[f"{k}_sum"], sm, err_msg=k)
        n = int(z[f"{k}_n"].ravel()[0])
        assert n == len(want), k
        np.testing.assert_array_equal(z[f"{k}_read"][:n], want, err_msg=k)
        np.testing.assert_array_equal(z[f"{k}_ev_idx"][:n].reshape(n, top), idx[want], err_msg=k)
        np.testing.assert_array_equal(z[f"{k}_ev_sum"][:n].reshape(n, top), sm[want], err_msg=k)
    assert (z["dev_read"][len(want):] == SENT).all() and (z["dev_ev_sum"][len(want):] == SENT).all()


# ---------------------------------------------------------------- codes mode
@pytest.fixture(scope="module")
def small(gpu):
    """the fixture of tests/test_gpu_consensus.py: 600 genomes, s = 64, 2 800 reads of 200 to 400 bases, 16 genotype columns"""
    from sketchy_amd import api, synth
    ref = synth.make_reference(600, 64, rng_seed=901, device="numpy")
    bases, offsets = synth.make_reads(ref["genome"], 2800, 300, rng_seed=902, lognormal_sigma=0.4, min_len=200, max_len=400)
    codes = (np.random.default_rng(903).integers(0, 3, (600, 16)) * 1000 + 7).astype(np.uint32)
    R = api.ReferenceSketch(ref["ref"], ref["col_len"])
    R.set_genotypes(codes)
    S = api.SumOfSharedHashes(R, top=5, max_batch_reads=700, max_batch_bases=700 * 400)
    cuts = [0, 700, 1400, 2100, 2800]
    idx, sm, _ = drive(S, "push", bases, offsets, cuts, 5, 1)
    S.close()
    yield dict(R=R, ref=ref, bases=bases, offsets=offsets, codes=codes, cuts=cuts, idx=idx, sum=sm)
    R.close()


@pytest.mark.parametrize("bind_cons", (False, True), ids=("events_only", "with_consensus"))
@pytest.mark.parametrize("entry", ("push", "push_device", "enqueue_device", "submit"))
def test_codes_mode(small, entry, bind_cons):
    from sketchy_amd import api
    idx, sm, cuts = small["idx"], small["sum"], small["cuts"]
    call = consensus_ref(idx, small["codes"], [600])
    n_codes = [len(changes_ref(call[a:b])) for a, b in zip(cuts[:-1], cuts[1:])]
    n_idx = [len(changes_ref(idx[a:b])) for a, b in zip(cuts[:-1], cuts[1:])]
    assert sum(n_codes) < sum(n_idx) and sum(n > 1 for n in n_codes) >= 2, (n_codes, n_idx)
    S = api.SumOfSharedHashes(small["R"], top=5, max_batch_reads=700, max_batch_bases=700 * 400)
    got_idx, got_sum, ev = drive(S, entry, small["bases"], small["offsets"], cuts, 5, 1, n_feat=16, cap=700, codes=True, bind_cons=bind_cons)
    S.close()
    np.testing.assert_array_equal(got_idx, idx)
    assert [e["n"] for e in ev] == n_codes
    check_events(ev, cuts, idx, sm, 700, call=call, what=f"{entry} codes")


def test_three_species(gpu):
    from sketchy_amd import api
    sizes = (70, 129, 64)
    refs, bases, offsets = workload_species(sizes, 64, 900, read_len=300, rng_seed=931)
    R = api.ReferenceSketch([r["ref"] for r in refs])
    cuts = [0, 300, 600, 900]
    try:
        S0 = api.SumOfSharedHashes(R, top=3, max_batch_reads=300, max_batch_bases=300 * 300)
        idx, sm, _ = drive(S0, "push", bases, offsets, cuts, 3, 3)
        S0.close()
        diff = (idx[1:] != idx[:-1]).any(axis=2)  # [read, species]
        for sp in range(3):
            alone = diff[:, sp] & ~np.delete(diff, sp, axis=1).any(axis=1)
            assert alone.any(), f"no read changes the row of species {sp} alone"
        for entry in ("push", "enqueue_device", "submit"):
            S = api.SumOfSharedHashes(R, top=3, max_batch_reads=300, max_batch_bases=300 * 300)
            got_idx, got_sum, ev = drive(S, entry, bases, offsets, cuts, 3, 3, cap=300)
            S.close()
            np.testing.assert_array_equal(got_idx, idx)
            check_events(ev, cuts, idx, sm, 300, what=entry)
    finally:
        R.close()


def test_compact_ranking(gpu):
    """The truth-strain stream of test_gpu_consensus.test_compact_ranking: batches ranked on their candidates, whose rows go through
    launch_cand_rows_back before anything may compare them."""
    import tempfile
    from sketchy_amd import api
    from test_gpu_patterns import B, NB, _generate
    d = tempfile.mkdtemp(prefix="skx_chg_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    try:
        _generate(d)
        ref, bases, offsets = np.load(d + "/ref.npy"), np.load(d + "/bases.npy"), np.load(d + "/offsets.npy")
    finally:
        for f in os.listdir(d):
            os.remove(os.path.join(d, f))
        os.rmdir(d)
    R = api.ReferenceSketch(ref)
    try:
        cuts = [i * B for i in range(NB + 1)]
        cap_b = int(np.max(offsets[B::B] - offsets[:-B:B]))
        S0 = api.SumOfSharedHashes(R, top=3, max_batch_reads=B, max_batch_bases=cap_b)
        idx, sm, _ = drive(S0, "enqueue_device", bases, offsets, cuts, 3, 1)
        S0.close()
        S = api.SumOfSharedHashes(R, top=3, max_batch_reads=B, max_batch_bases=cap_b)
        got_idx, got_sum, ev = drive(S, "enqueue_device", bases, offsets, cuts, 3, 1, cap=256)
        st = S.stats()
        S.close()
        assert st["batches_compact"] >= 1, st
        np.testing.assert_array_equal(got_idx, idx)
        np.testing.assert_array_equal(got_sum, sm)
        check_events(ev, cuts, idx, sm, 256, what="compact")
    finally:
        R.close()


# ---------------------------------------------------------------- errors, one-shot, empty batches
def test_errors_and_the_one_shot_binding(small):
    from sketchy_amd import _lib, api
    L = _lib.load()
    b, o = small["bases"], small["offsets"]
    S = api.SumOfSharedHashes(small["R"], top=5, max_batch_reads=700, max_batch_bases=700 * 400)
    n_ev, ev_read = np.full(1, SENT, np.uint32), np.full(8, SENT, np.uint32)
    # at bind time
    assert L.skx_stream_bind_changes(None, 8, _p(n_ev), _p(ev_read), None, None, None) == _lib.ERR_INVALID
    assert L.skx_stream_bind_changes(S._h, 0, _p(n_ev), _p(ev_read), None, None, None) == _lib.ERR_INVALID
    assert L.skx_stream_bind_changes(S._h, 8, None, _p(ev_read), None, None, None) == _lib.ERR_INVALID
    assert L.skx_stream_bind_changes(S._h, 8, _p(n_ev), None, None, None, None) == _lib.ERR_INVALID
    first = S.push(b, o[:101])  # (nothing of the above bound anything)
    assert n_ev[0] == SENT and (ev_read == SENT).all()
    # one-shot: the second batch writes nothing into the arrays of the first
    S.reset()
    got = S.push(b, o[:101], want_changes=100)
    want = changes_ref(first["topk_idx"])
    assert got["changes"]["n"] == len(want) and got["changes"]["read"].tolist() == want.tolist()
    np.testing.assert_array_equal(got["changes"]["idx"], first["topk_idx"][want])
    np.testing.assert_array_equal(got["changes"]["sum"], first["topk_sum"][want])
    S.bind_changes(8, _p(n_ev), _p(ev_read))
    S.push(b, o[100:201])
    n_first, reads_first = int(n_ev[0]), ev_read.copy()
    assert n_first >= 1 and reads_first[0] == 0
    S.push(b, o[200:301])
    assert int(n_ev[0]) == n_first and (ev_read == reads_first).all()
    # an empty batch
    n_ev[:] = SENT
    S.bind_changes(8, _p(n_ev), _p(ev_read))
    S.push(b, o[:1])
    assert n_ev[0] == 0 and (ev_read == reads_first).all()
    d_b, d_o = api.DeviceBuffer.from_numpy(b), api.DeviceBuffer.from_numpy(np.ascontiguousarray(o[300:401]))
    d_n, d_r, d_i = api.DeviceBuffer.from_numpy(n_ev), api.DeviceBuffer.from_numpy(ev_read), api.DeviceBuffer(100 * 5 * 4)
    try:
        for fn in (S.push_device, S.enqueue_device):
            _lib.check(L.skx_dev_upload(0, d_n.ptr, _p(np.full(1, SENT, np.uint32)), 4))
            fn(d_b.ptr, d_o.ptr, 0, 0, d_i.ptr, None, changes=(8, d_n.ptr, d_r.ptr))
            S.sync()
            assert d_n.to_numpy(np.uint32, 1)[0] == 0
        # a _device entry point without its own row array: refused, and the binding is gone
        _lib.check(L.skx_dev_upload(0, d_n.ptr, _p(np.full(1, SENT, np.uint32)), 4))
        for fn in (L.skx_stream_push_device, L.skx_stream_enqueue_device):
            S.bind_changes(8, d_n.ptr, d_r.ptr)
            assert fn(S._h, d_b.ptr, d_o.ptr, 100, int(o[400] - o[300]), None, None) == _lib.ERR_INVALID
            assert "d_topk_idx" in L.skx_last_error().decode()
        reads = S.reads
        S.push_device(d_b.ptr, d_o.ptr, 100, int(o[400] - o[300]), None, None)  # unbound now: as ever, and no events anywhere
        S.sync()
        assert S.reads == reads + 100 and d_n.to_numpy(np.uint32, 1)[0] == SENT
    finally:
        for d in (d_b, d_o, d_n, d_r, d_i):
            d.free()
    S.close()
    # a stream without a ranking: binding succeeds, the batch call fails and consumes it
    n_ev[:] = SENT
    S = api.SumOfSharedHashes(small["R"], top=0, max_batch_reads=700, max_batch_bases=700 * 400)
    S.bind_changes(8, _p(n_ev), _p(ev_read))
    with pytest.raises(_lib.SketchyHipError) as e:
        S.push(b, o[:101])
    assert e.value.code == _lib.ERR_INVALID and "top_k" in str(e.value) and S.reads == 0
    S.push(b, o[:101])
    assert S.reads == 100 and n_ev[0] == SENT
    hb = api.HostBuffer(len(b))
    ho = api.HostBuffer(101 * 8)
    hb.view(np.uint8)[:] = b
    ho.view(np.uint64)[:] = o[:101]
    S.bind_changes(8, _p(n_ev), _p(ev_read))
    with pytest.raises(_lib.SketchyHipError) as e:
        S.submit(hb.ptr, ho.ptr, 100)
    assert e.value.code == _lib.ERR_INVALID and "top_k" in str(e.value)
    S.drain()
    S.close()
    hb.free()
    ho.free()
    # codes mode on a reference without a genotype table
    R = api.ReferenceSketch(small["ref"]["ref"], small["ref"]["col_len"])
    S = api.SumOfSharedHashes(R, top=5, max_batch_reads=700, max_batch_bases=700 * 400)
    ev_codes = np.full((8, 16), SENT, np.uint32)
    S.bind_changes(8, _p(n_ev), _p(ev_read), None, None, _p(ev_codes))
    with pytest.raises(_lib.SketchyHipError) as e:
        S.push(b, o[:101])
    assert e.value.code == _lib.ERR_INVALID and "genotype table" in str(e.value)
    got = S.push(b, o[:101])
    np.testing.assert_array_equal(got["topk_idx"], first["topk_idx"])
    assert n_ev[0] == SENT and (ev_codes == SENT).all()
    S.close()
    R.close()


# ---------------------------------------------------------------- the CLI with the real library
def _cli(*args):
    p = subprocess.run([BIN, *args], capture_output=True)
    return p.returncode, p.stdout.decode(), p.stderr.decode()


@pytest.fixture(scope="module")
def cli_inputs(tmp_path_factory):
    """the first sample of tests/test_gpu_rank_sketches.py::cli_inputs (5 000 reads of 400 bases against 64 genomes, s = 1000), as a
    mapped FASTQ and -- a sequential stream: batches of exactly -b reads -- gzipped"""
    d = tmp_path_factory.mktemp("changes_cli")
    ref, bases, offsets = workload(64, 1000, 5701, read_len=400, genome_len=40000, rng_seed=77)
    names = [f"genome{i:02d}.fa" for i in range(64)]
    msh, tsv = str(d / "ref.msh"), str(d / "geno.tsv")
    write_msh(msh, names, ref["ref"], kmer=16, seed=0, lengths=[40000] * 64)
    with open(tsv, "w") as f:
        f.write("id\tmlst\n" + "".join(f"{nm}\tST{i % 7}\n" for i, nm in enumerate(names)))
    text = "".join(f"@r{i}\n{r.decode()}\n+\n{'I' * len(r)}\n" for i, r in enumerate(unpack_reads(bases, offsets)[:5000]))
    fq, gz = str(d / "sample0.fq"), str(d / "sample0.fq.gz")
    open(fq, "w").write(text)
    with gzip.open(gz, "wt", compresslevel=1) as f:
        f.write(text)
    return msh, tsv, fq, gz


@pytest.mark.parametrize("args", (("-t", "1"), ("-t", "5"), ("-c", "-t", "5")), ids=("top1", "top5", "consensus_top5"))
def test_cli_changes_prints_the_filtered_stream(gpu, cli_inputs, args):
    msh, tsv, fq, gz = cli_inputs
    assert "skx_stream_bind_changes" in subprocess.check_output(["nm", "-D", "--undefined-only", BIN], text=True)
    top = 1 if "-c" in args else int(args[-1])
    base = ("predict", "-s", "-r", msh, "-g", tsv, *args)
    rc, full, err = _cli(*base, "-i", fq, "-b", "512")
    assert rc == 0 and full.count("\n") == 5000 * top, err
    want, kept = filter_changes(full, top)
    assert 1 <= len(kept) < 5000
    # 5 000 reads in batches of exactly 250 (the gzipped input): at least three batches, one of which begins at a read that is no
    # change point -- there the writer must drop the batch's first event
    starts = set(range(0, 5000, 250))
    assert len(starts) >= 3 and starts - set(kept), "every batch begins at a change point: pick another batch size"
    for extra in (("-i", gz, "-b", "250", "--changes"), ("-i", fq, "-b", "512", "-x"), ("-i", fq, "-b", "100000", "-x"),
                  ("-i", gz, "-b", "250", "-x", "-H")):
        rc, got, err = _cli(*base, *extra)
        assert rc == 0, err
        header = "reads\tsketch_id\tshared_hashes\tmlst\n" if "-H" in extra else ""
        assert got == header + want, extra
