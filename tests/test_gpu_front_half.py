"""The front half of a deferred pass -- row counts, gains, tables, candidates, the compact matrices' rare rows -- behind ONE clear
(skx_kernels.hip, pass_clear_kernel) that zeroes the per-row arrays and the compact matrices only as far as their slot's last use
dirtied them: every row of every batch and the final table against oracle.stream_fast (src/sketchy.rs:337-349), through every order
of large and small passes, resets and forced-full passes in which a stale row beyond an extent would show.

Shapes: SURVEY 8(d)'s SNP reference in small -- N = 3000 genomes, s = 1000, 15 lineages of 200, reads of the truth strain, batches of
4096 reads: the smallest at which all row classes exist together (a species of more than kCandCap = 1024 genomes: static dense
dictionary and a legacy first pass; lineages of more than 8 genomes: bit rows and patterns; short lists).  They reach the compact
ranking (8-20 compact batches per case on an MI355X); every case asserts from the stream's statistics that shared passes and compact
rankings really happened.

Two cases of the plan cannot be driven through the library's entry points as worded, and use the nearest thing that can:
 * the per-read shared counts (which force a batch's ranking onto the full matrix) can only be bound by a synchronous push, and a
   push is a pass of its own -- so the forced-full batches are passes BETWEEN shared passes of one stream, not batches inside one;
 * the query-row capacity only regrows when a pass has more distinct hashes than the initial 65 536 rows, which a reference of
   3000 x 1000 hashes cannot supply (a batch cannot exceed max_batch_reads either) -- the case alternates pushes of very different
   sizes and resets instead, which is how test_gpu_patterns.py::test_rare_rows_stay_exact_through_stride_changes_and_resets changes a
   buffer set's row stride; the regrow itself happens in bench.py's C2 stream (query_rows_grown = 1), whose rows its oracle check
   compares."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
N, S_, LIN, B, NB = 3000, 1000, 15, 4096, 17   # (17 batches: 14 of a sample + what the large-small-large case reads beyond them)
N2 = 1500                                       # genomes per species of the two-species case
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _generate(d):
    # (in a child: torch's bundled HIP runtime and the library's do not share a process, as in the other GPU tests)
    code = (
        "import sys, numpy as np; sys.path.insert(0, %r)\n"
        "import torch\n"
        "from sketchy_amd import synth\n"
        "def reads(src, n_batches, b, seed):\n"
        "    parts, lens = [], []\n"
        "    for i in range(n_batches):\n"
        "        x, o = synth.make_reads_torch(src, b, 1500, rng_seed=seed + i, device='cuda')\n"
        "        parts.append(x.cpu().numpy()); lens.append(np.diff(o.cpu().numpy().astype(np.int64)))\n"
        "    return parts, lens\n"
        "def pack(parts, lens):\n"
        "    offsets = np.zeros(1 + sum(len(x) for x in lens), np.uint64)\n"
        "    offsets[1:] = np.cumsum(np.concatenate(lens)).astype(np.uint64)\n"
        "    return np.concatenate(parts), offsets\n"
        "d = %r\n"
        "ref = synth.make_reference(%d, %d, rng_seed=3, device='cuda', mode='snp', n_lineages=%d)\n"
        "bases, offsets = pack(*reads(torch.from_numpy(ref['truth_genome']).to('cuda'), %d, %d, 4100))\n"
        "np.save(d + '/ref.npy', ref['ref']); np.save(d + '/bases.npy', bases); np.save(d + '/offsets.npy', offsets)\n"
        "np.save(d + '/truth.npy', np.array([ref['truth_index']]))\n"
        # two species: a SNP reference each, the reads of both truth strains interleaved read by read
        "rs = [synth.make_reference(%d, %d, rng_seed=11 + 7 * i, device='cuda', mode='snp', n_lineages=10) for i in range(2)]\n"
        "two = [reads(torch.from_numpy(r['truth_genome']).to('cuda'), 5, %d, 5100 + 100 * i) for i, r in enumerate(rs)]\n"
        "rl = [[np.split(p, np.cumsum(l)[:-1]) for p, l in zip(*t)] for t in two]\n"
        "mixed = [x for j in range(5) for pair in zip(rl[0][j], rl[1][j]) for x in pair]\n"
        "b2, o2 = pack(mixed, [np.array([len(x) for x in mixed])])\n"
        "np.save(d + '/ref2a.npy', rs[0]['ref']); np.save(d + '/ref2b.npy', rs[1]['ref'])\n"
        "np.save(d + '/bases2.npy', b2); np.save(d + '/offsets2.npy', o2)\n"
    ) % (ROOT, d, N, S_, LIN, NB, B, N2, S_, B // 2)
    subprocess.check_call([sys.executable, "-c", code])


@pytest.fixture(scope="module")
def snp(gpu):
    d = tempfile.mkdtemp(prefix="skx_fh_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    try:
        _generate(d)
        out = {k: np.load(f"{d}/{k}.npy") for k in ("ref", "bases", "offsets", "ref2a", "ref2b", "bases2", "offsets2")}
        out["truth"] = int(np.load(d + "/truth.npy")[0])
    finally:
        for f in os.listdir(d):
            os.remove(os.path.join(d, f))
        os.rmdir(d)
    from sketchy_amd import api
    out["R"] = api.ReferenceSketch(out["ref"])
    out["memo"] = {}
    yield out
    out["R"].close()


def _expect(snp, bounds, top):
    """the oracle's rows of the batches [bounds[i], bounds[i + 1]) of one sample, each computed once per (history, top)"""
    from oracle import oracle as orc
    memo, cum, out = snp["memo"], None, []
    for i in range(len(bounds) - 1):
        key = (top, tuple(bounds[:i + 2]))
        if key not in memo:
            memo[key] = orc.stream_fast(16, 0, S_, snp["ref"], None, snp["bases"], snp["offsets"][bounds[i]:bounds[i + 1] + 1],
                                        top_k=max(top, 1), cum=cum, rows=True)
        out.append(memo[key])
        cum = memo[key]["cum"]
    return out


class _Run:
    """one stream over the fixture's reads; enqueue() queues the batches of `bounds`, rows() fetches what they wrote"""

    def __init__(self, snp, top, max_reads=B):
        from sketchy_amd import api
        self.api, self.snp, self.top = api, snp, top
        off = snp["offsets"]
        self.S = api.SumOfSharedHashes(snp["R"], top=top, max_batch_reads=max_reads, max_batch_bases=int(np.max(off[max_reads:] - off[:-max_reads])))
        self.d_b = api.DeviceBuffer.from_numpy(snp["bases"])
        self.bufs = []

    def enqueue(self, bounds):
        off, top = self.snp["offsets"], self.top
        first = len(self.bufs)
        for a, b in zip(bounds[:-1], bounds[1:]):
            n = b - a
            d_o = self.api.DeviceBuffer.from_numpy(np.ascontiguousarray(off[a:b + 1]))
            d_i = self.api.DeviceBuffer(n * top * 4) if top else None
            d_s = self.api.DeviceBuffer(n * top * 8) if top else None
            self.bufs.append((n, d_o, d_i, d_s))
            self.S.enqueue_device(self.d_b.ptr, d_o.ptr, n, int(off[b] - off[a]), d_i.ptr if top else None, d_s.ptr if top else None)
        return first

    def check(self, first, exp, what):
        for j, e in enumerate(exp):
            n, _, d_i, d_s = self.bufs[first + j]
            np.testing.assert_array_equal(d_s.to_numpy(np.uint64, (n, self.top)), e["topk_sum"], err_msg=f"{what}: sums of batch {j}")
            np.testing.assert_array_equal(d_i.to_numpy(np.uint32, (n, self.top)), e["topk_idx"], err_msg=f"{what}: genomes of batch {j}")

    def close(self):
        self.d_b.free()
        for t in self.bufs:
            for x in t[1:]:
                if x is not None:
                    x.free()
        self.S.close()


def _reached_the_compact_path(st):
    print("stats:", st)
    assert st["passes_shared"] >= 2, st
    assert st["batches_compact"] >= 2, st


def _even(n_batches, b=B, start=0):
    return [start + i * b for i in range(n_batches + 1)]


@pytest.mark.parametrize("top", [1, 3])
def test_fourteen_batches_back_to_back(snp, top):
    """deferred passes of eight batches and the closing pass of the rest"""
    bounds = _even(14)
    run = _Run(snp, top)
    try:
        run.enqueue(bounds)
        run.S.sync()
        exp = _expect(snp, bounds, top)
        run.check(0, exp, "14 batches")
        np.testing.assert_array_equal(run.S.table(), exp[-1]["cum"], err_msg="final table")
        assert int(np.argmax(exp[-1]["cum"])) == snp["truth"]
        _reached_the_compact_path(run.S.stats())
    finally:
        run.close()


def test_closing_passes_of_every_size(snp):
    """the sample cut off after 9, 10, 11 and 14 batches: closing passes of 1, 2, 3 and 6 batches, with nothing sketched beside them"""
    run = _Run(snp, 1)
    try:
        for nb in (9, 10, 11, 14):
            bounds = _even(nb)
            first = run.enqueue(bounds)
            run.S.sync()
            exp = _expect(snp, bounds, 1)
            run.check(first, exp, f"sample of {nb} batches")
            np.testing.assert_array_equal(run.S.table(), exp[-1]["cum"], err_msg=f"table after {nb} batches")
            run.S.reset()
        _reached_the_compact_path(run.S.stats())
    finally:
        run.close()


def test_large_then_small_then_large_passes(snp):
    """eight batches of 4096 reads, eight of 256, eight of 4096 on one stream: whatever a small pass leaves untouched of the arrays a
    large one filled must not show in the next large one"""
    bounds = _even(8) + [8 * B + 256 * i for i in range(1, 9)]
    bounds += [bounds[-1] + B * i for i in range(1, 9)]
    assert bounds[-1] <= NB * B
    run = _Run(snp, 1)
    try:
        run.enqueue(bounds)
        run.S.sync()
        exp = _expect(snp, bounds, 1)
        run.check(0, exp, "large, small, large")
        np.testing.assert_array_equal(run.S.table(), exp[-1]["cum"], err_msg="final table")
        _reached_the_compact_path(run.S.stats())
    finally:
        run.close()


def test_reset_in_the_middle_then_the_sample_again_twice(snp):
    bounds = _even(14)
    exp = _expect(snp, bounds, 1)
    run = _Run(snp, 1)
    try:
        run.enqueue(_even(5))   # (a sample abandoned half-way)
        run.S.reset()
        for rep in range(2):
            first = run.enqueue(bounds)
            run.S.sync()
            run.check(first, exp, f"repetition {rep}")
            np.testing.assert_array_equal(run.S.table(), exp[-1]["cum"], err_msg=f"table of repetition {rep}")
            run.S.reset()
        _reached_the_compact_path(run.S.stats())
    finally:
        run.close()


def test_pushes_of_very_different_sizes_and_resets_between_shared_passes(snp):
    """(the module docstring's second note) shared passes, then pushes that change the buffer sets' row stride, a reset, shared passes
    again"""
    from oracle import oracle as orc
    ref, bases, off = snp["ref"], snp["bases"], snp["offsets"]
    run = _Run(snp, 1)
    try:
        bounds = _even(10)
        first = run.enqueue(bounds)
        run.S.sync()
        exp = _expect(snp, bounds, 1)
        run.check(first, exp, "before the pushes")
        cum, pos = exp[-1]["cum"], bounds[-1]
        for n in (B, 300, 64, B, 257, 1):
            cut = np.ascontiguousarray(off[pos:pos + n + 1])
            got = run.S.push(bases, cut)
            e = orc.stream_fast(16, 0, S_, ref, None, bases, cut, top_k=1, cum=cum, rows=True)
            cum = e["cum"]
            np.testing.assert_array_equal(got["topk_sum"], e["topk_sum"], err_msg=f"push of {n} at read {pos}")
            np.testing.assert_array_equal(got["topk_idx"], e["topk_idx"], err_msg=f"push of {n} at read {pos}")
            pos += n
        np.testing.assert_array_equal(run.S.table(), cum)
        run.S.reset()
        bounds = _even(14)
        first = run.enqueue(bounds)
        run.S.sync()
        exp = _expect(snp, bounds, 1)
        run.check(first, exp, "after the pushes")
        np.testing.assert_array_equal(run.S.table(), exp[-1]["cum"], err_msg="final table")
        st = run.S.stats()
        print("query rows grown:", st["query_rows_grown"])
        _reached_the_compact_path(st)
    finally:
        run.close()


def test_forced_full_batches_between_compact_passes(snp):
    """(the module docstring's first note) two pushes that bind the per-read shared counts -- they rank on everything -- between the
    shared passes of one sample, whose later batches rank compactly"""
    from oracle import oracle as orc
    ref, bases, off = snp["ref"], snp["bases"], snp["offsets"]
    col = np.full(N, S_, np.uint32)
    run = _Run(snp, 1)
    try:
        bounds = _even(8)
        first = run.enqueue(bounds)
        run.S.sync()
        exp = _expect(snp, bounds, 1)
        run.check(first, exp, "before")
        cum, pos = exp[-1]["cum"], bounds[-1]
        for n in (200, 130):
            cut = np.ascontiguousarray(off[pos:pos + n + 1])
            got = run.S.push(bases, cut, want_shared=True)
            e = orc.stream(16, 0, S_, ref, col, bases, cut, top_k=1, want_shared=True, cum=cum)
            cum = e["cum"]
            np.testing.assert_array_equal(got["shared"], e["shared"], err_msg=f"shared counts of the push of {n}")
            np.testing.assert_array_equal(got["topk_sum"], e["topk_sum"], err_msg=f"push of {n}")
            np.testing.assert_array_equal(got["topk_idx"], e["topk_idx"], err_msg=f"push of {n}")
            pos += n
        bounds = _even(8, start=pos)
        first = run.enqueue(bounds)
        run.S.sync()
        for j in range(8):
            cut = off[bounds[j]:bounds[j + 1] + 1]
            e = orc.stream_fast(16, 0, S_, ref, None, bases, cut, top_k=1, cum=cum, rows=True)
            cum = e["cum"]
            run.check(first + j, [e], f"after, batch {j}")
        np.testing.assert_array_equal(run.S.table(), cum, err_msg="final table")
        _reached_the_compact_path(run.S.stats())
    finally:
        run.close()


def test_a_batch_that_meets_nothing_in_the_reference(snp):
    """a batch of reads of N's among the batches of a shared pass, and one in a pass of its own (P == 0) between two shared passes"""
    from oracle import oracle as orc
    from sketchy_amd import api
    ref, off = snp["ref"], snp["offsets"]
    n_n = 512
    nb = np.full(n_n * 300, ord("N"), np.uint8)
    no = np.arange(n_n + 1, dtype=np.uint64) * 300
    run = _Run(snp, 1)
    d_nb, d_no = api.DeviceBuffer.from_numpy(nb), api.DeviceBuffer.from_numpy(no)
    outs = []

    def enqueue_n():
        d_i, d_s = api.DeviceBuffer(n_n * 4), api.DeviceBuffer(n_n * 8)
        outs.append((d_i, d_s))
        run.S.enqueue_device(d_nb.ptr, d_no.ptr, n_n, int(no[-1]), d_i.ptr, d_s.ptr)

    try:
        bounds = _even(14)
        exp = _expect(snp, bounds, 1)
        run.enqueue(bounds[:5])          # batches 0 .. 3
        enqueue_n()                      # ... the empty one among them
        run.enqueue(bounds[4:9])         # 4 .. 7
        run.S.sync()
        enqueue_n()                      # a pass of its own
        run.S.sync()
        run.enqueue(bounds[8:])          # 8 .. 13
        run.S.sync()
        run.check(0, exp, "around the empty batches")
        for k, at in enumerate((4, 8)):  # the empty batches' rows: the table's leader as it stood, at every read
            e = orc.stream_fast(16, 0, S_, ref, None, nb, no, top_k=1, cum=exp[at - 1]["cum"], rows=True)
            np.testing.assert_array_equal(e["cum"], exp[at - 1]["cum"])
            np.testing.assert_array_equal(outs[k][1].to_numpy(np.uint64, (n_n, 1)), e["topk_sum"], err_msg=f"empty batch {k}: sums")
            np.testing.assert_array_equal(outs[k][0].to_numpy(np.uint32, (n_n, 1)), e["topk_idx"], err_msg=f"empty batch {k}: genomes")
        np.testing.assert_array_equal(run.S.table(), exp[-1]["cum"], err_msg="final table")
        _reached_the_compact_path(run.S.stats())
    finally:
        for t in outs:
            t[0].free(); t[1].free()
        d_nb.free(); d_no.free()
        run.close()


def test_unranked_stream_table_only(snp):
    """top = 0: no rows, no candidates (the pass zeroes the candidate counts instead) -- the table alone"""
    bounds = _even(14)
    run = _Run(snp, 0)
    try:
        run.enqueue(bounds)
        run.S.sync()
        np.testing.assert_array_equal(run.S.table(), _expect(snp, bounds, 1)[-1]["cum"], err_msg="final table")
        st = run.S.stats()
        print("stats:", st)
        assert st["passes_shared"] >= 2, st   # (an unranked stream has no rankings, compact or other)
    finally:
        run.close()


def test_two_species(snp):
    """two SNP references of 1500 genomes each in one matrix, the reads of both truth strains interleaved: the dense rows' gains read
    only their own species' words (segw), the compact matrices have two groups per species"""
    from oracle import oracle as orc
    from sketchy_amd import api
    refs, bases, off = [snp["ref2a"], snp["ref2b"]], snp["bases2"], snp["offsets2"]
    nb = 10
    n = (len(off) - 1) // nb
    R = api.ReferenceSketch(refs)
    S = api.SumOfSharedHashes(R, top=1, max_batch_reads=n, max_batch_bases=int(np.max(off[n:] - off[:-n])))
    d_b = api.DeviceBuffer.from_numpy(bases)
    bufs = []
    try:
        assert R.n_species == 2 and R.static_dense[0]
        for i in range(nb):
            d_o = api.DeviceBuffer.from_numpy(np.ascontiguousarray(off[i * n:(i + 1) * n + 1]))
            d_i, d_s = api.DeviceBuffer(n * 2 * 4), api.DeviceBuffer(n * 2 * 8)
            bufs.append((d_o, d_i, d_s))
            S.enqueue_device(d_b.ptr, d_o.ptr, n, int(off[(i + 1) * n] - off[i * n]), d_i.ptr, d_s.ptr)
        S.sync()
        cums = None
        for i in range(nb):
            e = orc.stream_fast_species(16, 0, S_, refs, bases, off[i * n:(i + 1) * n + 1], top_k=1, cums=cums)
            cums = e["cums"]
            np.testing.assert_array_equal(bufs[i][2].to_numpy(np.uint64, (n, 2, 1)), e["topk_sum"], err_msg=f"sums of batch {i}")
            np.testing.assert_array_equal(bufs[i][1].to_numpy(np.uint32, (n, 2, 1)), e["topk_idx"], err_msg=f"genomes of batch {i}")
        np.testing.assert_array_equal(S.table(), np.concatenate(cums), err_msg="final tables")
        _reached_the_compact_path(S.stats())
    finally:
        d_b.free()
        for t in bufs:
            for x in t:
                x.free()
        S.close()
        R.close()
