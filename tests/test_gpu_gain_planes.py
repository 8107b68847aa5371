"""The dense rows' gains as an int8 matrix product (skx_kernels.hip: gain_operand_kernel, gain_dense_mfma_kernel): a row's count goes
into the product as 7-bit planes -- planes 0 and 1 in one operand (counts below 2^14), planes 2 and 3 in a second one that is issued
only for the words that hold such a count.  The counts are made known here: a batch of c copies of ONE short read of the truth
strain that holds a hash most genomes of the reference have (a dense row: the reference's 22 807 distinct hashes are held by one
genome, by a few, by the 200 of a lineage -- the index's lists -- or by 1000 and more, which stay with the scan) gives that row the count
c, and the oracle's table must rise by c times the read's shared hashes for every genome -- the cases assert that from the oracle
before they compare the device's rows and table with it.  c = 127, 128, 129 (the first plane boundary), 16 383 and 16 384 (the
second pair), 2^20 (the high bits of plane 2).

On the recipe and the data of test_gpu_front_half.py (SNP reference N = 3000, s = 1000, 15 lineages of 200, batches of 4096 reads
of the truth strain; every row of every batch and the final table against oracle.stream_fast), the repeated reads as batches of
their own among the sample's.  A fresh sample's first pass takes six batches and leaves the table to its ranking chains (no gains);
the repeated reads come behind it: in a pass of 8 followed by one of 6 (first boundary), in a pass of 8 followed by one of 1 (second
pair) -- both cases assert the number of passes; the 2^20 case does not depend on how its batches are grouped.  N = 3000 is no
multiple of 64: the last workgroup of the gain kernel has pad genomes.  stats() gives the dense rows of the most recent pass
("dictionary_dense"): the first case asserts that they are no multiple of 64 (a partly used last word) and that their words are no
multiple of the four waves a workgroup splits them over.  The two-species case reads only its own species' words (segw).  The
pattern matrix goes through the same launcher in every pass of these streams (the rows with a pattern list are the lineages'):
the rows and tables cover it.  Not reached by any small case: the split-array scan (m_int), which needs ~192 rows per band of
dense query words -- the launcher leaves that path on the bit-by-bit kernel.

Which kernel ran is not visible in rows that are right either way: the last case runs a stream with a batch of 16 384 copies twice in
the experiments build, with and without SKX_GAIN_MFMA=0, and reads that build's launch counters (skx_debug_gain_launches): every
dense-gain launch of the first run took the int8 product, every one of the second the bit-by-bit kernel -- which stays in the
library for the calls the launcher declines and is under test here again --, and both runs give the same rows and table."""
import subprocess
import sys

import numpy as np
import pytest

from helpers import ROOT, exp_env

from test_gpu_front_half import B, N, S_, _reached_the_compact_path, snp  # noqa: F401  (snp: that module's data, generated once here)

pytestmark = pytest.mark.gpu
READ = 100  # bases of the repeated read


@pytest.fixture(scope="module")
def short_read(snp):
    """(bases of a 100-base window of the sample's first reads that shares a hash with more than half of the genomes, its shared
    hashes per genome)"""
    from oracle import oracle as orc
    n_c = 256
    o0 = int(snp["offsets"][0])
    cand = np.ascontiguousarray(snp["bases"][o0:o0 + n_c * READ])
    off = np.arange(n_c + 1, dtype=np.uint64) * READ
    sh = orc.stream(16, 0, S_, snp["ref"], np.full(N, S_, np.uint32), cand, off, top_k=1, want_shared=True)["shared"]
    ok = np.flatnonzero((sh > 0).sum(axis=1) > N // 2)
    assert len(ok), "no window of the first reads holds a hash of most genomes"
    i = int(ok[0])
    return cand[i * READ:(i + 1) * READ].copy(), sh[i].astype(np.uint64)


class _Mixed:
    """a stream over the sample's batches with batches of repeated reads among them, and the oracle's chain beside it"""

    def __init__(self, snp, max_reads):
        from sketchy_amd import api
        off = snp["offsets"]
        self.snp, self.api = snp, api
        self.S = api.SumOfSharedHashes(snp["R"], top=1, max_batch_reads=max_reads,
                                       max_batch_bases=max(max_reads * READ, int(np.max(off[B:] - off[:-B]))))
        self.d_b = api.DeviceBuffer.from_numpy(snp["bases"])
        self.exp, self.out, self.cum, self.keep = [], [], None, [self.d_b]

    def sample(self, a, b):
        """the sample's batches a .. b - 1"""
        from oracle import oracle as orc
        snp, off, api = self.snp, self.snp["offsets"], self.api
        for j in range(a, b):
            cut = np.ascontiguousarray(off[j * B:(j + 1) * B + 1])
            d_o, d_i, d_s = api.DeviceBuffer.from_numpy(cut), api.DeviceBuffer(B * 4), api.DeviceBuffer(B * 8)
            self.keep += [d_o, d_i, d_s]
            self.S.enqueue_device(self.d_b.ptr, d_o.ptr, B, int(cut[-1] - cut[0]), d_i.ptr, d_s.ptr)
            e = orc.stream_fast(16, 0, S_, snp["ref"], None, snp["bases"], cut, top_k=1, cum=self.cum, rows=True)
            self.cum = e["cum"]
            self.exp.append(e)
            self.out.append((d_o, d_i, d_s))

    def copies(self, read, shared, c):
        """one batch of c copies of `read`: the table rises by c x shared, exactly"""
        from oracle import oracle as orc
        api = self.api
        bases = np.tile(read, c)
        off = np.arange(c + 1, dtype=np.uint64) * len(read)
        e = orc.stream_fast(16, 0, S_, self.snp["ref"], None, bases, off, top_k=1, cum=self.cum, rows=True)
        before = np.zeros(N, np.uint64) if self.cum is None else self.cum
        np.testing.assert_array_equal(e["cum"] - before, shared * np.uint64(c), err_msg=f"the oracle's gain of {c} copies")
        self.cum = e["cum"]
        d_b, d_o = api.DeviceBuffer.from_numpy(bases), api.DeviceBuffer.from_numpy(off)
        d_i, d_s = api.DeviceBuffer(c * 4), api.DeviceBuffer(c * 8)
        self.keep += [d_b, d_o, d_i, d_s]
        self.S.enqueue_device(d_b.ptr, d_o.ptr, c, int(off[-1]), d_i.ptr, d_s.ptr)
        self.exp.append(e)
        self.out.append((d_o, d_i, d_s))

    def check(self):
        self.S.sync()
        for j, (e, (_, d_i, d_s)) in enumerate(zip(self.exp, self.out)):
            n = len(e["topk_sum"])
            np.testing.assert_array_equal(d_s.to_numpy(np.uint64, (n, 1)), e["topk_sum"], err_msg=f"sums of batch {j}")
            np.testing.assert_array_equal(d_i.to_numpy(np.uint32, (n, 1)), e["topk_idx"], err_msg=f"genomes of batch {j}")
        np.testing.assert_array_equal(self.S.table(), self.cum, err_msg="final table")
        st = self.S.stats()
        _reached_the_compact_path(st)
        return st

    def close(self):
        for x in self.keep:
            x.free()
        self.S.close()


def test_first_plane_boundary(snp, short_read):
    """127, 128 and 129 copies in a pass of eight batches, a closing pass of six; the dense rows end inside a word, their words inside
    a round of the four waves"""
    m = _Mixed(snp, B)
    try:
        m.sample(0, 6)
        for c in (127, 128, 129):
            m.copies(*short_read, c)
        m.sample(6, 17)
        st = m.check()
        assert st["passes"] == 3, st
        nd = st["dictionary_dense"]
        print("dense rows:", nd)
        assert nd % 64 != 0 and ((nd + 63) // 64) % 4 != 0, nd
    finally:
        m.close()


def test_second_plane_pair(snp, short_read):
    """16 383 and 16 384 copies among six batches of the sample: a pass whose second operand one word needs; a closing pass of one"""
    m = _Mixed(snp, 16384)
    try:
        m.sample(0, 9)
        m.copies(*short_read, 16383)
        m.copies(*short_read, 16384)
        m.sample(9, 13)
        st = m.check()
        assert st["passes"] == 3, st   # (6, then 8 with the copies among them, then 1)
    finally:
        m.close()


def test_one_row_at_two_to_the_twenty(snp, short_read):
    """2^20 copies in one batch behind the first pass, seven batches of the sample behind it"""
    m = _Mixed(snp, 1 << 20)
    try:
        m.sample(0, 6)
        m.copies(*short_read, 1 << 20)
        m.sample(6, 13)
        m.check()
    finally:
        m.close()


def test_two_species_with_a_repeated_read(snp):
    """the two-species reference of test_gpu_front_half.py (segw: a workgroup reads its own species' words only), 200 copies of its
    first read as a batch among the others"""
    from oracle import oracle as orc
    from sketchy_amd import api
    refs, bases, off = [snp["ref2a"], snp["ref2b"]], snp["bases2"], snp["offsets2"]
    nb = 10
    n = (len(off) - 1) // nb
    c = 200
    r0 = np.ascontiguousarray(bases[int(off[0]):int(off[1])])
    rb, ro = np.tile(r0, c), np.arange(c + 1, dtype=np.uint64) * len(r0)
    R = api.ReferenceSketch(refs)
    S = api.SumOfSharedHashes(R, top=1, max_batch_reads=n, max_batch_bases=max(int(np.max(off[n:] - off[:-n])), len(rb)))
    d_b, d_rb = api.DeviceBuffer.from_numpy(bases), api.DeviceBuffer.from_numpy(rb)
    batches = [(d_b, off[i * n:(i + 1) * n + 1], bases) for i in range(nb)]
    batches.insert(nb - 3, (d_rb, ro, rb))   # (in the second pass)
    bufs = []
    try:
        assert R.n_species == 2 and R.static_dense[0]
        for d_x, o, _ in batches:
            m = len(o) - 1
            d_o = api.DeviceBuffer.from_numpy(np.ascontiguousarray(o))
            d_i, d_s = api.DeviceBuffer(m * 2 * 4), api.DeviceBuffer(m * 2 * 8)
            bufs.append((d_o, d_i, d_s))
            S.enqueue_device(d_x.ptr, d_o.ptr, m, int(o[-1] - o[0]), d_i.ptr, d_s.ptr)
        S.sync()
        cums = None
        for i, (_, o, x) in enumerate(batches):
            m = len(o) - 1
            e = orc.stream_fast_species(16, 0, S_, refs, x, o, top_k=1, cums=cums)
            cums = e["cums"]
            np.testing.assert_array_equal(bufs[i][2].to_numpy(np.uint64, (m, 2, 1)), e["topk_sum"], err_msg=f"sums of batch {i}")
            np.testing.assert_array_equal(bufs[i][1].to_numpy(np.uint32, (m, 2, 1)), e["topk_idx"], err_msg=f"genomes of batch {i}")
        np.testing.assert_array_equal(S.table(), np.concatenate(cums), err_msg="final tables")
        _reached_the_compact_path(S.stats())
    finally:
        d_b.free(); d_rb.free()
        for t in bufs:
            for x in t:
                x.free()
        S.close()
        R.close()


def test_the_int8_product_is_what_runs_and_the_old_kernel_agrees():
    """(the module docstring's last paragraph) children, so that the experiments build and its knob are what is loaded"""
    code = (
        "import sys, ctypes as C, hashlib, numpy as np; sys.path.insert(0, %r)\n"
        "import torch\n"
        "from sketchy_amd import api, synth, _lib\n"
        "ref = synth.make_reference(3000, 1000, rng_seed=5, device='cuda', mode='snp', n_lineages=15)\n"
        "src = torch.from_numpy(ref['truth_genome']).to('cuda')\n"
        "R = api.ReferenceSketch(ref['ref'])\n"
        "S = api.SumOfSharedHashes(R, top=1, max_batch_reads=16384, max_batch_bases=16384 * 1500)\n"
        "keep, outs = [], []\n"
        "def enqueue(p_b, p_o, n, n_bases):\n"
        "    d_i, d_s = api.DeviceBuffer(n * 4), api.DeviceBuffer(n * 8); outs.append((n, d_i, d_s))\n"
        "    S.enqueue_device(p_b, p_o, n, n_bases, d_i.ptr, d_s.ptr)\n"
        "def sample(i):\n"
        "    b, o = synth.make_reads_torch(src, 4096, 1500, rng_seed=50 + i, device='cuda'); keep.append((b, o))\n"
        "    enqueue(b.data_ptr(), o.data_ptr(), 4096, int(o[-1].item()))\n"
        "for i in range(9):\n"
        "    sample(i)\n"
        "b0, o0 = keep[0]\n"
        "r = b0[int(o0[0].item()):int(o0[1].item())].cpu().numpy()\n"
        "d_rb = api.DeviceBuffer.from_numpy(np.tile(r, 16384))\n"
        "d_ro = api.DeviceBuffer.from_numpy(np.arange(16385, dtype=np.uint64) * len(r))\n"
        "enqueue(d_rb.ptr, d_ro.ptr, 16384, 16384 * len(r))\n"
        "for i in range(9, 13):\n"
        "    sample(i)\n"
        "S.sync()\n"
        "h = hashlib.sha256()\n"
        "for n, d_i, d_s in outs:\n"
        "    h.update(d_i.to_numpy(np.uint32, (n,)).tobytes()); h.update(d_s.to_numpy(np.uint64, (n,)).tobytes())\n"
        "h.update(S.table().tobytes())\n"
        "L = _lib.load(); L.skx_debug_gain_launches.restype = None\n"
        "n = (C.c_ulonglong * 2)(); L.skx_debug_gain_launches(n, 0)\n"
        "st = S.stats()\n"
        "print('RESULT', h.hexdigest(), int(n[0]), int(n[1]), st['batches_compact'], st['passes_shared'], int(S.table().max()))\n"
    ) % ROOT
    outs = []
    for knob in (1, 0):
        p = subprocess.run([sys.executable, "-c", code], env=exp_env(SKX_GAIN_MFMA=knob), capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-2000:]
        outs.append([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT")][-1].split())
    print(outs)
    assert int(outs[0][2]) > 0 and int(outs[0][3]) == 0, outs[0]     # every launch as the int8 product ...
    assert int(outs[1][2]) == 0 and int(outs[1][3]) > 0, outs[1]     # ... and, with the knob, bit by bit
    assert int(outs[0][2]) == int(outs[1][3])                         # (the same launches)
    assert outs[0][1] == outs[1][1]                                   # same rows, same table
    assert int(outs[0][4]) >= 2 and int(outs[0][5]) >= 2              # shared deferred passes and compact rankings happened
    assert int(outs[0][6]) >= 16384                                   # (the copies' hashes are in the table: counts of 2^14 were summed)
