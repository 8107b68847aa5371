"""Child process of tests/test_gpu_composition.py: with whatever library and knobs the environment selects (the experiments build; knobs
are read once per process) runs the balanced three-species case of the composition tests -- synchronous pushes cut at [0, 250, 251, n]
with min_hits = 1, twelve enqueued batches with min_hits = 3 and one push of all reads on top, the query after every step -- against the oracle's expectation.
Prints a fixed last line on success; any difference ends it with a non-zero status."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import composition_cases as pc  # noqa: E402
import coverage_cases as cc  # noqa: E402
import hash_classes as hc  # noqa: E402

d, refs, col_lens, bases, offsets, hits = pc.balanced()
n = len(offsets) - 1
R, _, _ = cc.create_reference(d, hc.R_TEST, s=refs[0].shape[1])
print("index:", hc.index_figures(R))
cuts = (*pc.CUTS, n)
parts, table = pc.check_pushes(R, bases, offsets, hits, 1, cuts, what="worker pushes")
plain, plain_table = cc.plain_pushes(R, bases, offsets, cuts)
np.testing.assert_array_equal(table, plain_table)
for a, b in zip(parts, plain):
    np.testing.assert_array_equal(a["topk_idx"], b["topk_idx"])
    np.testing.assert_array_equal(a["topk_sum"], b["topk_sum"])
S = pc.stream(R, bases, 2 * n, top=1)
S.enable_composition(3)
edges = [int(x) for x in np.linspace(0, n, 13)]
cc.enqueue_batches(S, bases, offsets, edges, query_after=(4, 8, 12),
                   on_query=lambda b: pc.check(S, pc.composition(hits, 3, 0, b), what=f"worker enqueued, {b} reads"))
pc.check(S, pc.composition(hits, 3), what="worker enqueued, end")
np.testing.assert_array_equal(S.table(), plain_table)
st = S.stats()
print("enqueued:", st)
S.push(bases, offsets)   # (all reads once more, in one push)
once = pc.composition(hits, 3)
pc.check(S, (2 * once[0], 2 * once[1]), what="worker, every read twice")
if os.environ.get("SKX_PASS_READS"):
    assert S.stats()["last_passes"] > 1, S.stats()
S.close()
R.close()
print("composition ok")
