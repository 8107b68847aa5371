"""Child process of tests/test_gpu_winners.py: with whatever library and knobs the environment selects (the experiments build; knobs are
read once per process) runs the 64-dense single-species case of the winners tests -- synchronous pushes cut at [0, 500, 501, n] and
twelve enqueued batches, the three queries after every step -- against the oracle's expectation.  Prints a fixed last line on success;
any difference ends it with a non-zero status."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import coverage_cases as cc  # noqa: E402
import hash_classes as hc  # noqa: E402
import winner_cases as wc  # noqa: E402
from sketchy_amd import api  # noqa: E402

d, refs, col_lens, bases, offsets = cc.single(64)
exp = wc.single_expected(64, None, (400, 500, 501, 800, 1200))
R, _, _ = cc.create_reference(d, hc.R_TEST, s=cc.S_SINGLE)
print("index:", hc.index_figures(R))
parts, table = wc.check_pushes(R, d.species, bases, offsets, cc.CUTS_1300, exp, cc.ROWS_1300, (1, 5, 64), what="worker pushes")
plain, plain_table = cc.plain_pushes(R, bases, offsets, cc.CUTS_1300)
np.testing.assert_array_equal(table, plain_table)
for a, b in zip(parts, plain):
    np.testing.assert_array_equal(a["topk_idx"], b["topk_idx"])
S = api.SumOfSharedHashes(R, top=1, max_batch_reads=2400, max_batch_bases=len(bases))
S.enable_coverage()
cc.enqueue_batches(S, bases, offsets, list(range(0, 1201, 100)), query_after=(4, 8, 12),
                   on_query=lambda b: wc.check_queries(S, exp[b], d.species, cc.ROWS_1300, (5,), what=f"worker enqueued, {b} reads"))
wc.check_queries(S, exp[1200], d.species, cc.ROWS_1300, (1, 5, 64), what="worker enqueued, end")
np.testing.assert_array_equal(S.table(), plain_table)
st = S.stats()
print("enqueued:", st)
if os.environ.get("SKX_PASS_READS"):
    assert st["passes"] > 12, st
S.close()
R.close()
print("winners ok")
