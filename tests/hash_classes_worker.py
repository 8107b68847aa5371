"""Child process of tests/test_gpu_hash_classes.py: with whatever library and knobs the environment selects (the experiments build;
knobs are read once per process) runs the whole-sketch operators and the stream on the single-species designed reference
(tests/hash_classes.py: 64 dense hashes, rare_hash_genomes = 100) and compares everything with the oracle.  Prints a fixed last
line on success; any difference ends it with a non-zero status."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import hash_classes as hc  # noqa: E402

design = hc.single_species(64)
R, refs, col_lens = hc.create_reference(design, hc.R_TEST)
exp = hc.expected_index(design, hc.R_TEST)
got = hc.index_figures(R)
print("index figures:", got, "static rows of the design:", exp["static_dense"])
assert got["rare_index"] == exp["rare_index"], (got, exp)     # (bit rows, patterns and the static dictionary are what the knobs switch off)
names, q, qlen = hc.class_queries(design)
counts = hc.design_counts(design, q, qlen)
hc.check_operators(R, design.species, q, qlen, counts, (1, 5, 64), what="worker")
bases, offsets = hc.reads(design)
n = len(offsets) - 1
st = hc.check_pushes(R, hc.oracle_stream(refs, col_lens, bases, offsets, 1), bases, offsets, 1, [0, 500, 501, n], what="worker pushes")
print("pushes:", st)
st = hc.check_enqueued(R, hc.oracle_stream(refs, col_lens, bases, offsets, 3), bases, offsets, 3, list(range(0, n + 1, 100)), what="worker enqueued")
print("enqueued:", st)
if os.environ.get("SKX_PASS_READS"):
    assert st["passes"] > len(range(0, n, 100)), st
R.close()
print("hash classes ok")
