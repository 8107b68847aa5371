"""Child process of tests/test_gpu_sketch_counts.py: runs api.sketch_groups with and without counts on every case of an .npz file
with whatever library and knobs the environment selects (the experiments build with a forced row budget) and writes the results
next to it: sk / sl / vk / kc of the counted call, psk / psl / pvk of the plain one."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sketchy_amd import api  # noqa: E402

src, dst = sys.argv[1], sys.argv[2]
z = np.load(src)
out = {}
for i in range(int(z["n_cases"])):
    k, seed, s = (int(x) for x in z[f"params{i}"])
    args = (z[f"bases{i}"], z[f"offsets{i}"], z[f"first{i}"])
    out[f"psk{i}"], out[f"psl{i}"], out[f"pvk{i}"] = api.sketch_groups(*args, k=k, seed=seed, s=s, want_valid_kmers=True)
    out[f"sk{i}"], out[f"sl{i}"], out[f"vk{i}"], out[f"kc{i}"] = api.sketch_groups(*args, k=k, seed=seed, s=s, want_valid_kmers=True,
                                                                                   want_counts=True)
np.savez(dst, **out)
