"""Child process of tests/test_gpu_call_rows.py: with whatever library and knobs the environment selects (the experiments build).
  chunks IN.npz OUT.npz   api.call_rows on IN's idx, sums and codes (SKX_CALL_ROWS cuts the rows into chunks)"""
import sys

import numpy as np

sys.path.insert(0, __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__))))
from sketchy_amd import api  # noqa: E402


def chunks(z):
    return api.call_rows(z["idx"], z["sums"], z["codes"])


if __name__ == "__main__":
    mode, src, dst = sys.argv[1:4]
    np.savez(dst, **{"chunks": chunks}[mode](np.load(src)))
