"""skx_sketch_groups (one pooled bottom-s sketch per group of records): what can be checked without a device -- the symbol is
exported and bound, and every argument check runs before the device is touched (include/sketchy_hip.h)."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

from sketchy_amd import _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _call(k=16, seed=0, s=8, bases="ok", offsets="ok", n_records=3, group_first="ok", n_groups=2, sketches="ok", sketch_len="ok",
          valid="ok"):
    """One call with valid defaults (3 records in 2 groups); a keyword replaces one argument (None = NULL)."""
    L = _lib.load()
    d = dict(bases=np.frombuffer(b"ACGTACGTACGTACGTACGTACGTACGTAC", np.uint8).copy(), offsets=np.array([0, 10, 20, 30], np.uint64),
             group_first=np.array([0, 2, 3], np.uint32), sketches=np.zeros((max(n_groups, 1), max(s, 1)), np.uint64),
             sketch_len=np.zeros(max(n_groups, 1), np.uint32), valid=np.zeros(max(n_groups, 1), np.uint64))
    given = dict(bases=bases, offsets=offsets, group_first=group_first, sketches=sketches, sketch_len=sketch_len, valid=valid)
    a = {name: (d[name] if isinstance(v, str) else v) for name, v in given.items()}
    rc = L.skx_sketch_groups(0, k, seed, s, _p(a["bases"]), _p(a["offsets"]), n_records, _p(a["group_first"]), n_groups,
                             _p(a["sketches"]), _p(a["sketch_len"]), _p(a["valid"]))
    return rc, L.skx_last_error().decode()


def test_symbol_is_exported_and_bound():
    L = _lib.load()
    assert "skx_sketch_groups" in {n for n, _, _ in _lib.SYMBOLS}
    assert hasattr(L, "skx_sketch_groups")
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    assert re.search(r"\bT skx_sketch_groups\b", out)
    from sketchy_amd import api
    assert callable(api.sketch_groups)


@pytest.mark.parametrize("kw, names", [
    (dict(offsets=None), "offsets"),
    (dict(group_first=None), "group_first"),
    (dict(sketches=None), "sketches"),
    (dict(sketch_len=None), "sketch_len"),
    (dict(bases=None), "bases"),
    (dict(k=0), "k"),
    (dict(k=_lib.MAX_K + 1), "k"),
    (dict(s=0), "s"),
    (dict(offsets=np.array([0, 20, 10, 30], np.uint64)), "offsets"),
    (dict(group_first=np.array([1, 2, 3], np.uint32)), "group_first"),      # does not start at 0
    (dict(group_first=np.array([0, 2, 2], np.uint32)), "group_first"),      # does not end at n_records
    (dict(group_first=np.array([0, 3, 2], np.uint32)), "group_first"),      # decreases
    (dict(group_first=np.array([0, 4, 3], np.uint32)), "group_first"),      # decreases, ends at n_records
])
def test_argument_errors_come_before_the_device(kw, names):
    rc, msg = _call(**kw)
    assert rc == _lib.ERR_INVALID, (rc, msg)
    assert re.search(r"\b%s\b" % names, msg), msg


def test_no_groups_is_ok():
    rc, msg = _call(n_records=0, n_groups=0, offsets=np.array([0], np.uint64), group_first=np.array([0], np.uint32), bases=None)
    assert rc == _lib.OK, msg
    rc, msg = _call(n_records=0, n_groups=0, offsets=np.array([7], np.uint64), group_first=np.array([0], np.uint32), valid=None)
    assert rc == _lib.OK, msg


def test_valid_arguments_without_a_device():
    if _lib.load().skx_device_count() > 0:
        pytest.skip("a device is present")
    for kw in (dict(), dict(valid=None), dict(group_first=np.array([0, 0, 3], np.uint32))):
        rc, msg = _call(**kw)
        assert rc == _lib.ERR_NO_DEVICE, (rc, msg)
        assert "no HIP device" in msg
    from sketchy_amd import api
    with pytest.raises(_lib.SketchyHipError) as e:
        api.sketch_groups(np.frombuffer(b"ACGTACGTAC", np.uint8), np.array([0, 10], np.uint64), np.array([0, 1], np.uint32), k=4, s=5)
    assert e.value.code == _lib.ERR_NO_DEVICE
