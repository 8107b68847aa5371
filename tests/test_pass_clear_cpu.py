"""The table of ranges a deferred pass clears in one launch (sketchy_amd/csrc/skx_pass_clear.hpp) is put together on the host:
tests/stub/pass_clear_check.cpp drives that code alone -- extreme batch counts, row strides and row extents; ranges inside their
arrays, disjoint, exactly as long as a slot's last use dirtied it; a full table refused -- built here with -fsanitize=address,undefined
and run once."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_clear_ranges_under_sanitizers(tmp_path):
    exe = str(tmp_path / "pass-clear-check")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "sketchy_amd", "csrc"), os.path.join(ROOT, "tests", "stub", "pass_clear_check.cpp"),
           "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=99", UBSAN_OPTIONS="halt_on_error=1:exitcode=98")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert re.search(r"\b0 failures\b", r.stdout), r.stdout
    assert int(r.stdout.split()[0]) > 500
