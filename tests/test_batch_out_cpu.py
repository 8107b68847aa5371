"""The record of a batch's bound outputs (sketchy_amd/csrc/skx_batch_out.hpp) and the view of a holder's device arrays the kernels
get for it are plain host code: tests/stub/batch_out_check.cpp drives that header alone -- every combination of bound optional
columns for the change list, the species call's list, the call rows and the whole record -- built here with
-fsanitize=address,undefined and run once."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_batch_out_views_under_sanitizers(tmp_path):
    exe = str(tmp_path / "batch-out-check")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "sketchy_amd", "csrc"), os.path.join(ROOT, "tests", "stub", "batch_out_check.cpp"),
           "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=99", UBSAN_OPTIONS="halt_on_error=1:exitcode=98")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert re.search(r"\b0 failures\b", r.stdout), r.stdout
    assert int(r.stdout.split()[0]) > 5000
