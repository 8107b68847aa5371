"""A list of genomes -> the aligned 64-genome groups (padded order) that the per-genome queries of a stream's statistics walk
(sketchy_amd/csrc/skx_genome_groups.hpp) is worked out on the host: tests/stub/genome_groups_check.cpp drives that code alone -- one and
several species, every genome, duplicates, species borders, out-of-range entries at every position -- against a brute-force real2pad,
built here with -fsanitize=address,undefined and run once."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_genome_groups_under_sanitizers(tmp_path):
    exe = str(tmp_path / "genome-groups-check")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "sketchy_amd", "csrc"), os.path.join(ROOT, "tests", "stub", "genome_groups_check.cpp"),
           "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=99", UBSAN_OPTIONS="halt_on_error=1:exitcode=98")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert re.search(r"\b0 failures\b", r.stdout), r.stdout
    assert int(r.stdout.split()[0]) > 500
