"""Change points of a stream, restated on the CPU: changes_ref (numpy; what tests/test_gpu_changes.py holds the device to) and
filter_changes (the text `predict -s --changes` must print, derived from what `predict -s` prints), with the host's own comparison
over full rows -- the path a library without skx_stream_bind_changes takes -- run against the stub-linked sanitizer build of
tests/test_host_cpu.py."""
import numpy as np
import pytest

from test_host_cpu import _fastq, _reference, _run, asan_bin  # noqa: F401  (asan_bin: that module's build of the stub-linked host)


def changes_ref(rows):
    """rows [n, ...] -> ascending indices r with r == 0 or rows[r] != rows[r - 1] in any element"""
    rows = np.asarray(rows)
    n = rows.shape[0]
    if n == 0:
        return np.zeros(0, np.int64)
    flat = rows.reshape(n, -1)
    flag = np.ones(n, bool)
    flag[1:] = (flat[1:] != flat[:-1]).any(axis=1)
    return np.flatnonzero(flag)


def filter_changes(text, top, header=""):
    """Of the text `predict -s` prints (blocks of `top` lines per read; one line with -c), the blocks `--changes` keeps: the first,
    and every block that differs from the block before it in anything but the read number and the shared_hashes column."""
    assert text.startswith(header)
    lines = text[len(header):].splitlines(keepends=True)
    assert len(lines) % top == 0
    out, prev, kept = [header], None, []
    for i in range(0, len(lines), top):
        block = lines[i:i + top]
        key = [ln.split("\t")[1:2] + ln.split("\t")[3:] for ln in block]
        if prev is None or key != prev:
            out += block
            kept.append(i // top)
        prev = key
    return "".join(out), kept


def test_changes_ref_small_cases():
    same = np.full((7, 3), 5, np.uint32)
    assert changes_ref(same).tolist() == [0]
    assert changes_ref(np.arange(12, dtype=np.uint32).reshape(6, 2)).tolist() == [0, 1, 2, 3, 4, 5]
    wide = np.zeros((5, 4096), np.uint32)
    wide[3:, -1] = 1  # one element differs, at the last position of a wide row
    assert changes_ref(wide).tolist() == [0, 3]
    wide[4, 0] = 9
    assert changes_ref(wide).tolist() == [0, 3, 4]
    assert changes_ref(np.zeros((0, 4), np.uint32)).tolist() == []
    assert changes_ref(np.zeros((1, 4), np.uint32)).tolist() == [0]
    cube = np.zeros((4, 3, 2), np.uint32)  # [reads, species, top]: any species' row counts
    cube[2:, 1, 1] = 7
    assert changes_ref(cube).tolist() == [0, 2]
    assert changes_ref(np.array([3, 3, 4, 4, 3], np.uint32)).tolist() == [0, 2, 4]


def test_filter_changes_ignores_read_number_and_sums():
    text = "1\ta\t10\tx\n2\ta\t11\tx\n3\tb\t11\tx\n4\tb\t11\ty\n5\tb\t12\ty\n"
    got, kept = filter_changes(text, 1)
    assert kept == [0, 2, 3] and got == "1\ta\t10\tx\n3\tb\t11\tx\n4\tb\t11\ty\n"
    two = "1\ta\t1\tx\n1\tb\t1\tx\n2\ta\t2\tx\n2\tb\t2\tx\n3\tb\t2\tx\n3\ta\t2\tx\n"
    assert filter_changes(two, 2)[1] == [0, 2]
    assert filter_changes("H\n" + text, 1, header="H\n")[0] == "H\n" + got


def _run_reads():
    """Reads whose stub rows -- genome (length + t) mod 23, sum = a hash of the bases -- repeat in runs: lengths 23 apart share a row
    but never a sum; runs of 1 to 40 reads, so that batches begin inside runs and at their starts."""
    rng = np.random.default_rng(4)
    alpha = np.frombuffer(b"ACGT", np.uint8)
    reads = []
    while len(reads) < 600:
        base = int(rng.integers(30, 53))
        for _ in range(int(rng.integers(1, 41))):
            reads.append(alpha[rng.integers(0, 4, base + 23 * int(rng.integers(0, 4)))].tobytes())
    return reads[:600]


@pytest.mark.parametrize("cons", (False, True), ids=("rows", "consensus"))
def test_cli_changes_is_the_filtered_stream_on_a_library_without_the_entry_point(asan_bin, tmp_path, cons):  # noqa: F811
    names, geno, msh, tsv = _reference(tmp_path)
    reads = _run_reads()
    fq = str(tmp_path / "runs.fq")
    _fastq(fq, reads)
    top = 3
    header = "reads\tsketch_id\tshared_hashes\tmlst\tmeca\n"
    base = ["predict", "-r", msh, "-g", tsv, "-i", fq, "-s", "-t", str(top), "-H", "-j", "5"] + (["-c"] if cons else [])
    rc, full, err = _run(*base, "-b", "16")
    assert rc == 0, err
    want, kept = filter_changes(full, 1 if cons else top, header)
    assert 5 < len(kept) < 300 and kept[0] == 0
    for extra in (("-b", "16", "--changes"), ("-b", "16", "-x"), ("-b", "100000", "-x"), ("-b", "7", "-x", "-j", "2")):
        rc, got, err = _run(*base, *extra)
        assert rc == 0, err
        assert got == want, extra
    # through stdin a batch is exactly -b = 4 reads (a mapped file is cut by bytes): batches that begin at a change point and batches that
    # begin inside a run, where the writer has to drop the batch's first block
    starts = set(range(0, 600, 4))
    assert starts & set(kept[1:]) and starts - set(kept), "batches must begin both at a change point and inside a run"
    piped = [a for a in base if a not in ("-i", fq)]
    rc, got, err = _run(*piped, "-b", "4", "-x", stdin=open(fq, "rb").read())
    assert rc == 0, err
    assert got == want
    rc, got, err = _run(*base, "-b", "16", "-x", "-l", "137")
    assert rc == 0 and got == filter_changes(_run(*base, "-b", "16", "-l", "137")[1], 1 if cons else top, header)[0]


def test_cli_changes_needs_a_stream(asan_bin, tmp_path):  # noqa: F811
    names, geno, msh, tsv = _reference(tmp_path)
    fq = str(tmp_path / "r.fq")
    _fastq(fq, _run_reads()[:5])
    for flag in ("--changes", "-x"):
        rc, out, err = _run("predict", "-r", msh, "-g", tsv, "-i", fq, flag)
        assert rc == 2 and out == "" and "--changes" in err and "-s" in err
