"""imsame_amd/bin/revComp, the drop-in for the reference's `revComp IN OUT`
(the second program of bin/all_vs_all_metagenomes_IMSAME.sh), and
imsame_amd.revcomp_file, the same path in-process.  One process at a time."""
import os
import subprocess
import time

import pytest

import imsame_amd
from imsame_amd import REVCOMP
from tests import golden_io as G

pytestmark = pytest.mark.gpu

USE = "ERR**** USE: reverseComplement seqFile.IN reverseComplementarySeq.OUT ****\n"
RCD = os.path.join(G.GOLDEN, "revcomp")
NAMES = sorted(f[:-3] for f in os.listdir(RCD) if f.endswith(".in"))


def run(*args, timeout=120):
    return subprocess.run([REVCOMP, *args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                          timeout=timeout)


@pytest.mark.parametrize("opts", [(), ("-window_bytes", "64")], ids=["default", "window64"])
def test_tool_matches_reference_goldens(tmp_path, opts):
    assert len(NAMES) >= 7
    for n in NAMES:
        out = tmp_path / (n + ".out")
        p = run(os.path.join(RCD, n + ".in"), str(out), *opts)
        assert (p.returncode, p.stdout) == (0, ""), (n, p.stdout, p.stderr)
        assert out.read_bytes() == open(os.path.join(RCD, n + ".out"), "rb").read(), n


def test_tool_without_records_writes_an_empty_file(tmp_path):
    src = tmp_path / "plain.txt"
    src.write_bytes(b"no record here\nACGT\n")
    out = tmp_path / "o.fa"
    out.write_bytes(b"stale")
    p = run(str(src), str(out), "-device", "0")
    assert (p.returncode, p.stdout) == (0, "")
    assert out.read_bytes() == b""


def test_tool_argument_and_open_errors(tmp_path):
    src = os.path.join(RCD, "basic.in")
    out = tmp_path / "o.fa"
    for args in ((src,), (src, str(out), str(out) + "2"), (), ("-window_bytes", "64", src, str(out)),
                 (src, str(out), "-window_bytes"), (src, str(out), "-no_such_option", "1")):
        p = run(*args)
        assert (p.returncode, p.stdout) == (255, USE), args
    assert not out.exists()
    p = run(str(tmp_path / "missing.fa"), str(out))
    assert (p.returncode, p.stdout) == (255, "ERR**** opening IN sequence FASTA file ****\n")
    assert not out.exists()
    p = run(src, str(tmp_path / "no_such_dir" / "o.fa"))
    assert (p.returncode, p.stdout) == (255, "ERR**** opening OUT sequence Words file ****\n")


def test_tool_on_an_input_past_4_gib(tmp_path):
    """A sparse file of 4 GiB + 64 MiB with one record at every 64 MiB
    boundary (the holes read as NUL bytes, which are no letters): u64 file
    offsets and the window arithmetic, at no cost in memory or disk."""
    step, n = 64 << 20, 66
    src = tmp_path / "sparse.fa"
    with open(src, "wb") as f:
        for k in range(n):
            f.seek(k * step)
            f.write(b">r%d\nACGT\n" % k)
    st = os.stat(src)
    assert st.st_size > (4 << 30) + step
    if st.st_blocks * 512 > (64 << 20):
        pytest.skip("the file system did not keep the file sparse")
    out = tmp_path / "sparse.r.fa"
    t = time.perf_counter()
    p = run(str(src), str(out), timeout=300)
    print(f"4 GiB + 64 MiB sparse input: {time.perf_counter() - t:.2f} s")
    assert (p.returncode, p.stdout) == (0, ""), (p.stdout, p.stderr)
    assert out.read_bytes() == b"".join(b">r%d\nACGT\n" % k for k in reversed(range(n)))


def test_revcomp_file_in_process(tmp_path):
    for n, w in (("synthetic", 4096), ("gt_in_header", 0)):
        out = tmp_path / (n + ".out")
        exp = open(os.path.join(RCD, n + ".out"), "rb").read()
        assert imsame_amd.revcomp_file(os.path.join(RCD, n + ".in"), str(out), window_bytes=w) == len(exp)
        assert out.read_bytes() == exp, n
