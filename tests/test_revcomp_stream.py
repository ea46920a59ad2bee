"""imsame_dev_revcomp_stream on the GPU: reverse complement in windows, u64
output offsets, per-thread work that does not grow with a line's length --
against the reference's goldens, the oracle and the one-shot call."""
import ctypes as C
import os
import time

import numpy as np
import pytest

import imsame_amd
from imsame_amd import Device, abi
from tests import golden_io as G

pytestmark = pytest.mark.gpu

ALPHABET = np.frombuffer(b"ACGTacgtNnUuRY*-\r\n>", dtype=np.uint8)
WINDOWS = [1, 16, 17, 257, 4096, 0]      # 1: every record doubles; 16 / 17: around the 16-byte loads; 0: default


@pytest.fixture(scope="module")
def dev():
    d = Device(0)
    yield d
    d.close()


@pytest.fixture(scope="module")
def cases(oracle):
    """(name, image, expected): the goldens with the reference's own output,
    20 random images with the oracle's (computed once)"""
    d = os.path.join(G.GOLDEN, "revcomp")
    out = []
    for n in sorted(f[:-3] for f in os.listdir(d) if f.endswith(".in")):
        data = open(os.path.join(d, n + ".in"), "rb").read()
        exp = open(os.path.join(d, n + ".out"), "rb").read()
        assert oracle.revcomp(data) == exp, n
        out.append((n, data, exp))
    assert len(out) >= 7
    rng = np.random.default_rng(21)
    for k in range(20):
        blob = ALPHABET[rng.integers(0, len(ALPHABET), int(rng.integers(0, 5001)))].tobytes()
        out.append((f"random{k}", blob, oracle.revcomp(blob)))
    return out


@pytest.mark.parametrize("window", WINDOWS)
def test_goldens_and_random_images(dev, cases, window):
    for name, data, exp in cases:
        assert dev.revcomp_stream(data, window) == exp, (name, window)
        if window == 0:
            assert dev.revcomp(data) == exp, name


EDGES = {
    "empty": b"",
    "no_gt": b"ACGT\nACGT\n",
    "pre_text": b"text before\nACGT\n>a\nAACC\n>b\nGG\n",
    "gt_last_byte": b">a\nAC\n>",
    "header_without_nl_at_eof": b">a\nAC\n>tail without newline",
    "nested": b">a>b>c\n",
    "nested_with_body": b">x\nTT\n>a>b>c\nACG\nT\n>y\nA\n",
    "crlf": b">a\r\nAC\r\nGT\r\n>b\r\nA\r\n",
    "long_then_short": b">long\n" + b"ACGTTGCA\n" * 700 + b">s1\nAC\n>s2\nG\n>s3\n\n",
}


@pytest.mark.parametrize("window", [1, 0])
@pytest.mark.parametrize("name", sorted(EDGES))
def test_edge_images(dev, oracle, name, window):
    img = EDGES[name]
    exp = oracle.revcomp(img)
    assert dev.revcomp_stream(img, window) == exp
    if name == "long_then_short":       # the record is longer than these windows too
        for w in (64, 1000):
            assert dev.revcomp_stream(img, w) == exp, w


def test_long_header_bounded_work(dev, oracle):
    """A 1 MiB header line with a '>' every 64 KiB: 16 records that repeat
    the rest of the line.  Header ends come from a scan and headers are copied
    per byte, so no thread walks the line."""
    img = (b">" + b"h" * (65536 - 1)) * 16 + b"\n" + b"ACGTACGTAC\n"
    exp = oracle.revcomp(img)
    assert len(exp) > 8_000_000
    assert dev.revcomp_stream(img) == exp
    assert dev.revcomp_stream(img, 4096) == exp


def test_past_the_reference_record_limit(dev, oracle):
    """1,000,001 records (the reference's offset array holds 1,000,000)"""
    img = b">\nA\n" * 1_000_001
    exp = oracle.revcomp(img)
    assert exp == b">\nT\n" * 1_000_001
    assert dev.revcomp_stream(img) == exp
    assert dev.revcomp_stream(img, 1 << 20) == exp      # four windows


# 93,000 '>' and one '\n': record k is the header's rest from its '>' on, so
# the output is, for m = 1 .. N, m x '>' then "\n\n": N(N+1)/2 + 2N bytes
NEST_N = 93_000
NEST_TOTAL = NEST_N * (NEST_N + 1) // 2 + 2 * NEST_N


def _nest_expected(a, b, n=NEST_N):
    """bytes [a, b) of that output (n: the number of '>')"""
    m = np.arange(1, n + 2, dtype=np.int64)
    start = (m - 1) * (m + 4) // 2                       # where piece m begins
    x = np.arange(a, b, dtype=np.int64)
    k = np.searchsorted(start, x, side="right") - 1
    return np.where(x - start[k] < m[k], 0x3E, 0x0A).astype(np.uint8)


def test_nest_expected_matches_oracle(oracle):
    """the analytic form above, on a small N against the oracle"""
    exp = oracle.revcomp(b">" * 300 + b"\n")
    assert len(exp) == 300 * 301 // 2 + 600
    assert _nest_expected(0, len(exp), 300).tobytes() == exp


def test_one_shot_reports_the_true_size(dev):
    """The one-shot call sees the u64 total: 4,324,732,500 bytes do not fit its
    buffer (nor its u32 contract), so it says so and writes nothing.  (A u32
    scan of the sizes wraps to 29,765,204.)"""
    assert NEST_TOTAL == 4_324_732_500
    img = np.frombuffer(b">" * NEST_N + b"\n", dtype=np.uint8)
    cap = 1 << 20
    out = np.full(cap, 0x55, dtype=np.uint8)
    ol = C.c_uint64()
    rc = imsame_amd.lib().imsame_dev_revcomp(dev._h, img.ctypes.data, len(img), out.ctypes.data, cap, C.byref(ol))
    assert rc == abi.IMSAME_E_ARG
    assert ol.value == NEST_TOTAL
    assert (out == 0x55).all()


def test_output_offsets_past_4_gib(dev):
    """The same image through the stream: 4.3 GB of output, checked around
    offsets 0, 2^32 and the end against the analytic form; the only test of
    output offsets past 2^32."""
    img = b">" * NEST_N + b"\n"
    span = 1 << 20
    regions = [(0, span), ((1 << 32) - span, (1 << 32) + span), (NEST_TOTAL - span, NEST_TOTAL)]
    expect = [_nest_expected(a, b) for a, b in regions]
    seen = [0] * len(regions)
    at = [0]

    def sink(piece):
        lo, hi = at[0], at[0] + len(piece)
        for r, (a, b) in enumerate(regions):
            x, y = max(a, lo), min(b, hi)
            if x < y:
                assert np.array_equal(piece[x - lo:y - lo], expect[r][x - a:y - a]), (r, x, y)
                seen[r] += y - x
        at[0] = hi

    t = time.perf_counter()
    total = dev.revcomp_stream(img, 0, sink=sink)
    print(f"4.3 GB stream: {time.perf_counter() - t:.2f} s")
    assert total == NEST_TOTAL and at[0] == NEST_TOTAL
    assert seen == [b - a for a, b in regions]


def test_callback_failure_is_an_io_error(dev):
    """a source or sink that fails ends the call with IMSAME_E_IO; the context
    runs the next call as if nothing had happened"""
    assert imsame_amd.lib().imsame_strerror(abi.IMSAME_E_IO) == b"input or output callback failed"
    img = np.frombuffer(b">a\nACGT\n" * 100, dtype=np.uint8)
    L = imsame_amd.lib()
    ok_src = abi.RC_SOURCE_FN(lambda u, o, n, d: C.memmove(d, img.ctypes.data + o, n) and 0)
    bad_src = abi.RC_SOURCE_FN(lambda u, o, n, d: 1)
    ok_sink = abi.RC_SINK_FN(lambda u, p, n: 0)
    bad_sink = abi.RC_SINK_FN(lambda u, p, n: 1)
    ol = C.c_uint64()
    for src, snk, want in ((bad_src, ok_sink, abi.IMSAME_E_IO), (ok_src, bad_sink, abi.IMSAME_E_IO),
                           (ok_src, ok_sink, 0)):
        for w in (64, 0):
            assert L.imsame_dev_revcomp_stream(dev._h, src, None, len(img), w, snk, None, C.byref(ol)) == want
    assert ol.value == len(img)
    assert dev.revcomp_stream(img.tobytes(), 64) == b">a\nACGT\n" * 100
