"""Edges of the packed NW kernel's first sweep (nw16_kernel.hip): its start
(lanes at rows <= 1), its end (lanes past a record's last rows, the last-row
best) and the stretch where a record is so short that both overlap; ties of
the best cell; predicted windows clipped at a record's first and last row.

Every case runs twice: on the CPU wave emulator (the kernel source) and,
marked `gpu`, on the device through Device.nw_pairs / Device.align.  Every
result field is compared with the oracle, every path with the 10-column
one-pass form's."""
import ctypes as C

import numpy as np
import pytest

import imsame_amd
from imsame_amd import PARITY_FIELDS
from tests import synth
from tests.emu_bind import Emu

FIELDS = ("score", "bx", "by", "length", "identities", "igaps", "egaps", "head_x", "head_y")
ACGT = synth.ACGT


class _EmuBackend:
    name = "emu"

    def __init__(self):
        self.emu = Emu.load()
        self.win = self.emu.lib.emu_win_count
        self.win.restype = C.c_uint32

    def nw_pairs(self, X, Y, p):
        p.want_paths = 1
        rc, res, paths, fl = self.emu.nw_pairs(X, Y, p, paths_cap=sum(len(x) + len(y) for x, y in zip(X, Y)) + 16)
        assert rc == 0 and fl == 0
        return res, paths

    def align(self, ref, rst, q, qs, p):
        """(results, halves that walked their first-sweep window, NW runs)"""
        self.win()
        rc, res, _, st = self.emu.align(ref, rst, q, qs, p, 4)
        assert rc == 0
        return res, self.win(), st.n_nw


class _GpuBackend:
    name = "gpu"

    def __init__(self):
        self.dev = imsame_amd.Device(0)

    def close(self):
        self.dev.close()

    def nw_pairs(self, X, Y, p):
        res, paths, _ = self.dev.nw_pairs(X, Y, p, want_paths=True)
        return res, paths

    def align(self, ref, rst, q, qs, p):
        self.dev.index(ref, rst)
        self.dev.set_query(q, qs)
        res, _, st = self.dev.align(n_threads=4, params=p)
        return res, st.nw_win, st.n_nw


@pytest.fixture(scope="module", params=["emu", pytest.param("gpu", marks=pytest.mark.gpu)])
def be(request):
    if request.param == "emu":
        yield _EmuBackend()
    else:
        b = _GpuBackend()
        yield b
        b.close()


def _params(oracle, flags=0):
    return oracle.params(min_coverage=1e-9, min_identity=1e-9, want_paths=1, flags=flags)


def _path(res, paths, k):
    r = res[k]
    return paths[r["path_off"]:r["path_off"] + r["path_len"]].tolist()


@pytest.fixture(scope="module")
def short_pairs():
    """150-base reads against records of 2 .. 151 bases in ONE launch: records
    shorter than the skewed start (G + 1 steps: 9 at 19 columns per lane, 16
    at 10), around one checkpoint interval (48) and, with 2 and 151 in one
    wave, a tail of xmax - xmin + G + 1 > 150 steps.  Each length twice: a
    record cut from its read (a real path) and a random one.  Two more whose
    only 4 on the last column is on row 0 (record AC / ACC, a read without C
    that ends in A): the column best takes rows 1 .. xlen-2 only, so a lane
    still at row 0 must not count."""
    rng = np.random.default_rng(4151)
    X, Y = [], []
    for xl in (2, 151, 3, 97, 9, 49, 10, 48, 17):
        for cut in (True, False):
            y = ACGT[rng.integers(0, 4, 150)]
            if cut and xl <= 150:
                o = int(rng.integers(0, 150 - xl + 1))
                x = y[o:o + xl].copy()
            elif cut:
                x = np.concatenate([ACGT[rng.integers(0, 4, xl - 150)], y])
            else:
                x = ACGT[rng.integers(0, 4, xl)]
            X.append(x.tobytes()); Y.append(y.tobytes())
    for x in (b"AC", b"ACC"):
        y = np.frombuffer(b"AGT", np.uint8)[rng.integers(0, 3, 150)]
        y[-1] = ord("A")
        X.append(x); Y.append(y.tobytes())
    return X, Y


@pytest.fixture(scope="module")
def short_expected(oracle, short_pairs):
    X, Y = short_pairs
    return [oracle.nw(x, y, text=False) for x, y in zip(X, Y)]


_ref_paths = {}


def _reference_paths(be, oracle, key, X, Y, monkeypatch):
    """paths of the 10-column one-pass form (per backend, computed once)"""
    if (be.name, key) not in _ref_paths:
        monkeypatch.setenv("IMSAME_NW_K", "10")
        res, paths = be.nw_pairs(X, Y, _params(oracle, imsame_amd.FLAG_NW16_ONEPASS))
        monkeypatch.delenv("IMSAME_NW_K")
        _ref_paths[be.name, key] = [_path(res, paths, k) if res[k]["status"] == 1 else None for k in range(len(X))]
    return _ref_paths[be.name, key]


def _check_pairs(be, oracle, key, X, Y, expected, monkeypatch, cols, band, onepass):
    ref = _reference_paths(be, oracle, key, X, Y, monkeypatch)
    monkeypatch.setenv("IMSAME_NW_BAND", band)
    if cols:
        monkeypatch.setenv("IMSAME_NW_K", cols)
    res, paths = be.nw_pairs(X, Y, _params(oracle, imsame_amd.FLAG_NW16_ONEPASS if onepass else 0))
    for k, o in enumerate(expected):
        for f in FIELDS:
            assert int(res[k][f]) == int(o[f]), (f, k, len(X[k]), cols, band, onepass)
        if ref[k] is not None:
            assert res[k]["status"] == 1 and _path(res, paths, k) == ref[k], (k, len(X[k]), cols, band, onepass)


@pytest.mark.parametrize("onepass", [False, True], ids=["two", "one"])
@pytest.mark.parametrize("band", ["200", "0"])
def test_short_records(be, oracle, short_pairs, short_expected, band, onepass, monkeypatch):
    """the 19-column form (every read has 150 bases): one and two passes, a
    band that holds every path and none (the redo from row 1)"""
    X, Y = short_pairs
    if be.name == "emu":
        k19 = be.emu.lib.emu_k19_count
        k19.restype = C.c_uint32
        k19()
    _check_pairs(be, oracle, "short", X, Y, short_expected, monkeypatch, None, band, onepass)
    if be.name == "emu":
        assert k19() > 0


@pytest.mark.parametrize("cols", ["10", "5", "3"])
def test_short_records_column_forms(be, oracle, short_pairs, short_expected, cols, monkeypatch):
    """the same launch in the 10-, 5- and 3-column forms: one step source"""
    X, Y = short_pairs
    _check_pairs(be, oracle, "short", X, Y, short_expected, monkeypatch, cols, "200", False)
    _check_pairs(be, oracle, "short", X, Y, short_expected, monkeypatch, cols, "0", True)


@pytest.fixture(scope="module")
def tie_pairs():
    """Homopolymer, dinucleotide and tandem repeats, 150-base reads against
    200 and 480 rows: the maximum recurs along the last column and the last
    row, in several checkpoint blocks (48 steps) -- `>=` must take the last
    row of the last column, the last row's best wins an equal score, and its
    last column wins among equals."""
    rng = np.random.default_rng(4152)
    rnd = lambda n: ACGT[rng.integers(0, 4, n)]                     # noqa: E731
    full = lambda n, b: np.full(n, ord(b), np.uint8)                # noqa: E731
    tile = lambda u, n: np.tile(np.frombuffer(u, np.uint8), n // len(u) + 2)[:n]   # noqa: E731
    X, Y = [], []
    for xl in (200, 480):
        unit = rnd(7).tobytes()
        y = rnd(150)
        twice = np.concatenate([rnd(20), y, rnd(xl - 20 - 2 * 150 - 5), y, rnd(5)]) if xl >= 330 else \
            np.concatenate([rnd(xl - 150), y])
        pairs = [
            (full(xl, "A"), full(150, "A")),                         # every cell a match
            (tile(b"AC", xl), tile(b"AC", 150)),                     # dinucleotide, in phase
            (tile(b"AC", xl), tile(b"CA", 150)),                     # ... out of phase
            (tile(unit, xl), tile(unit, 153)[3:]),                   # tandem repeat, shifted by 3
            (full(xl, "A"), np.concatenate([full(75, "A"), full(75, "C")])),   # best on the last column? no: last row
            (np.concatenate([full(xl - 60, "G"), full(60, "T")]), np.concatenate([full(90, "G"), full(60, "T")])),
            (tile(b"ACG", xl), tile(b"ACG", 150)),
            (twice, y),                                              # the read twice: equal maxima blocks apart
            (np.concatenate([y, rnd(xl - 150)]), y),                 # the read at the record's head
        ]
        for x, yy in pairs:
            assert len(x) == xl and len(yy) == 150
            X.append(x.tobytes()); Y.append(yy.tobytes())
    return X, Y


@pytest.fixture(scope="module")
def tie_expected(oracle, tie_pairs):
    X, Y = tie_pairs
    return [oracle.nw(x, y, text=False) for x, y in zip(X, Y)]


@pytest.mark.parametrize("cols,onepass", [(None, False), (None, True), ("10", False)], ids=["k19", "k19-one", "k10"])
def test_ties(be, oracle, tie_pairs, tie_expected, cols, onepass, monkeypatch):
    X, Y = tie_pairs
    last_row = [k for k, o in enumerate(tie_expected) if o["bx"] == len(X[k]) - 1]
    last_col = [k for k, o in enumerate(tie_expected) if o["bx"] < len(X[k]) - 1 and o["by"] == 149]
    assert len(last_row) >= 4 and len(last_col) >= 4, (last_row, last_col)
    _check_pairs(be, oracle, "ties", X, Y, tie_expected, monkeypatch, cols, "200", onepass)


@pytest.fixture(scope="module")
def edge_reads(oracle):
    """240 kbp in 700-base records; ~100 reads that start within 10 bases of a
    record's first base or end within 10 bases of its last one (2 %
    substitutions), so their predicted windows are clipped at row 1 and at
    the record's last row, and 10 % random reads."""
    ref, rst = synth.make_reference_arr(240_000, 700, seed=63)
    rng = np.random.default_rng(4153)
    reads = []
    for k in range(100):
        r = int(rng.integers(0, len(rst)))
        d = int(rng.integers(0, 10))
        o = int(rst[r]) + (d if k % 2 == 0 else 700 - 150 - d)
        y = ref[o:o + 150].copy()
        m = rng.random(150) < 0.02
        y[m] = ACGT[(np.searchsorted(ACGT, y[m]) + rng.integers(1, 4, int(m.sum()))) % 4]
        reads.append(y)
    reads += [ACGT[rng.integers(0, 4, 150)] for _ in range(11)]
    order = rng.permutation(len(reads))
    q = np.concatenate([reads[k] for k in order])
    qs = np.arange(0, len(q), 150, dtype=np.uint64)
    rc, exp, _ = oracle.align(ref, rst, q, qs, oracle.params(), 4)
    assert rc == 0
    return ref, rst, q, qs, exp


@pytest.mark.parametrize("window", ["1", "0", "bottom40"])
def test_window_edges(be, oracle, edge_reads, window, monkeypatch):
    """windows on, off, and on with the bottom window of unpredicted
    candidates (IMSAME_NW_WIN_BOTTOM, off by default)"""
    ref, rst, q, qs, exp = edge_reads
    if window == "bottom40":
        monkeypatch.setenv("IMSAME_NW_WIN_BOTTOM", "40")
        window = "1"
    monkeypatch.setenv("IMSAME_NW_WINDOW", window)
    got, n_win, n_nw = be.align(ref, rst, q, qs, oracle.params())
    for f in PARITY_FIELDS:
        assert np.array_equal(got[f], exp[f]), f
    acc = int((exp["status"] == 1).sum())
    assert acc >= 90, acc
    if window == "1":           # both kinds of half: walked in the window, and sent to the second sweep
        assert 0 < n_win < n_nw, (n_win, n_nw)
    else:
        assert n_win == 0
