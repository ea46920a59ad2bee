"""The packed NW kernel's first-sweep stop (nw16_kernel.hip): the
sweep ends once no lower row can hold the best cell.

CPU: the theorem behind it on a plain numpy statement of the recurrence
 -- `clear`, Bmin and the row formula, restated
here in Python -- and the kernel source on the wave emulator with the stop on
and off.  GPU (marked `gpu`): the same sets through Device.nw_pairs and
Device.align against the oracle, on and off."""
import ctypes as C
import functools
import re

import numpy as np
import pytest

import imsame_amd
from imsame_amd import PARITY_FIELDS
from tests import golden_io, synth
from tests.emu_bind import Emu

FIELDS = ("score", "bx", "by", "length", "identities", "igaps", "egaps", "head_x", "head_y")
ACGT = synth.ACGT
MER = 12        # the probed word
STRIDE = 4      # every fourth record row is probed (rows = 0 mod 4) ...
RUN = MER + STRIDE - 1      # ... so a run of 15 matches always holds a probed row with its whole 12-mer
GAPS = ((-5, -2), (-8, -1), (-1, -4))
NEG = -(1 << 28)


# ----------------------------------------------------------------- the theorem's terms, restated

@functools.lru_cache(maxsize=None)
def bmin(ylen, ig, eg):
    """1 + the best score of a chain without a diagonal run of RUN matches:
    max 4m - 4x - (|ig| + |eg|) g over m <= (RUN - 1) (x + g + 1), m + x <= ylen"""
    c = -(ig + eg)
    return 1 + max(4 * min(ylen - x, (RUN - 1) * (x + g + 1)) - 4 * x - c * g
                   for x in range(ylen + 1) for g in range(ylen // (RUN - 1) + 2))


def clear_row(x, y):
    """1 + the last probed row of x (every STRIDE-th) where a 12-mer of y
    starts; 0: none.  Below it no diagonal run of RUN matches starts: such a
    run holds a probed row within its first STRIDE rows, whose 12-mer lies
    inside the run."""
    mers = {y[j:j + MER].tobytes() for j in range(len(y) - MER + 1)}
    for i in range(len(x) - MER, -1, -1):
        if i % STRIDE == 0 and x[i:i + MER].tobytes() in mers:
            return i + 1
    return 0


def first_safe_row(clear, ylen, B, eg):
    """the first row i with i > clear - 2 + ylen + (4 ylen - B) / |eg|"""
    return clear - 2 + ylen + (4 * ylen - B) // (-eg) + 1


def dp_tables(Xs, Ys, ig, eg):
    """T of Q8 for every pair, [n, xmax, ymax] (a pair's own table is its top
    left corner: no value depends on a later row or column), swept along
    anti-diagonals: mf is a row's state, mc a column's"""
    n, XM, YM = len(Xs), max(map(len, Xs)), max(map(len, Ys))
    Xc = np.full((n, XM), 1, np.uint8)
    Yc = np.full((n, YM), 2, np.uint8)
    for k in range(n):
        Xc[k, :len(Xs[k])] = Xs[k]
        Yc[k, :len(Ys[k])] = Ys[k]
    S = np.where(Xc[:, :, None] == Yc[:, None, :], 4, -4).astype(np.int32)
    T = np.full((n, XM, YM), NEG, np.int32)
    T[:, 0, :] = S[:, 0, :]
    T[:, :, 0] = S[:, :, 0]
    MFs, MFy = T[:, :, 0].copy(), np.zeros((n, XM), np.int32)       # mf = (T[i][0], i, 0)
    MCs, MCx = T[:, 0, :].copy(), np.zeros((n, YM), np.int32)       # mc[j] = (T[0][j], 0, j)
    ar = np.arange(n)[:, None]
    for t in range(2, XM + YM - 1):
        J = np.arange(max(1, t - (XM - 1)), min(YM - 1, t - 1) + 1)
        I = t - J
        j2, i1 = (J > 1)[None, :], (I > 1)[None, :]
        Jm2, Im2 = np.maximum(J - 2, 0), np.maximum(I - 2, 0)
        # 1. mf.score <= T[i][j-2] -> mf = (T[i-1][j-2], i-1, j-2)
        mfs, mfy = MFs[ar, I], MFy[ar, I]
        rep = j2 & (mfs <= T[ar, I, Jm2])
        mfs = np.where(rep, T[ar, I - 1, Jm2], mfs)
        mfy = np.where(rep, J - 2, mfy)
        MFs[ar, I], MFy[ar, I] = mfs, mfy
        # 2.-5. the value (the choice among equals does not change it)
        diag = T[ar, I - 1, J - 1]
        left = np.where(j2, mfs + ig + (J - mfy - 1) * eg, NEG)
        mcs, mcx = MCs[ar, J - 1], MCx[ar, J - 1]
        up = np.where(i1, mcs + ig + (I - mcx - 1) * eg, NEG)
        T[ar, I, J] = np.maximum(diag, np.maximum(left, up)) + S[ar, I, J]
        # 6. T[i-2][j-1] > mc[j-1].score -> mc[j-1] = (T[i-2][j-1], i-2, j-1)
        t2 = T[ar, Im2, J - 1]
        upd = i1 & j2 & (t2 > mcs)
        MCs[ar, J - 1] = np.where(upd, t2, mcs)
        MCx[ar, J - 1] = np.where(upd, I - 2, mcx)
    return T


def best_cell(T):
    """Q9: row-major over the last column and the last row (i, j >= 1), `>=`"""
    xl, yl = T.shape
    best = (NEG, 0, 0)
    for i in range(1, xl):
        for j in (range(1, yl) if i == xl - 1 else (yl - 1,)):
            if T[i, j] >= best[0]:
                best = (int(T[i, j]), i, j)
    return best


# ----------------------------------------------------------------- the pairs

def _rnd(rng, n):
    return ACGT[rng.integers(0, 4, max(int(n), 0))]


def _other(rng, b):
    """a base that differs from b"""
    return ACGT[(int(np.searchsorted(ACGT, b)) + int(rng.integers(1, 4))) % 4]


def _subs_at(rng, y, pos):
    y = y.copy()
    for p in pos:
        y[p] = _other(rng, y[p])
    return y


def _spread(n, k):
    """k positions that cut n bases into runs of about n / (k + 1)"""
    return [int((q + 1) * n / (k + 1)) for q in range(k)]


def adversarial_pairs(rng, ylen, xlen, eg):
    """(x, y) pairs built against the stop's argument, for one read length,
    records of xlen rows at most (each pair may be shorter) and |eg|:
    the read planted with a few substitutions, and below it, at distances
    around the formula's row, a second copy -- exact, or with 1-12
    substitutions (12 spread ones leave no 12-mer) -- or only shared words of
    11, 12, 14 and 15 bases (around the probed word and the run a probe cannot
    miss), at every row phase; the read's suffix on the record's last rows; repeats; a read with
    12+ errors (B < Bmin)."""
    out = []
    room = xlen - 2 * ylen
    assert room >= 40

    def planted(y, nsub):
        return _subs_at(rng, y, rng.choice(ylen, nsub, replace=False)) if nsub else y

    # a second copy below the first, its distance around the row formula
    # (first copy's clear - 2 + ylen + (4 ylen - B) / |eg| - its own rows)
    for nsub2 in (0, 1, 3, 6, 12):
        for nsub1 in (0, 2):
            a = int(rng.integers(0, 20))
            slack = (8 * nsub1) // (-eg)
            for d in sorted({0, 1, max(0, slack - 1), slack + 1, slack + 13, min(room - a - 2, slack + ylen)}):
                y = _rnd(rng, ylen)                               # (a read of its own per pair)
                second = _subs_at(rng, y, _spread(ylen, nsub2)) if nsub2 else y
                x = np.concatenate([_rnd(rng, a), planted(y, nsub1), _rnd(rng, d), second,
                                    _rnd(rng, rng.integers(0, room - a - d))])
                out.append((x, y))
    # the read's suffix alone, ending on the record's last row
    for cut in (1, ylen // 3, ylen - MER, ylen - MER + 1):
        a, y = int(rng.integers(0, 20)), _rnd(rng, ylen)
        x = np.concatenate([_rnd(rng, a), planted(y, 1), _rnd(rng, rng.integers(0, room - a)), y[cut:]])
        out.append((x, y))
    # exactly an 11-mer / a 12-mer of the read in the lower part (both neighbours differ)
    for k in (MER - 1, MER, RUN - 1, RUN):
        for ph in range(4):
            a, p, y = int(rng.integers(0, 20)), int(rng.integers(1, ylen - k - 1)), _rnd(rng, ylen)
            w = np.concatenate([[_other(rng, y[p - 1])], y[p:p + k], [_other(rng, y[p + k])]]).astype(np.uint8)
            x = np.concatenate([_rnd(rng, a), planted(y, int(rng.integers(0, 3))), _rnd(rng, rng.integers(1, max(2, room // 8)) * 4 + ph), w,
                                _rnd(rng, rng.integers(0, max(1, room // 4)))])
            out.append((x, y))
    # tandem repeats and homopolymers
    for unit in (b"A", b"AC", _rnd(rng, 7).tobytes(), _rnd(rng, 13).tobytes()):
        u = np.frombuffer(unit, np.uint8)
        yy = np.tile(u, ylen // len(u) + 2)[:ylen]
        out.append((np.tile(u, xlen // len(u) + 2)[:xlen], yy))
        out.append((np.concatenate([_rnd(rng, 30), yy, _rnd(rng, min(room, 200))]), yy))
    # 12+ errors: no run of 12 left, so B < Bmin and no stop
    y = _rnd(rng, ylen)
    x = np.concatenate([_rnd(rng, 10), _subs_at(rng, y, _spread(ylen, max(12, ylen // MER + 1))), _rnd(rng, min(room, 150))])
    out.append((x, y))
    # 9 clustered errors: long runs and a seed, but B = 4 ylen - 72 < Bmin at 150 bases
    y = _rnd(rng, ylen)
    x = np.concatenate([_rnd(rng, 10), _subs_at(rng, y, [ylen // 2 + 2 * q for q in range(min(9, ylen // 4))]), _rnd(rng, min(room, 150))])
    out.append((x, y))
    for x, yy in out:
        assert 2 <= len(x) <= xlen and len(yy) == ylen, (len(x), len(yy))
    return out


def theorem_sets():
    """per gap pair: a few hundred pairs in all, reads of 30-160 bases,
    records of 200-1,200 rows, random or adversarial"""
    rng = np.random.default_rng(16012)
    sets = []
    for gi, (ig, eg) in enumerate(GAPS):
        pairs = []
        for yi, (ylen, xlen) in enumerate(((30, 200), (64, 420), (100, 300), (150, 520), (160, 1200 if gi == 0 else 600))):
            # (every second kind at 150 bases, every fourth elsewhere, a different quarter at each length)
            pairs += adversarial_pairs(rng, ylen, xlen, eg)[(yi + gi) % 2::2] if ylen == 150 else \
                adversarial_pairs(rng, ylen, xlen, eg)[(yi + gi) % 4::4]
            for _ in range(6):                                    # random pairs, and planted reads with errors
                y = _rnd(rng, ylen)
                pairs.append((_rnd(rng, rng.integers(200, xlen + 1)), y))
                yy = _subs_at(rng, y, rng.choice(ylen, int(rng.integers(0, 5)), replace=False))
                a = int(rng.integers(0, xlen - ylen))
                pairs.append((np.concatenate([_rnd(rng, a), yy, _rnd(rng, xlen - ylen - a)]), y))
        sets.append((ig, eg, pairs))
    return sets


@pytest.fixture(scope="module")
def theorem_tables():
    """(ig, eg, x, y, T) of every pair; tables computed once, in batches of one shape class"""
    out = []
    for ig, eg, pairs in theorem_sets():
        order = sorted(range(len(pairs)), key=lambda k: (len(pairs[k][1]), len(pairs[k][0])))
        for b in range(0, len(order), 48):
            idx = order[b:b + 48]
            T = dp_tables([pairs[k][0] for k in idx], [pairs[k][1] for k in idx], ig, eg)
            for q, k in enumerate(idx):
                x, y = pairs[k]
                out.append((ig, eg, x, y, T[q, :len(x), :len(y)].copy()))
    return out


def test_numpy_statement_matches_oracle(oracle, theorem_tables):
    """the numpy recurrence is the oracle's: best cell and score of every pair"""
    assert 200 <= len(theorem_tables) <= 900
    for ig, eg, x, y, T in theorem_tables[::3]:
        o = oracle.nw(x.tobytes(), y.tobytes(), igap=ig, egap=eg, text=False)
        assert best_cell(T) == (o["score"], o["bx"], o["by"]), (ig, eg, len(x), len(y))


def test_bmin(oracle):
    """tight enough to matter, the kernel header's equals this file's, and off where the argument fails"""
    assert bmin(150, -5, -2) <= 4 * 150 - 60
    assert bmin(150, -5, -2) == 4 * 150 - 7 * 10 + 1                    # 150 matches in eleven runs: x = 0, g = 10
    f = Emu.load().lib.emu_nw16_bmin
    f.restype, f.argtypes = C.c_int32, [C.c_int64, C.c_int64, C.c_int64]
    for ig, eg in GAPS + ((0, -1), (-30, -7)):
        for ylen in (12, 13, 30, 64, 149, 150, 160, 320):
            assert f(ylen, ig, eg) == bmin(ylen, ig, eg), (ylen, ig, eg)
    for ylen, ig, eg in ((150, -5, 0), (150, 1, -2), (150, -5, 2), (11, -5, -2), (321, -5, -2)):
        assert f(ylen, ig, eg) == 2 ** 31 - 1


def test_theorem(theorem_tables):
    """For every pair and every row r, with B the last column's best over rows
    1 .. r: if B >= Bmin, no cell on or below the formula's first safe row
    reaches B.  (B changes only where the running best does, so each of its
    values is checked once, at the first row that holds it.)"""
    checked = stops = 0
    for ig, eg, x, y, T in theorem_tables:
        xl, yl = T.shape
        clear, bm = clear_row(x, y), bmin(yl, ig, eg)
        below = np.maximum.accumulate(T.max(axis=1)[::-1])[::-1]       # best of any cell on rows >= i
        run = np.maximum.accumulate(T[1:, yl - 1])
        for B in np.unique(run):
            B = int(B)
            if B < bm:
                continue
            checked += 1
            i0 = max(first_safe_row(clear, yl, B, eg), 0)
            if i0 < xl:
                stops += 1
                assert below[i0] < B, (ig, eg, xl, yl, clear, B, i0, int(below[i0]))
    assert checked >= 150 and stops >= 60, (checked, stops)             # the sets do reach the stop


# ----------------------------------------------------------------- the kernel: emulator and device

class _EmuBackend:
    name = "emu"

    def __init__(self):
        self.emu = Emu.load()
        self._cnt = self.emu.lib.emu_nw16_stop_counts
        self._cnt.argtypes = [C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]

    def counts(self):
        a, b = C.c_uint64(), C.c_uint64()
        self._cnt(C.byref(a), C.byref(b))
        return a.value, b.value

    def nw_pairs(self, X, Y, p):
        p.want_paths = 1
        rc, res, paths, fl = self.emu.nw_pairs(X, Y, p, paths_cap=sum(len(x) + len(y) for x, y in zip(X, Y)) + 16)
        assert rc == 0 and fl == 0
        return res, paths

    def align(self, ref, rst, q, qs, p, capfd=None):
        """(results, paths, (waves that stopped, steps they skipped))"""
        self.counts()
        p.want_paths = 1
        rc, res, paths, _ = self.emu.align(ref, rst, q, qs, p, 4, paths_cap=len(ref) + len(q) + 1024)
        assert rc == 0
        return res, paths, self.counts()


class _GpuBackend:
    name = "gpu"

    def __init__(self):
        self.dev = imsame_amd.Device(0)

    def close(self):
        self.dev.close()

    def nw_pairs(self, X, Y, p):
        res, paths, _ = self.dev.nw_pairs(X, Y, p, want_paths=True)
        return res, paths

    def align(self, ref, rst, q, qs, p, capfd=None):
        """the counters come from the [nwprof] line (the test sets IMSAME_NW_PROF)"""
        self.dev.index(ref, rst)
        self.dev.set_query(q, qs)
        capfd.readouterr()
        res, paths, _ = self.dev.align(n_threads=4, params=p, want_paths=True, paths_cap=len(ref) + len(q) + 1024)
        m = re.search(r"stop\(waves steps_skipped\) (\d+) (\d+)", capfd.readouterr().err)
        assert m, "no [nwprof] line"
        return res, paths, (int(m.group(1)), int(m.group(2)))


@pytest.fixture(scope="module", params=["emu", pytest.param("gpu", marks=pytest.mark.gpu)])
def be(request):
    if request.param == "emu":
        yield _EmuBackend()
    else:
        b = _GpuBackend()
        yield b
        b.close()


def _path(res, paths, k):
    r = res[k]
    return paths[r["path_off"]:r["path_off"] + r["path_len"]].tolist()


def _paths(res, paths):
    """every accepted read's path"""
    return [_path(res, paths, k) if res[k]["status"] == 1 else None for k in range(len(res))]


def _set_form(monkeypatch, cols, stop):
    monkeypatch.setenv("IMSAME_NW_STOP", stop)
    monkeypatch.setenv("IMSAME_NW_PROF", "1")
    if cols != "19":
        monkeypatch.setenv("IMSAME_NW_K", cols)


def _db(pairs):
    """records and reads of the pairs as one database and one query"""
    ref = np.concatenate([x for x, _ in pairs])
    rst = np.cumsum([0] + [len(x) for x, _ in pairs[:-1]]).astype(np.uint64)
    q = np.concatenate([y for _, y in pairs])
    qs = np.cumsum([0] + [len(y) for _, y in pairs[:-1]]).astype(np.uint64)
    return ref, rst, q, qs


def _on_and_off(be, oracle, db, exp, cols, monkeypatch, capfd):
    """the pipeline (it carries the predicted rows the stop needs) with the stop
    on and off: every parity field is the oracle's both times, every path the
    same; returns the counters of the run with the stop on"""
    runs, cnts = {}, {}
    for stop in ("1", "0"):
        _set_form(monkeypatch, cols, stop)
        got, paths, cnts[stop] = be.align(*db, oracle.params(), capfd)
        for f in PARITY_FIELDS:
            assert np.array_equal(got[f], exp[f]), (f, cols, stop)
        runs[stop] = _paths(got, paths)
    assert runs["1"] == runs["0"], cols
    assert any(r for r in runs["1"])
    assert cnts["0"] == (0, 0), (cols, cnts)
    return cnts["1"]


@pytest.fixture(scope="module")
def planted(oracle):
    """96 reads of 150 bases, each in a 2,000-row record of its own at a
    random row, 0-4 substitutions: every wave can stop"""
    rng = np.random.default_rng(16013)
    pairs = []
    for _ in range(96):
        y = _rnd(rng, 150)
        a = int(rng.integers(0, 1850))
        yy = _subs_at(rng, y, rng.choice(150, int(rng.integers(0, 5)), replace=False))
        pairs.append((np.concatenate([_rnd(rng, a), yy, _rnd(rng, 1850 - a)]), y))
    db = _db(pairs)
    rc, exp, _ = oracle.align(*db, oracle.params(), 4)
    assert rc == 0 and int((exp["status"] == 1).sum()) == 96
    return db, exp


@pytest.fixture(scope="module")
def adversarial(oracle):
    """the theorem's adversarial pairs at 150 bases in records of up to 2,000
    rows (one has all 2,000, so the launch's LDS share holds the table), each
    pair a record and a read of one database: ~90 candidates and more"""
    rng = np.random.default_rng(16014)
    pairs = adversarial_pairs(rng, 150, 2000, -2)
    y = _rnd(rng, 150)
    pairs.append((np.concatenate([_rnd(rng, 400), y, _rnd(rng, 1450)]), y))
    assert 64 <= len(pairs) <= 512 and max(len(x) for x, _ in pairs) == 2000
    db = _db(pairs)
    rc, exp, _ = oracle.align(*db, oracle.params(), 4)
    assert rc == 0 and int((exp["status"] == 1).sum()) >= 48
    return pairs, db, exp


COLS = ["19", "10", "5", "3"]
# (lanes per candidate pair, candidates per wave, checkpoint interval) of the forms at 150 bases
FORM = {"19": (8, 16, 48), "10": (15, 8, 48), "5": (30, 4, 32), "3": (50, 2, 14)}


@pytest.mark.parametrize("cols", COLS)
def test_planted_stops(be, oracle, planted, cols, monkeypatch, capfd):
    """the stop fires on planted reads and changes no result and no path; off, the counters stay 0"""
    db, exp = planted
    cnt = _on_and_off(be, oracle, db, exp, cols, monkeypatch, capfd)
    assert cnt[0] > 0 and cnt[1] >= 2 * cnt[0], (cols, cnt)               # a stop leaves out a pair of steps at least


@pytest.mark.parametrize("cols", COLS)
def test_adversarial_pipeline(be, oracle, adversarial, cols, monkeypatch, capfd):
    """second copies, shared 11-, 12-, 14- and 15-mers, suffixes, repeats and
    bad reads through the pipeline, against the oracle, on and off, paths included"""
    _, db, exp = adversarial
    _on_and_off(be, oracle, db, exp, cols, monkeypatch, capfd)


@pytest.mark.parametrize("cols", COLS)
def test_adversarial_pipeline_one_pass(be, oracle, adversarial, cols, monkeypatch, capfd):
    """one pass: no predicted rows reach the kernel, so no stop"""
    _, db, exp = adversarial
    monkeypatch.setenv("IMSAME_NW_ONEPASS", "1")
    assert _on_and_off(be, oracle, db, exp, cols, monkeypatch, capfd) == (0, 0)


# ---- the step a wave stops at, term by term

XLEN, YLEN, NREADS = 2000, 150, 64


def stop_step(cols, a, clear, B, ig=-5, eg=-2, drop_score=False, drop_ylen=False):
    """The step before which a wave whose candidates all sit at row `a` of
    XLEN-row records, with last-column best B and `clear`, ends its first
    sweep: the first checkpoint step t = 1 + m CK (m >= 1, a pair of steps
    still to run) past the window's end with B >= Bmin and t - (G - 1) past
    the formula's row; None: never.  drop_*: the same with one term of the
    formula left out (what a wrong kernel would do)."""
    G, _, CK = FORM[cols]
    tend = XLEN - 1 + G
    hi = min(a + YLEN - 1 + 24, XLEN) + G                  # the window's end (NW16_WIN_DOWN), made odd
    tw1 = hi + ((hi & 1) ^ 1)
    if B < bmin(YLEN, ig, eg):
        return None
    base = clear - 2 + (0 if drop_ylen else YLEN)
    for t in range(1 + CK, tend - 1, CK):
        if t >= tw1 and (-eg) * (t - (G - 1) - base) > (0 if drop_score else 4 * YLEN - B):
            return t
    return None


def uniform_set(oracle, a, nsub, seed):
    """NREADS reads, each at row `a` of its own XLEN-row record with the same
    nsub substitutions (bases 60, 62, ...: a seed before and after them), so
    every candidate has one B = 600 - 8 nsub, one `clear` and one predicted
    row, and every wave stops at one step whatever its candidates"""
    rng = np.random.default_rng(seed)
    pairs = []
    clear = a + max(j for j in range(YLEN - MER + 1) if (a + j) % STRIDE == 0) + 1    # the last probed 12-mer of the copy
    while len(pairs) < NREADS:
        y = _rnd(rng, YLEN)
        yy = _subs_at(rng, y, [60 + 2 * q for q in range(nsub)])
        x = np.concatenate([_rnd(rng, a), yy, _rnd(rng, XLEN - YLEN - a)])
        o = oracle.nw(x.tobytes(), y.tobytes(), text=False)
        # (no chance 12-mer in the random rows below, and no gapped path that beats the plain diagonal)
        if clear_row(x, y) == clear and (o["score"], o["bx"]) == (4 * YLEN - 8 * nsub, a + YLEN - 1):
            pairs.append((x, y))
    return pairs, clear


def pick_row(cols, nsub):
    """a row `a` at which each term of the stop test decides the step: without
    the score term, or without ylen in the row, the wave would stop at another
    checkpoint (found by the model above, not by running the kernel)"""
    B = 4 * YLEN - 8 * nsub
    if B < bmin(YLEN, -5, -2):
        return 200                                                # no stop at any row
    for a in range(200, 400):
        j = max(j for j in range(YLEN - MER + 1) if (a + j) % STRIDE == 0)     # the last intact, probed 12-mer
        clear = a + j + 1
        t = stop_step(cols, a, clear, B)
        if t is not None and t != stop_step(cols, a, clear, B, drop_ylen=True) and \
                (nsub == 0 or t != stop_step(cols, a, clear, B, drop_score=True)):
            return a
    raise AssertionError("no such row")


_uniform = {}


def _uniform_case(oracle, cols, nsub):
    if (cols, nsub) not in _uniform:
        a = pick_row(cols, nsub)
        pairs, clear = uniform_set(oracle, a, nsub, 16100 + nsub)
        db = _db(pairs)
        rc, exp, _ = oracle.align(*db, oracle.params(), 4)
        assert rc == 0 and (exp["status"] == 1).all()
        assert (exp["score"] == 4 * YLEN - 8 * nsub).all() and (exp["bx"] == a + YLEN - 1).all()
        _uniform[cols, nsub] = (a, clear, db, exp)
    return _uniform[cols, nsub]


@pytest.mark.parametrize("nsub", [0, 8, 9])
@pytest.mark.parametrize("cols", COLS)
def test_stop_step(be, oracle, cols, nsub, monkeypatch, capfd):
    """Every wave of a uniform set stops at the step the formula gives, and so
    the counters are known: exact reads (B = 600), 8 substitutions (B = 536 >=
    Bmin = 531: the score term moves the stop by a checkpoint) and 9 (B = 528
    < Bmin: no wave may stop).  The emulator runs the form asked for; on the
    device the launch may take any of the four forms."""
    a, clear, db, exp = _uniform_case(oracle, cols, nsub)
    cnt = _on_and_off(be, oracle, db, exp, cols, monkeypatch, capfd)

    def expected(c):
        G, cpw, _ = FORM[c]
        t = stop_step(c, a, clear, 4 * YLEN - 8 * nsub)
        waves = -(-NREADS // cpw)
        return (0, 0) if t is None else (waves, waves * (XLEN - 1 + G - t))
    if nsub == 9:
        assert cnt == (0, 0), (cols, cnt)
    elif be.name == "emu":
        assert cnt == expected(cols), (cols, nsub, cnt, expected(cols))
    else:
        assert cnt in [expected(c) for c in COLS], (cols, nsub, cnt, [expected(c) for c in COLS])


@pytest.fixture(scope="module")
def mixed(oracle):
    """128 reads at row 300 of their records: 7 exact ones among 121 with 14
    substitutions in their last 60 bases (seeded and predicted like the
    others, B = 600 - 112 < Bmin) and, 400 rows lower, a copy with 12 spread
    substitutions -- no 12-mer, so `clear` does not see it, but at 504 it
    outscores the first.  A wave of the 19-column form holds 16 candidates,
    one of the 10-column form 8: with 7 good ones none is free of a bad half,
    so no wave may stop, and one that did would lose the better copy."""
    rng = np.random.default_rng(16015)
    pairs = []
    for k in range(128):
        y = _rnd(rng, 150)
        if k % 19 == 3:
            pairs.append((np.concatenate([_rnd(rng, 300), y, _rnd(rng, 1550)]), y))
        else:
            first, second = _subs_at(rng, y, [91 + 4 * q for q in range(14)]), _subs_at(rng, y, _spread(150, 12))
            pairs.append((np.concatenate([_rnd(rng, 300), first, _rnd(rng, 400), second, _rnd(rng, 1000)]), y))
    assert sum(1 for k in range(128) if k % 19 == 3) == 7
    db = _db(pairs)
    rc, exp, _ = oracle.align(*db, oracle.params(), 4)
    assert rc == 0
    bad = [k for k in range(128) if k % 19 != 3]
    assert (exp["score"][bad] == 600 - 96).all() and (exp["bx"][bad] == 300 + 150 + 400 + 149).all()
    return db, exp


@pytest.mark.parametrize("cols", ["19", "10"])
def test_mixed_waves(be, oracle, mixed, cols, monkeypatch, capfd):
    """halves that must not stop (B < Bmin) beside halves that could: with more
    bad halves than waves have room to avoid, no wave stops, and every read
    keeps the lower, better copy"""
    db, exp = mixed
    assert _on_and_off(be, oracle, db, exp, cols, monkeypatch, capfd) == (0, 0)


def test_short_records_stay_off(be, oracle, monkeypatch, capfd):
    """700-row records: the LDS share of a half cannot hold the table at load
    factor 0.6, so the launch runs without the stop"""
    ref, rst = synth.make_reference_arr(96 * 700, 700, seed=77)
    q, qs = synth.make_reads_arr(ref, 96, 150, seed=78, frac_true=1.0)
    rc, exp, _ = oracle.align(ref, rst, q, qs, oracle.params(), 4)
    assert rc == 0 and int((exp["status"] == 1).sum()) >= 80
    assert _on_and_off(be, oracle, (ref, rst, q, qs), exp, "19", monkeypatch, capfd) == (0, 0)


# ---- nw_pairs: no predicted rows reach the kernel there, so the stop never
# runs; these check that the switch, the table and the new launch fields change
# nothing on that route (the stop itself is checked through the pipeline above)

@pytest.fixture(scope="module")
def golden_and_random(oracle, adversarial):
    """the golden NW pairs the packed kernel takes (reads of 12-160 bases, 40
    of them), 24 random pairs with planted reads, and every third adversarial pair"""
    rng = np.random.default_rng(16016)
    X, Y = [], []
    for g in golden_io.nw_pairs():
        if MER <= len(g["Y"]) <= 160 and 2 <= len(g["X"]) <= 2000 and len(X) < 40:
            X.append(g["X"].encode()); Y.append(g["Y"].encode())
    for k in range(24):
        y = _rnd(rng, 150)
        x = _rnd(rng, rng.integers(160, 2001)) if k % 3 == 0 else \
            np.concatenate([_rnd(rng, rng.integers(0, 900)), _subs_at(rng, y, rng.choice(150, 3, replace=False)),
                            _rnd(rng, rng.integers(0, 900))])
        X.append(x.tobytes()); Y.append(y.tobytes())
    for x, y in adversarial[0][::3]:
        X.append(x.tobytes()); Y.append(y.tobytes())
    return X, Y, [oracle.nw(x, y, text=False) for x, y in zip(X, Y)]


@pytest.mark.parametrize("onepass", [False, True], ids=["two", "one"])
@pytest.mark.parametrize("cols", COLS)
def test_pairs_route_unchanged(be, oracle, golden_and_random, cols, onepass, monkeypatch):
    X, Y, expected = golden_and_random
    runs = {}
    for stop in ("1", "0"):
        _set_form(monkeypatch, cols, stop)
        p = oracle.params(min_coverage=1e-9, min_identity=1e-9, want_paths=1,
                          flags=imsame_amd.FLAG_NW16_ONEPASS if onepass else 0)
        res, paths = be.nw_pairs(X, Y, p)
        for k, o in enumerate(expected):
            for f in FIELDS:
                assert int(res[k][f]) == int(o[f]), (f, k, cols, onepass, stop)
        runs[stop] = [_path(res, paths, k) for k in range(len(X))]
    assert runs["1"] == runs["0"]
