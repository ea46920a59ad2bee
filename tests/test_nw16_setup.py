"""The packed NW kernel's task setup (nw16_kernel.hip): candidate
fetch, stop table, stop scan, staging and column codes issue their loads in
batches, at clamped addresses instead of under predicates.  These are the
smallest shapes at which such loads can go wrong -- reads and records at every
offset mod 16 of their buffers, the first and the last of each buffer, lengths
around 16 and around the lanes per pair, launches of one and of an odd number
of candidates, planted reads on row 0, between probed rows and on a record's
last rows -- on the wave emulator (the same kernel source) and on the device,
against the oracle: every parity field, and the oracle's text for every
accepted path.  Through nw_pairs (no predicted rows) and through the pipeline
(predicted rows; the stop on and off), every column form forced."""
import numpy as np
import pytest

import imsame_amd
from imsame_amd import PARITY_FIELDS
from tests.test_nw16_stop import be  # noqa: F401  (the emulator / device fixture)
from tests.test_nw16_stop import (COLS, FIELDS, FORM, MER, STRIDE, XLEN, YLEN, NREADS, _path, _rnd, _set_form,
                                  _subs_at, bmin, clear_row, stop_step, uniform_set)

# record lengths around a 16-byte load and around the lanes per pair of every
# form (G = 8, 15/16, 30/32, 50), and the longest records with their neighbour
SHORT_X = (2, 8, 9, 15, 16, 17, 30, 31, 32, 33, 50, 51)
LONG_X = (2000, 1999)
_memo = {}


def _residues(lens):
    return {int(s) % 16 for s in np.cumsum([0] + list(lens[:-1]))}


def _record_for(rng, y, xl, where):
    """a record of xl rows: the read with 0-3 substitutions at `where` ("top",
    "bottom" or a random row) if it fits, else its first xl bases or random rows"""
    yl = len(y)
    if xl < yl:
        return y[:xl].copy() if xl % 2 else _rnd(rng, xl)
    c = _subs_at(rng, y, rng.choice(yl, int(rng.integers(0, 4)), replace=False))
    a = 0 if where == "top" else xl - yl if where == "bottom" else int(rng.integers(0, xl - yl + 1))
    return np.concatenate([_rnd(rng, a), c, _rnd(rng, xl - yl - a)])


def pair_set(ylens, seed):
    """one pair per read length given: the corner record lengths first, then
    lengths chosen so that the records start at every residue mod 16"""
    rng = np.random.default_rng(seed)
    xlens = list(SHORT_X) + list(LONG_X)
    while len(xlens) < len(ylens):
        xl, missing = int(rng.integers(150, 700)), set(range(16)) - _residues(xlens + [0])
        if missing:                                               # the next record starts at a residue not seen yet
            xl += (min(missing) - (sum(xlens) + xl)) % 16
        xlens.append(xl)
    assert _residues(xlens) == set(range(16)), sorted(_residues(xlens))
    X, Y = [], []
    for k, (yl, xl) in enumerate(zip(ylens, xlens)):
        y = _rnd(rng, yl)
        X.append(_record_for(rng, y, xl, ("top", "bottom", "any")[k % 3]).tobytes())
        Y.append(y.tobytes())
    return X, Y


# reads of one length (the 19-column form takes only these) and of every length
# around a 16-byte load, a 12-mer and the forms' column counts; an odd number of
# pairs, so the last wave has an absent B half and idle groups
def _ordered(lens):
    """the lengths in an order in which the reads start at as many residues mod 16 as they can"""
    left, out, seen, cum = list(lens[1:]), [lens[0]], {0}, lens[0]
    while left:
        seen.add(cum % 16)
        v = next((v for v in left if (cum + v) % 16 not in seen), left[0])
        left.remove(v); out.append(v); cum += v
    return out


UNI = [150] * 37
MIXED = _ordered([13] + [150] * 3 + [12, 13, 15, 16, 17, 29, 149, 150, 151, 160] * 3 + [150, 149, 150])
MIXED_K3 = _ordered([min(v, 150) if v != 151 else 147 for v in MIXED])   # the 3-column form's reads end at 150
MID = _ordered([161, 200, 170, 163, 199, 176, 161, 185, 200, 177, 192, 161, 168, 200, 171, 180, 161, 190, 165,
                162, 175, 200, 188, 161, 194, 169, 173, 182, 197])


def _pairs_case(oracle, key):
    if key not in _memo:
        ylens = {"uni": UNI, "mixed": MIXED, "mixed3": MIXED_K3, "mid": MID}[key]
        X, Y = pair_set(ylens, 16200 + len(ylens))
        assert len(X) % 2 == 1
        if key != "uni":
            assert _residues([len(y) for y in Y]) == set(range(16))
        _memo[key] = (X, Y, [oracle.nw(x, y, text=True) for x, y in zip(X, Y)])
    return _memo[key]


def _check_pairs(be, oracle, X, Y, exp, tag):
    p = oracle.params(min_coverage=1e-9, min_identity=1e-9, want_paths=1)
    res, paths = be.nw_pairs(X, Y, p)
    n_text = 0
    for k, o in enumerate(exp):
        for f in FIELDS:
            assert int(res[k][f]) == int(o[f]), (tag, f, k, len(X[k]), len(Y[k]))
        if res[k]["status"] == 1:
            txt, ident = imsame_amd.render(X[k], Y[k], res[k], np.array(_path(res, paths, k), dtype=np.uint32))
            assert txt == o["text"] and ident == o["identities"], (tag, k)
            n_text += 1
    return n_text


@pytest.mark.parametrize("stop", ["1", "0"])
@pytest.mark.parametrize("cols,key", [("19", "uni"), ("10", "uni"), ("10", "mixed"), ("5", "mixed"), ("3", "mixed3"),
                                      ("10", "mid")])
def test_pairs_corners(be, oracle, cols, key, stop, monkeypatch):  # noqa: F811
    """nw_pairs: every corner length and offset in one launch (records of 2
    to 2,000 rows in one wave: xmin != xmax), then launches of a single
    candidate -- the buffers' first pair and their last, which ends at the last
    byte of both"""
    X, Y, exp = _pairs_case(oracle, key)
    _set_form(monkeypatch, cols, stop)
    assert _check_pairs(be, oracle, X, Y, exp, (cols, key)) >= len(X) // 2
    if stop == "1":
        for k in (0, len(X) - 1, len(SHORT_X)):
            _check_pairs(be, oracle, X[k:k + 1], Y[k:k + 1], exp[k:k + 1], (cols, key, "alone", k))
        _check_pairs(be, oracle, X[-4:], Y[-4:], exp[-4:], (cols, key, "tail"))


# ----------------------------------------------------------------- the pipeline

def pipeline_set(ylen, seed, mixed):
    """80 records of about 2,000 rows (one of exactly 2,000, so the launch's
    LDS share holds the stop's table; the others a few rows shorter, so the
    records start at every residue mod 16) with one read planted in each: on row
    0, between probed rows (rows 4k+1 .. 4k+3), on the record's last rows, in
    the top block of the scan (rows < 200) and anywhere; a short read (13 bases and more) that
    seeds nothing stands first in the query and after every fifth read, so the
    reads start at every residue too.  mixed: some reads of ylen - 1 and of 29
    bases (not for the 19-column form, which takes one length only)."""
    rng = np.random.default_rng(seed)
    recs, reads = [], [_rnd(rng, 13)]
    for k in range(80):
        xl = XLEN if k == 0 else XLEN - int(rng.integers(0, 16)) if k < 79 else XLEN - 1
        yl = ylen if not mixed else ylen - 1 if k % 7 == 3 else 29 if k % 11 == 5 else ylen
        y = _rnd(rng, yl)
        kind = k % 8
        a = (0, 4 * int(rng.integers(1, 400)) + 1, 4 * int(rng.integers(1, 400)) + 2, 4 * int(rng.integers(1, 400)) + 3,
             xl - yl, xl - yl - int(rng.integers(1, 150)), int(rng.integers(1, 200)), int(rng.integers(0, xl - yl)))[kind]
        c = _subs_at(rng, y, rng.choice(yl, int(rng.integers(0, 4)), replace=False)) if yl > 40 else y
        recs.append(np.concatenate([_rnd(rng, a), c, _rnd(rng, xl - yl - a)]))
        reads.append(y)
        if k % 5 == 4 and k < 79:
            missing = set(range(16)) - _residues([len(r) for r in reads] + [0])
            cum = sum(len(r) for r in reads)
            reads.append(_rnd(rng, 13 + ((min(missing) - cum - 13) % 16 if mixed and missing else 0)))
    assert _residues([len(x) for x in recs]) == set(range(16))
    assert _residues([len(y) for y in reads]) == set(range(16))
    return recs, reads


def _pipeline_case(oracle, key, make):
    if key not in _memo:
        recs, reads = make()
        ref, q = np.concatenate(recs), np.concatenate(reads)
        rst = np.cumsum([0] + [len(x) for x in recs[:-1]]).astype(np.uint64)
        qs = np.cumsum([0] + [len(y) for y in reads[:-1]]).astype(np.uint64)
        rc, exp, _ = oracle.align(ref, rst, q, qs, oracle.params(), 4)
        assert rc == 0
        text = {k: oracle.nw(recs[int(exp[k]["db_seq"])].tobytes(), reads[k].tobytes(), text=True)["text"]
                for k in range(len(reads)) if exp[k]["status"] == 1}
        _memo[key] = (recs, reads, (ref, rst, q, qs), exp, text)
    return _memo[key]


def _run_pipeline(be, oracle, case, cols, monkeypatch, capfd):
    """stop on and off: the oracle's parity fields and text both times; the counters of the run with the stop on"""
    recs, reads, db, exp, text = case
    cnts = {}
    for stop in ("1", "0"):
        _set_form(monkeypatch, cols, stop)
        got, paths, cnts[stop] = be.align(*db, oracle.params(), capfd)
        for f in PARITY_FIELDS:
            assert np.array_equal(got[f], exp[f]), (f, cols, stop)
        for k, t in text.items():
            txt, _ = imsame_amd.render(recs[int(got[k]["db_seq"])], reads[k], got[k],
                                       np.array(_path(got, paths, k), dtype=np.uint32))
            assert txt == t, (cols, stop, k)
    assert cnts["0"] == (0, 0), (cols, cnts)
    return cnts["1"]


@pytest.mark.parametrize("cols", COLS)
def test_pipeline_corners(be, oracle, cols, monkeypatch, capfd):  # noqa: F811
    """the pipeline carries the predicted rows: table, scan and stop run on
    reads and records at every offset, planted at the scan's corner rows"""
    mixed = cols != "19"
    case = _pipeline_case(oracle, ("pipe", mixed), lambda: pipeline_set(YLEN, 16300, mixed))
    assert len(case[4]) >= 64                                      # candidates enough for predicted rows
    cnt = _run_pipeline(be, oracle, case, cols, monkeypatch, capfd)
    assert cnt[0] > 0, (cols, cnt)                                 # the stop did run


def test_pipeline_mid(be, oracle, monkeypatch, capfd):  # noqa: F811
    """reads of 161-200 bases (the mid form shares the setup; it runs without the stop)"""
    def make():
        rng = np.random.default_rng(16400)
        recs, reads = [], [_rnd(rng, 13)]
        for k in range(72):
            yl, xl = int(rng.integers(161, 201)), XLEN - int(rng.integers(0, 16)) if k else XLEN
            y = _rnd(rng, yl)
            a = (0, xl - yl, int(rng.integers(0, xl - yl)))[k % 3]
            recs.append(np.concatenate([_rnd(rng, a), _subs_at(rng, y, rng.choice(yl, 3, replace=False)), _rnd(rng, xl - yl - a)]))
            reads.append(y)
        return recs, reads
    case = _pipeline_case(oracle, ("pipe", "mid"), make)
    assert len(case[4]) >= 64
    assert _run_pipeline(be, oracle, case, "10", monkeypatch, capfd) == (0, 0)


# ---- `clear` and the waves that cannot stop, through the counters

def _row_with_phase(cols, phase):
    """a row = phase mod 4 at which the stop's step depends on `clear` to the
    row: with ylen left out of the formula the wave would stop elsewhere"""
    for a in range(200, 600):
        if a % STRIDE != phase:
            continue
        clear = a + max(j for j in range(YLEN - MER + 1) if (a + j) % STRIDE == 0) + 1
        t = stop_step(cols, a, clear, 4 * YLEN)
        if t is not None and t != stop_step(cols, a, clear, 4 * YLEN, drop_ylen=True):
            return a
    raise AssertionError("no such row")


def _uniform(oracle, key, a, nsub, seed):
    if key not in _memo:
        pairs, clear = uniform_set(oracle, a, nsub, seed)
        for x, y in pairs:
            assert clear_row(x, y) == clear
        recs, reads = [x for x, _ in pairs], [y for _, y in pairs]
        _memo[key] = (clear, _pipeline_case(oracle, (key, "db"), lambda: (recs, reads)))
    return _memo[key]


@pytest.mark.parametrize("cols", COLS)
def test_clear_between_probed_rows(be, oracle, cols, monkeypatch, capfd):  # noqa: F811
    """reads that start between probed rows: every wave of a uniform set stops
    at the step that clear_row's `clear` gives, so the counters are known"""
    phase = 1 + COLS.index(cols) % 3
    a = _row_with_phase(cols, phase)
    clear, case = _uniform(oracle, ("uni", cols), a, 0, 16500 + phase)
    cnt = _run_pipeline(be, oracle, case, cols, monkeypatch, capfd)

    def expected(c):
        G, cpw, _ = FORM[c]
        t = stop_step(c, a, clear, 4 * YLEN)
        waves = -(-NREADS // cpw)
        return (0, 0) if t is None else (waves, waves * (XLEN - 1 + G - t))
    if be.name == "emu":
        assert cnt == expected(cols), (cols, a, cnt, expected(cols))
    else:
        # IMSAME_NW_K is a wish on the device: plan_nw takes the 3- and 5-column forms
        # only where a launch is small enough for them and may run another form
        # (test_nw16_stop.py::test_stop_step), so any form's counters are right there;
        # the emulator runs the form asked for and pins `clear` to the row
        assert cnt in [expected(c) for c in COLS], (cols, a, cnt)


@pytest.mark.parametrize("cols", COLS)
def test_window_at_the_bottom_never_stops(be, oracle, cols, monkeypatch, capfd):  # noqa: F811
    """reads on the last rows of their records: the window ends at the
    record's bottom, no checkpoint step is left to test the stop at, and the
    wave skips the stop's setup -- counters (0, 0), results the oracle's, stop
    on and off"""
    a = XLEN - YLEN
    clear, case = _uniform(oracle, ("bottom",), a, 0, 16600)
    assert 4 * YLEN >= bmin(YLEN, -5, -2) and stop_step(cols, a, clear, 4 * YLEN) is None
    assert _run_pipeline(be, oracle, case, cols, monkeypatch, capfd) == (0, 0)
