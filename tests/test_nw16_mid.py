"""Reads of 161 .. 320 bases ("mid" reads) on the packed NW kernel
(nw16_kernel.hip: the 10-column form with G = 17 .. 32 lanes per candidate
pair and a 32-step checkpoint interval) and in the short-read scheduling
(imsame_dev.hip: class cut, lanes, round 1b, split rounds, pipelines).

Every case runs twice: on the CPU wave emulator (the kernel source) and,
marked `gpu`, on the device.  Every result field is compared with the oracle,
paths with the one-pass form's, rendered text with the oracle's.  Which kernel
ran is asserted: the emulator's launch counter, the device's diagnostics line
(pair launches) and launch masks (whole calls).

The emulator's host code (tests/emu/wave_emu.cpp) is as it was: it reaches the
mid form through the kernel source (nw16_fits admits the launch and honours
IMSAME_NW_MID; nw16_wave's 10-column form hands a launch shaped for mid reads
to the mid variant), it still cuts a call's classes at 160 bases (so the class
cut at 320 is checked on the device only) and it still takes IMSAME_NW_K=5."""
import contextlib
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import imsame_amd
from imsame_amd import PARITY_FIELDS
from tests import synth
from tests.emu_bind import Emu
from tests.oracle_bind import Oracle

FIELDS = ("score", "bx", "by", "length", "identities", "igaps", "egaps", "head_x", "head_y")
ACGT = synth.ACGT


@contextlib.contextmanager
def _env(kv):
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update(kv)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


class _EmuBackend:
    name = "emu"

    def __init__(self):
        self.emu = Emu.load()
        self.nwp = self.emu.lib.emu_nwp_count
        self.nwp.restype = C.c_uint32
        self.nwp.argtypes = [C.c_void_p]
        self.redo = self.emu.lib.emu_redo_count
        self.redo.restype = C.c_uint32

    def nw_pairs(self, X, Y, p, capfd=None):
        """(results, paths, {"long": the packed long-read kernel ran, "redo": waves that redid their band})"""
        p.want_paths = 1
        self.nwp(None), self.redo()
        rc, res, paths, fl = self.emu.nw_pairs(X, Y, p, paths_cap=sum(len(x) + len(y) for x, y in zip(X, Y)) + 16)
        assert rc == 0 and fl == 0
        n = self.nwp(None)
        assert n in (0, 1)
        return res, paths, {"long": n == 1, "redo": self.redo(), "shape": None}

    def align(self, ref, rst, q, qs, p, n_threads, want_paths=False, paths_cap=None):
        self.nwp(None)
        cap = (paths_cap if paths_cap is not None else 8 * len(qs) + 1024) if want_paths else 0
        p.want_paths = 1 if want_paths else 0
        rc, res, paths, st = self.emu.align(ref, rst, q, qs, p, n_threads, paths_cap=cap)
        assert rc == 0
        return res, paths, {"n_long": self.nwp(None), "n_nw": st.n_nw, "st": None}


class _GpuBackend:
    name = "gpu"

    def __init__(self):
        self.dev = imsame_amd.Device(0)
        self.loaded = None

    def close(self):
        self.dev.close()

    def nw_pairs(self, X, Y, p, capfd=None):
        with _env({"IMSAME_NW_PROF": "1"}):          # the launch's diagnostics line names its kernel and shape
            capfd.readouterr()
            res, paths, _ = self.dev.nw_pairs(X, Y, p, want_paths=True)
            err = capfd.readouterr().err
        raw = [l.split() for l in err.splitlines() if l.startswith("[nwprof-raw]")]
        lng = [l for l in err.splitlines() if l.startswith("[nwprof-long] kernel nwp")]
        shape = None
        if raw:
            w = raw[0]
            shape = tuple(int(w[w.index(k) + 1]) for k in ("G", "GPW", "k"))
        assert len(raw) + len(lng) <= 1
        return res, paths, {"long": bool(lng), "redo": None, "shape": shape}

    def align(self, ref, rst, q, qs, p, n_threads, want_paths=False, paths_cap=None):
        key = (id(ref), id(q))
        if self.loaded != key:
            self.dev.index(ref, rst)
            self.dev.set_query(q, qs)
            self.loaded = key
        res, paths, st = self.dev.align(n_threads=n_threads, params=p, want_paths=want_paths, paths_cap=paths_cap)
        nl = min(int(st.nw_launches), 64)
        return res, paths, {"n_long": bin(st.launch_nwp).count("1"), "n_nw": st.n_nw, "st": st, "all": (1 << nl) - 1}


@pytest.fixture(scope="module", params=["emu", pytest.param("gpu", marks=pytest.mark.gpu)])
def be(request):
    if request.param == "emu":
        yield _EmuBackend()
    else:
        b = _GpuBackend()
        yield b
        b.close()


def _params(oracle, flags=0, **kw):
    return oracle.params(min_coverage=1e-9, min_identity=1e-9, want_paths=1, flags=flags, **kw)


def _path(res, paths, k):
    r = res[k]
    return paths[r["path_off"]:r["path_off"] + r["path_len"]].tolist()


def _mutate(rng, y, sub=0.03, indel=True):
    y = y.copy()
    m = rng.random(len(y)) < sub
    y[m] = ACGT[(np.searchsorted(ACGT, y[m]) + rng.integers(1, 4, int(m.sum()))) % 4]
    if indel and len(y) > 20:
        o = int(rng.integers(5, len(y) - 5))
        y = np.concatenate([y[:o], ACGT[rng.integers(0, 4, 2)], y[o:]]) if rng.random() < 0.5 else \
            np.concatenate([y[:o], y[o + 2:]])
    return y


def _launch(seed, ylens, xlens):
    """One pair launch: pair k has a read of ylens[k] bases and a record of
    xlens[k]; records at least as long as the read hold a mutated copy of it
    (a real path), shorter ones are cut from the read, every fourth is random."""
    rng = np.random.default_rng(seed)
    X, Y = [], []
    for k, (yl, xl) in enumerate(zip(ylens, xlens)):
        y = ACGT[rng.integers(0, 4, yl)]
        if k % 4 == 3:
            x = ACGT[rng.integers(0, 4, xl)]
        elif xl >= yl + 4:
            c = _mutate(rng, y)[:xl]
            o = int(rng.integers(0, xl - len(c) + 1))
            x = np.concatenate([ACGT[rng.integers(0, 4, o)], c, ACGT[rng.integers(0, 4, xl - o - len(c))]])
        else:
            o = int(rng.integers(0, max(yl - xl, 0) + 1))
            x = np.resize(y[o:o + xl], xl)
        assert len(x) == xl and len(y) == yl
        X.append(x.tobytes()); Y.append(y.tobytes())
    return X, Y


def _cyc(vals, n):
    return [vals[k % len(vals)] for k in range(n)]


def _shape(ymax):
    G = -(-ymax // 10)
    return G, 64 // G


def _boundary_case(ymax):
    """Longest read ymax, shorter reads mixed in (40, 150, 161: lockstep
    garbage columns), 4 waves' worth + 1 candidates: an odd count (the absent
    B half) whose last wave leaves every group but one idle.  ymax = 320:
    every length a multiple of 10 (the LAST form)."""
    G, GPW = _shape(ymax)
    n = 4 * GPW + 1
    mix = [320, 40, 150, 160, 300, 320, 250] if ymax == 320 else [ymax, 40, 150, min(161, ymax), ymax - 1, ymax, 100]
    return _launch(1000 + ymax, _cyc(mix, n), _cyc([400, 150, 331, 97, 200, 161, 48, 410, 149], n))


CASES = {f"y{y}": (lambda y=y: _boundary_case(y)) for y in (161, 170, 210, 211, 250, 300, 319, 320)}
# records against the skew of G = 32: 2 .. 64 rows (the skewed start and the
# end overlap), mixed with ~150 and ~400 rows in one wave (several checkpoint
# intervals, xmax - xmin end steps); read lengths not multiples of 10
CASES["skew320"] = lambda: _launch(77, _cyc([320, 161, 319, 250, 40, 320, 311], 13),
                                   [2, 12, 31, 32, 33, 64, 150, 400, 64, 2, 33, 149, 410])
CASE_YMAX = {**{f"y{y}": y for y in (161, 170, 210, 211, 250, 300, 319, 320)}, "skew320": 320}

_cache = {}


def _case(oracle, key):
    if key not in _cache:
        X, Y = CASES[key]()
        _cache[key] = (X, Y, [oracle.nw(x, y, text=True) for x, y in zip(X, Y)])
    return _cache[key]


def _check(res, paths, X, Y, exp, ref_paths, tag):
    n_text = 0
    for k, o in enumerate(exp):
        for f in FIELDS:
            assert int(res[k][f]) == int(o[f]), (tag, f, k, len(X[k]), len(Y[k]))
        if res[k]["status"] == 1:
            pk = _path(res, paths, k)
            if ref_paths is not None:
                assert pk == ref_paths[k], (tag, k)
            txt, ident = imsame_amd.render(X[k], Y[k], res[k], np.array(pk, dtype=np.uint32))
            assert txt == o["text"] and ident == o["identities"], (tag, k)
            n_text += 1
    return n_text


def _assert_mid(be, info, ymax, tag):
    """the launch ran the packed kernel's mid form: not the packed long-read
    kernel and, on the device, a packed launch at all (the diagnostics line of
    a packed launch, absent for nwl_kernel and the int32 kernel) of the mid
    shape: G = ceil(ymax / 10) lanes per pair, 64 / G pairs, 10 columns"""
    assert not info["long"], tag
    if be.name == "gpu":
        assert info["shape"] is not None, tag
        assert info["shape"] == (*_shape(ymax), 10), (tag, info["shape"])


@pytest.mark.parametrize("key", list(CASES))
def test_mid_pair_launches(be, oracle, key, monkeypatch, capfd):
    """Group boundaries (G = 17 .. 32, 3 and 2 groups per wave) and records
    against the skew: the mid form runs (not the long-read kernel), two passes
    and one pass, bands 0 and 40 (the redo over 4 bands and from row 1) give
    the oracle's rows, the one-pass paths and the oracle's text; with
    IMSAME_NW_MID=0 the long kernel runs, with equal rows and paths."""
    X, Y, exp = _case(oracle, key)
    ymax = CASE_YMAX[key]
    assert max(len(y) for y in Y) == ymax
    res1, paths1, info = be.nw_pairs(X, Y, _params(oracle, imsame_amd.FLAG_NW16_ONEPASS), capfd)
    _assert_mid(be, info, ymax, key)                  # fails without the mid form
    ref = [_path(res1, paths1, k) if res1[k]["status"] == 1 else None for k in range(len(X))]
    assert _check(res1, paths1, X, Y, exp, None, (key, "one-pass")) >= len(X) // 2
    for band in (None, "0", "40"):
        if band is not None:
            monkeypatch.setenv("IMSAME_NW_BAND", band)
        res, paths, info = be.nw_pairs(X, Y, _params(oracle), capfd)
        _assert_mid(be, info, ymax, (key, band))
        _check(res, paths, X, Y, exp, ref, (key, "two-pass", band))
        if band == "0" and info["redo"] is not None and max(len(x) for x in X) > 100:
            assert info["redo"] > 0, key
    monkeypatch.delenv("IMSAME_NW_BAND")
    monkeypatch.setenv("IMSAME_NW_MID", "0")
    res, paths, info = be.nw_pairs(X, Y, _params(oracle), capfd)
    assert info["long"], key
    _check(res, paths, X, Y, exp, ref, (key, "off"))


@pytest.mark.gpu
def test_mid_ignores_column_switch(gdev, oracle, monkeypatch, capfd):
    """IMSAME_NW_K keeps its meaning up to 160 bases and is ignored above:
    the 5- and 3-column forms cannot hold CK + G <= 64 there.  Device only:
    the emulator's host code takes IMSAME_NW_K=5 whatever the length."""
    X, Y, exp = _case(oracle, "y250")
    for k in ("5", "3"):
        monkeypatch.setenv("IMSAME_NW_K", k)
        res, paths, info = gdev.nw_pairs(X, Y, _params(oracle), capfd)
        _assert_mid(gdev, info, 250, ("y250", "K", k))
        _check(res, paths, X, Y, exp, None, ("y250", "K", k))


# int16 limit: (id, xmax, egap, igap or None = the strongest the range proof
# admits for 10 columns and reads of 320 bases).  600 x -8 admits no launch at
# all: |eg| (xmax + 64 + 320 + 2) alone is 7888 of the 8191 - 16 - 1280 = 6895
# left, nw16_limit_igap is +993 -- so that shape must take the long kernel at
# any gap penalty; 400 x -8 is the nearest shape with that extension penalty
# that fits.
LIMITS = [("3000_e2", 3000, -2, None), ("600_e8", 600, -8, None), ("400_e8", 400, -8, None),
          ("3059_default", 3059, -2, -5)]


@pytest.mark.parametrize("cid,xmax,eg,ig", LIMITS, ids=[c[0] for c in LIMITS])
def test_mid_at_range_limit(be, oracle, cid, xmax, eg, ig, capfd):
    """synth.adversarial_short_pairs at 320 bases, at the limit of nw16_fits
    (R <= 8191 with ycols = 320): every field equals the oracle's on the mid
    form; one step past the limit the launch takes the long kernel, same
    results"""
    X, Y = synth.adversarial_short_pairs(xmax, 320)
    lim = synth.nw16_limit_igap(10, xmax, 320, eg)

    def run(ig_, xs, want_long):
        p = _params(oracle, igap=ig_, egap=eg)
        res, _, info = be.nw_pairs(xs, Y, p, capfd)
        assert info["long"] == want_long, (cid, ig_, eg, info)
        if not want_long:
            _assert_mid(be, info, 320, (cid, ig_, eg))
        for k, (x, y) in enumerate(zip(xs, Y)):
            o = oracle.nw(x, y, igap=ig_, egap=eg, text=False)
            for f in FIELDS:
                assert int(res[k][f]) == int(o[f]), (cid, f, k, ig_, eg)

    if lim > 0:                                   # no open penalty fits: the long kernel at the mildest one
        assert cid == "600_e8" and lim == 993
        run(0, X, True)
        return
    if ig is None:
        ig = lim
        run(ig, X, False)
        run(ig - 1, X, True)
    else:                                         # default gaps: the record cap is the limit
        assert lim == ig and synth.nw16_limit_igap(10, xmax + 1, 320, eg) > ig
        run(ig, X, False)
        X2, _ = synth.adversarial_short_pairs(xmax + 1, 320)
        run(ig, X2, True)


# ------------------------------------------------------------ whole pipeline
def _var_reads(ref, lens, seed, frac_true=0.7, rec=0):
    """reads of the given lengths: frac_true drawn from the reference (rec:
    from inside one record of that length) with 1 % substitutions and, one in
    four, a 2-base indel; the rest random"""
    rng = np.random.default_rng(seed)
    out = []
    for L in lens:
        L = int(L)
        if rng.random() < frac_true:
            o = int(rng.integers(0, len(ref) - L - 8))
            if rec:
                o = int(rng.integers(0, len(ref) // rec)) * rec + int(rng.integers(0, rec - L - 8))
            y = _mutate(rng, ref[o:o + L + 4], sub=0.01, indel=rng.random() < 0.25)[:L]
        else:
            y = ACGT[rng.integers(0, 4, L)]
        assert len(y) == L
        out.append(y)
    qs = np.concatenate([[0], np.cumsum([len(y) for y in out])[:-1]]).astype(np.uint64)
    return np.concatenate(out), qs


_wl = {}


def _workload(oracle, size, rec, mix, T):
    """(ref, rst, q, qs, expected rows for n_threads T); size "big": 300 kbp
    and 3,000 reads (the device), "small": 60 kbp and 64 reads (the emulator)"""
    total, n = (300_000, 3_000) if size == "big" else (60_000, 64)
    key = (size, rec, mix)
    if key not in _wl:
        ref, rst = synth.make_reference_arr(total, rec, seed=31 + rec)
        rng = np.random.default_rng(5 + rec)
        if mix == "u250":
            lens, ft = np.full(n, 250), 0.7
        elif mix == "v454":
            lens, ft = rng.integers(100, 321, n), 0.7
        else:                       # "mixed": 100 .. 600, every read drawn from inside a record
            lens, ft = rng.integers(100, 601, 96), 1.0
        q, qs = _var_reads(ref, lens, seed=17 + rec, frac_true=ft, rec=rec if mix == "mixed" else 0)
        _wl[key] = [ref, rst, q, qs, {}]
    w = _wl[key]
    if T not in w[4]:
        rc, exp, _ = oracle.align(w[0], w[1], w[2], w[3], oracle.params(), T)
        assert rc == 0
        w[4][T] = exp
    return w[0], w[1], w[2], w[3], w[4][T]


def _size(be):
    return "big" if be.name == "gpu" else "small"


def _rows_equal(got, exp, tag):
    for f in PARITY_FIELDS:
        assert np.array_equal(got[f], exp[f]), (tag, f)


@pytest.mark.parametrize("T", [1, 4])
@pytest.mark.parametrize("mix", ["u250", "v454"])
@pytest.mark.parametrize("rec", [2000, 3000])
def test_mid_align(be, oracle, rec, mix, T, monkeypatch):
    """uniform 250-base reads and lengths 100 .. 320 against 2 and 3 kbp
    records: all result fields equal the oracle's and every launch is a
    packed one, none the long-read kernel's (fails without the feature); with
    IMSAME_NW_MID=0 equal rows from the long kernel"""
    ref, rst, q, qs, exp = _workload(oracle, _size(be), rec, mix, T)
    assert (exp["status"] == 1).sum() > len(qs) // 2
    got, _, info = be.align(ref, rst, q, qs, oracle.params(), T)
    _rows_equal(got, exp, (rec, mix, T))
    assert info["n_long"] == 0, (rec, mix, T)
    if info["st"] is not None:
        st = info["st"]
        assert st.nw_launches > 0 and st.launch_pk == info["all"] and st.launch_nwp == 0
        assert st.launch_k5 == 0 and st.launch_k3 == 0 and st.launch_k19 == 0
    monkeypatch.setenv("IMSAME_NW_MID", "0")
    got, _, info = be.align(ref, rst, q, qs, oracle.params(), T)
    _rows_equal(got, exp, (rec, mix, T, "off"))
    assert info["n_long"] > 0


@pytest.mark.gpu
def test_mid_mixed_classes(gdev, oracle):
    """lengths 100 .. 600 in one call: reads up to 320 bases in packed
    launches, longer ones in the long-read kernel's.  Every read is drawn from
    the database and accepted at its first candidate (n_nw == reads, checked),
    so the long launches' candidates must number exactly the reads above 320.
    Device only: the emulator's host code cuts the classes at 160."""
    ref, rst, q, qs, exp = _workload(oracle, "small", 2000, "mixed", 4)
    lens = np.diff(np.concatenate([qs, [len(q)]]).astype(np.int64))
    n_long = int((lens > 320).sum())
    assert n_long > 10 and int(((lens > 160) & (lens <= 320)).sum()) > 10 and (exp["status"] == 1).all()
    got, _, info = gdev.align(ref, rst, q, qs, oracle.params(), 4)
    _rows_equal(got, exp, "mixed")
    assert info["n_nw"] == len(qs)
    assert info["n_long"] > 0
    st = info["st"]
    assert st.launch_pk != 0 and st.launch_nwp != 0 and (st.launch_pk & st.launch_nwp) == 0
    cand = [int(st.launch_cand[k]) for k in range(int(st.nw_launches))]
    assert sum(c for k, c in enumerate(cand) if (st.launch_nwp >> k) & 1) == n_long
    assert sum(c for k, c in enumerate(cand) if (st.launch_pk >> k) & 1) == len(qs) - n_long


@pytest.mark.gpu
def test_mid_paths_rewalk(gdev, oracle, monkeypatch):
    """a path arena too small for the call: the lost paths of mid reads are
    walked again (rewalk_lost, which the emulator does not have) and equal the
    big-arena run's"""
    ref, rst, q, qs, exp = _workload(oracle, "big", 2000, "u250", 4)
    big, pbig, _ = gdev.align(ref, rst, q, qs, oracle.params(), 4, want_paths=True, paths_cap=600 * len(qs))
    _rows_equal(big, exp, "paths-big")
    monkeypatch.setenv("IMSAME_DEV_PATHS_CAP", "3000")
    small, psmall, info = gdev.align(ref, rst, q, qs, oracle.params(), 4, want_paths=True, paths_cap=600 * len(qs))
    assert info["st"].n_rewalk > 0 and info["st"].launch_nwp == 0
    _rows_equal(small, exp, "paths-small")
    n = 0
    for k in range(len(qs)):
        if exp[k]["status"] == 1:
            assert _path(small, psmall, k) == _path(big, pbig, k), k
            n += 1
    assert n > len(qs) // 2


# ----------------------------------------------- device only: the scheduler
@pytest.fixture(scope="module")
def gdev():
    b = _GpuBackend()
    yield b
    b.close()


@pytest.mark.gpu
def test_mid_lanes(gdev, oracle, monkeypatch):
    """a call of 250-base reads takes lanes (it was forced to one): equal
    rows and paths, and imsame_dev_align_parts delivers the same rows"""
    ref, rst, q, qs, exp = _workload(oracle, "big", 2000, "u250", 4)
    monkeypatch.setenv("IMSAME_LANE_MIN", "1000")
    monkeypatch.setenv("IMSAME_LANES", "1")
    r1, p1, i1 = gdev.align(ref, rst, q, qs, oracle.params(), 4, want_paths=True, paths_cap=600 * len(qs))
    assert i1["st"].lanes == 1
    monkeypatch.setenv("IMSAME_LANES", "2")
    r2, p2, i2 = gdev.align(ref, rst, q, qs, oracle.params(), 4, want_paths=True, paths_cap=600 * len(qs))
    assert i2["st"].lanes == 2                      # fails without the feature
    assert i2["st"].launch_nwp == 0 and i2["st"].launch_pk == i2["all"]
    _rows_equal(r1, exp, "lanes1")
    _rows_equal(r2, exp, "lanes2")
    for k in range(len(qs)):
        if exp[k]["status"] == 1:
            assert _path(r2, p2, k) == _path(r1, p1, k), k
    r3, parts, st3 = gdev.dev.align_parts(n_threads=4, params=oracle.params())
    assert st3.lanes == 2 and len(parts) >= 2
    _rows_equal(r3, exp, "parts")
    monkeypatch.setenv("IMSAME_NW_MID", "0")        # the switch brings the single lane back
    r4, _, i4 = gdev.align(ref, rst, q, qs, oracle.params(), 4)
    assert i4["st"].lanes == 1 and i4["st"].launch_nwp != 0
    _rows_equal(r4, exp, "lanes-off")


@pytest.mark.gpu
def test_mid_lane_cap(gdev, oracle, monkeypatch):
    """the lanes of a mid call are cut where free HBM could not hold a
    persistent mid arena per lane beside 8 GB of headroom (mid_lane_cap):
    2 kbp records on 256 CUs need 3072 slots x (2032 steps x 64 x 3 + 65
    checkpoints x 45 x 64) dwords = 7.1 GB per lane, so 8 GiB + 2.5 arenas
    admit 2 of 3 lanes, and less than the headroom one; same rows."""
    ref, rst, q, qs, exp = _workload(oracle, "big", 2000, "u250", 4)
    per_lane = 256 * 3 * 4 * (2032 * 64 * 3 + 65 * 45 * 64) * 4
    monkeypatch.setenv("IMSAME_LANE_MIN", "500")
    monkeypatch.setenv("IMSAME_LANES", "3")
    for hbm, lanes in ((None, 3), ((8 << 30) + 5 * per_lane // 2, 2), (1 << 30, 1)):
        if hbm is not None:
            monkeypatch.setenv("IMSAME_DEBUG_MID_HBM", str(hbm))
        got, _, info = gdev.align(ref, rst, q, qs, oracle.params(), 4)
        assert info["st"].lanes == lanes, (hbm, info["st"].lanes)
        _rows_equal(got, exp, ("lane-cap", lanes))


# (name, environment of the form, of its off form, the IMSAME_DEBUG_ROUNDS line that proves the form ran)
SCHED = [
    ("pipes", {"IMSAME_PIPES": "1"}, {"IMSAME_PIPES": "0"}, "[round 1 pipes]"),
    ("round1b", {"IMSAME_PIPES": "0", "IMSAME_SPLIT_ROUNDS": "0"},
     {"IMSAME_PIPES": "0", "IMSAME_SPLIT_ROUNDS": "0", "IMSAME_ROUND1B": "0"}, "[round 1b]"),
    ("split", {"IMSAME_PIPES": "0", "IMSAME_SPLIT_MIN": "64"}, {"IMSAME_PIPES": "0", "IMSAME_SPLIT_ROUNDS": "0"},
     " split] "),
]


@pytest.mark.gpu
@pytest.mark.parametrize("name,on,off,line", SCHED, ids=[s[0] for s in SCHED])
def test_mid_scheduler_forms(gdev, oracle, name, on, off, line, capfd):
    """the forms the scheduler can now take with 250-base reads -- independent
    pipelines, round 1b, split rounds -- against their off forms and the
    oracle, each side once more with a stalled stream (IMSAME_DEBUG_STALL):
    the mid class passes the ordering checks the short class passes.  The
    debug lines prove that the form ran (it could not before: the class was
    the long one) and that the stalls were enqueued."""
    ref, rst, q, qs, exp = _workload(oracle, "big", 2000, "u250", 4)
    base = {"IMSAME_LANES": "1", "IMSAME_DEBUG_ROUNDS": "1"}
    nw = {}
    for side, env in (("on", on), ("off", off)):
        for stall in (None, "A:3000", "B:3000"):        # us: several times this call's longest launch
            e = {**base, **env}
            if stall:
                e["IMSAME_DEBUG_STALL"] = stall
            capfd.readouterr()
            with _env(e):
                got, _, info = gdev.align(ref, rst, q, qs, oracle.params(), 4)
            err = capfd.readouterr().err
            _rows_equal(got, exp, (name, side, stall))
            assert info["st"].launch_nwp == 0
            assert (line in err) == (side == "on"), (name, side, stall, err[-1500:])
            assert ("[stall] " in err) == (stall is not None), (name, side, stall, err[-1500:])
            nw.setdefault(side, info["st"].n_accepted)
            assert info["st"].n_accepted == nw["on"]


@pytest.mark.gpu
def test_mid_cli(oracle, tmp_path):
    """imsame -query -db -out on the 100 .. 320 mix: the .align bytes equal
    the oracle CLI's for -n_threads 1"""
    ref, rst, q, qs, _ = _workload(oracle, "big", 2000, "v454", 1)
    n = 400
    qs_n, q_n = qs[:n], q[:int(qs[n])]
    synth.write_fasta(tmp_path / "db.fa", ref, rst, "rec")
    synth.write_fasta(tmp_path / "q.fa", q_n, qs_n, "read")
    here = os.path.dirname(os.path.abspath(imsame_amd.__file__))
    cli = os.path.join(here, "bin", "imsame")
    args = ["-query", str(tmp_path / "q.fa"), "-db", str(tmp_path / "db.fa"), "-n_threads", "1"]
    r = subprocess.run([cli] + args + ["-out", str(tmp_path / "dev.align")], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0, r.stderr.decode()[-400:]
    o = Oracle.run_cli(args + ["-out", str(tmp_path / "ora.align")], timeout=120)
    assert o.returncode == 0, o.stderr.decode()[-400:]
    a, b = (tmp_path / "dev.align").read_bytes(), (tmp_path / "ora.align").read_bytes()
    assert len(b) > 10_000 and a == b
