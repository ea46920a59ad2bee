"""Order between a lane's two streams, tested adversarially (GPU).

imsame_dev.hip:align_one runs two read sets on two streams (and, with
independent pipelines, two host threads) that share cperm / crow, the
candidate regions, the active lists and the counters ("Hazards
between a lane's streams").  IMSAME_DEBUG_STALL puts a delay kernel ahead of
every launch of one side, so "A runs late" and "B runs late" are conditions
these tests set: every variant runs un-stalled, with A stalled and with B
stalled, and every run must give the rows, the NW count and the path text of
the joined, un-stalled rounds (IMSAME_PIPES=0), which equal the oracle on
three windows.  One variant runs with an identity bound that rejects most true
reads' first candidates, so that the first pipeline's later rounds are busy
too (its own joined baseline, checked against the oracle on 24 reads).

Shape: 8 Mbp database (the smallest at which random reads give weak
candidates), 32k reads of 150 bp, 40 % of them random.

Stall length.  The longest single launch of the un-stalled runs at this shape
(stats.launch_ms over every variant) measured 4.785 ms on an MI355X
(MEASURED_LAUNCH_MS; a call's seed scans take 0.9-1.1 ms together); the stall
is 4 x that, rounded up to 0.5 ms: 19.5 ms (STALL_US, below the knob's clamp
of 20 ms), so the stalled side stays behind the other side's whole next
launch and its host sync.  The fixture prints the run's own figure.
"""
import contextlib
import os
import re

import numpy as np
import pytest

from imsame_amd import Device, render, PARITY_FIELDS
from tests import synth

pytestmark = pytest.mark.gpu

MEASURED_LAUNCH_MS = 4.785     # longest NW launch, un-stalled (see the module docstring)
STALL_US = 19_500              # ceil(4 x MEASURED_LAUNCH_MS / 0.5 ms) x 0.5 ms

N_READS = 32_000
KNOBS = ("IMSAME_PIPES", "IMSAME_CUT_WEAK", "IMSAME_PRIO_B", "IMSAME_SPEC", "IMSAME_SPEC_WEAK", "IMSAME_SPLIT_MIN",
         "IMSAME_SPLIT_SEQ", "IMSAME_SPLIT_ROUNDS", "IMSAME_LANES", "IMSAME_LANE_MIN", "IMSAME_NW_WEAK_ROWS",
         "IMSAME_NW_R1B_ROWS", "IMSAME_DEBUG_STALL", "IMSAME_DEBUG_ROUNDS")


@contextlib.contextmanager
def _env(env):
    old = {k: os.environ.get(k) for k in KNOBS}
    for k in KNOBS:
        os.environ.pop(k, None)
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


class Shape:
    pass


@pytest.fixture(scope="module")
def shape(oracle):
    """The database indexed once, the query set once, the joined un-stalled
    baseline and its three oracle windows."""
    s = Shape()
    s.ref, s.rst = synth.make_reference_arr(8_000_000, 2_000, seed=191)
    s.q, s.qs = synth.make_reads_arr(s.ref, N_READS, 150, seed=192, frac_true=0.6, ins=0.002, dele=0.002)
    s.dev = Device(0)
    s.dev.index(s.ref, s.rst)
    s.dev.set_query(s.q, s.qs)
    wins = [(0, 500), (N_READS // 2 - 250, N_READS // 2 + 250), (N_READS - 500, N_READS)]
    s.baseline = {}
    for strict in (False, True):
        pkw = STRICT if strict else {}
        with _env({"IMSAME_PIPES": "0"}):
            base, pb, sb = s.dev.align(n_threads=16, want_paths=True, params=s.dev.params(**pkw))
        # (a rejected true read scans on through every hit: ~75 ms per read in the oracle)
        w = [(N_READS // 2 - 12, N_READS // 2 + 12)] if strict else wins
        rc, exp, _ = oracle.align_windows(s.ref, s.rst, s.q, s.qs, w, oracle.params(**pkw), 16)
        assert rc == 0
        for (a, b), e in zip(w, exp):
            assert not _cmp(base[a:b], e), (strict, (a, b), _cmp(base[a:b], e))
        acc = np.flatnonzero(base["status"] == 1)
        assert len(acc) > (2_000 if strict else N_READS // 2), len(acc)
        s.baseline[strict] = (base, sb, {int(k): _text(s, base, pb, k) for k in acc[::173]})
    s.longest = 0.0
    yield s
    print(f"\n[streams] longest un-stalled NW launch {s.longest:.3f} ms -> stall "
          f"{np.ceil(4 * s.longest / 0.5) * 0.5:.1f} ms (STALL_US = {STALL_US})")
    s.dev.close()


def _cmp(r, ref):
    bad = []
    for f in PARITY_FIELDS:
        idx = np.flatnonzero(r[f] != ref[f])
        bad += [(int(i), f, int(r[f][i]), int(ref[f][i])) for i in idx[:5]]
    return bad


def _text(s, res, paths, k):
    r = res[k]
    x0 = int(s.rst[int(r["db_seq"])])
    X = s.ref[x0:x0 + 2_000].tobytes()
    Y = s.q[int(s.qs[k]):int(s.qs[k]) + int(r["ylen"])].tobytes()
    return render(X, Y, r, paths[r["path_off"]:r["path_off"] + r["path_len"]])[0]


# how a variant proves that its path ran, from the IMSAME_DEBUG_ROUNDS lines
def _proof_pipes(err):
    m = re.findall(r"\[round 1 pipes\] cand=(\d+) unpredicted=(\d+) paused=(\d+)", err)
    assert m, err[-1500:]
    for cand, unp, paused in m:
        assert int(unp) > 0 and int(cand) > int(unp) and int(paused) > 0, m
    assert re.search(r"\[round \d+ pipe A\]", err) and re.search(r"\[round \d+ pipe B\]", err), err[-1500:]


def _proof_pipes_busy_a(err):               # ... and A's round 2 holds thousands of reads
    _proof_pipes(err)
    m = re.search(r"\[round 2 pipe A\] active=(\d+) .* cand=(\d+) ", err)
    assert m and int(m.group(1)) > 5_000 and int(m.group(2)) > 5_000, err[-1500:]


def _proof_pipes_uncut(err):                # IMSAME_CUT_WEAK=0: one round-1 launch on A, nothing unpredicted
    m = re.findall(r"\[round 1 pipes\] cand=(\d+) unpredicted=(\d+) paused=(\d+)", err)
    assert m and all(int(c) > 0 and int(u) == 0 and int(p) > 0 for c, u, p in m), err[-1500:]
    assert re.search(r"\[round \d+ pipe A\]", err) and re.search(r"\[round \d+ pipe B\]", err), err[-1500:]


def _proof_prio_b(err):
    _proof_pipes(err)
    assert "[prio_b] " in err, err[-1500:]


def _proof_split(err):
    assert " split] " in err, err[-1500:]


def _proof_r1b(err):
    m = re.findall(r"\[round 1b\] paused=(\d+) .*? cand=(\d+)\+(\d+) ", err)
    assert m and all(int(p) > 0 and int(a) > 0 and int(b) > 0 for p, a, b in m), err[-1500:]
    assert " split] " not in err and " pipes] " not in err


def _proof_lanes(err):
    _proof_pipes(err)
    assert len(re.findall(r"\[round 1 pipes\]", err)) == 3, err[-1500:]


PIPES = {"IMSAME_PIPES": "1"}
# an identity bound only error-free reads pass: most true reads' round-1
# candidates (predicted, pipeline A) are rejected, so A's later rounds are as
# busy as B's and rewrite the lists and the order B's weak launch still reads
STRICT = {"min_identity": 0.995}
VARIANTS = [
    # 1. independent pipelines
    ("pipes", PIPES, _proof_pipes, True),
    ("pipes_uncut", {**PIPES, "IMSAME_CUT_WEAK": "0"}, _proof_pipes_uncut, True),
    ("pipes_prio_b", {**PIPES, "IMSAME_PRIO_B": "1"}, _proof_prio_b, True),
    ("pipes_spec", {**PIPES, "IMSAME_SPEC": "2", "IMSAME_SPEC_WEAK": "8"}, _proof_pipes, False),
    ("pipes_strict", {**PIPES, "strict": "1"}, _proof_pipes_busy_a, True),
    # 2. split rounds (joined rounds)
    ("split", {"IMSAME_PIPES": "0", "IMSAME_SPLIT_MIN": "1024"}, _proof_split, True),
    ("split_at_once", {"IMSAME_PIPES": "0", "IMSAME_SPLIT_MIN": "1024", "IMSAME_SPLIT_SEQ": "0"}, _proof_split, True),
    # 3. round 1b alone
    ("round1b", {"IMSAME_PIPES": "0", "IMSAME_SPLIT_ROUNDS": "0"}, _proof_r1b, True),
    # 4. three lanes, each with its two pipelines
    ("lanes3", {**PIPES, "IMSAME_LANES": "3", "IMSAME_LANE_MIN": "1000"}, _proof_lanes, True),
    # 5. weak hits predicting rows: a weak read's candidates stay on one side of round 1's cut
    ("weak_rows", {**PIPES, "IMSAME_NW_WEAK_ROWS": "1"}, _proof_pipes, True),
    ("weak_r1b_rows", {**PIPES, "IMSAME_NW_WEAK_ROWS": "1", "IMSAME_NW_R1B_ROWS": "1"}, _proof_pipes, True),
]


@pytest.mark.parametrize("stalled", ["none", "A", "B"])
@pytest.mark.parametrize("name,env,proof,same_nw", VARIANTS, ids=[v[0] for v in VARIANTS])
def test_stream_order_under_stalls(shape, capfd, name, env, proof, same_nw, stalled):
    """One variant of align_one's two-stream forms, un-stalled or with every
    launch of one side delayed by STALL_US: every PARITY_FIELDS field of every
    row, the NW count (default speculation widths) and the text of every
    173rd accepted read equal the joined un-stalled baseline; the debug lines
    prove that the variant's path ran and, when stalled, that the stalls were
    enqueued on that side only.  (STALL_US: 19.5 ms = 4 x the longest
    un-stalled launch at this shape, 4.785 ms measured, rounded up to 0.5 ms.)"""
    s = shape
    e = dict(env, IMSAME_DEBUG_ROUNDS="1")
    strict = e.pop("strict", None) is not None
    base, sb, text = s.baseline[strict]
    if stalled != "none":
        e["IMSAME_DEBUG_STALL"] = f"{stalled}:{STALL_US}"
    capfd.readouterr()
    with _env(e):
        r, pp, st = s.dev.align(n_threads=16, want_paths=True, params=s.dev.params(**(STRICT if strict else {})))
    err = capfd.readouterr().err
    if stalled == "none":
        s.longest = max([s.longest] + [float(st.launch_ms[k]) for k in range(min(int(st.nw_launches), len(st.launch_ms)))])
        with capfd.disabled():
            print(f"\n[streams] {name}: {int(st.nw_launches)} NW launches, longest so far {s.longest:.3f} ms, "
                  f"seed scans {st.ms_seed:.3f} ms in all")
    assert not _cmp(r, base), (name, stalled, _cmp(r, base))
    if same_nw:
        assert st.n_nw == sb.n_nw, (name, stalled, st.n_nw, sb.n_nw)
    for k, t0 in text.items():
        assert _text(s, r, pp, k) == t0, (name, stalled, k)
    proof(err)
    m = re.findall(r"\[stall\] A=(\d+) B=(\d+)", err)
    if stalled == "none":
        assert not m, m
    else:
        assert m, err[-1500:]
        na, nb = sum(int(a) for a, _ in m), sum(int(b) for _, b in m)
        assert (na > 0 and nb == 0) if stalled == "A" else (nb > 0 and na == 0), (name, stalled, m)
