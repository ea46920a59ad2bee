"""Input draws for the mid- and long-read golden vectors.

tests/golden/make_golden.py records the reference's outputs on these draws
(nw_pairs_mid_long, the mid_mixed and dup_records e2e cases); the live
differential in tests/test_oracle.py draws fresh ones from the same functions
with another seed wherever the compiled reference is at hand.  Every function
takes its own numpy Generator: nothing here touches the stream that feeds the
older fixtures.
"""
import hashlib
import os
import subprocess

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.join(REPO, "oracle", "_ref")

ACGT = "ACGT"
NW_FIELDS = ("score", "bx", "by", "length", "identities", "igaps", "egaps", "head_x", "head_y")

# the gap pairs the NW tests use, and two with a positive term
NW_GAPS = [(-5, -2), (0, 0), (-1, 0), (-1, -1), (-7, -1), (-10, -3), (-2, -4), (-40, -2), (-20, -1), (3, 1), (1, -1)]
NW_KINDS = ("rand", "embed", "lowcx", "lowcx_cut")


def rand_seq(rng, n):
    return "".join(ACGT[i] for i in rng.integers(0, 4, n))


def mutate(rng, s, sub, ins, dele):
    out = []
    for c in s:
        r = rng.random()
        if r < dele:
            continue
        if r < dele + ins:
            out.append(ACGT[rng.integers(0, 4)])
        if rng.random() < sub:
            c = ACGT.replace(c, "")[rng.integers(0, 3)]
        out.append(c)
    return "".join(out)


def low_complexity(rng, n):
    """n bases of one of: a homopolymer, a repeat of period 1-8, a two-letter
    alphabet, a repeat of period 13-60 with ~3 % point changes."""
    kind = int(rng.integers(0, 4))
    if kind == 0:
        return ACGT[rng.integers(0, 4)] * n
    if kind == 1:
        unit = rand_seq(rng, int(rng.integers(1, 9)))
        return (unit * (n // len(unit) + 1))[:n]
    if kind == 2:
        a, b = rng.choice(4, 2, replace=False)
        return "".join((ACGT[a], ACGT[b])[i] for i in rng.integers(0, 2, n))
    unit = rand_seq(rng, int(rng.integers(13, 61)))
    return mutate(rng, (unit * (n // len(unit) + 2)), 0.03, 0.0, 0.0)[:n]


def _fit(rng, s, n, filler):
    """s cut or extended (by filler(rng, k)) to n bases"""
    return s[:n] if len(s) >= n else s + filler(rng, n - len(s))


def nw_pair(rng, kind, xl, yl):
    """One (record X of xl bases, read Y of yl bases) of the given kind."""
    div = float(rng.choice([0.01, 0.05, 0.15]))
    if kind == "rand":
        return rand_seq(rng, xl), rand_seq(rng, yl)
    if kind == "embed":                 # the read inside the record (or the record inside the read), with edits
        if xl >= yl:
            x = rand_seq(rng, xl)
            o = int(rng.integers(0, xl - yl + 1))
            y = _fit(rng, mutate(rng, x[o:o + yl], div * 0.6, div * 0.2, div * 0.2), yl, rand_seq)
        else:
            y = rand_seq(rng, yl)
            o = int(rng.integers(0, yl - xl + 1))
            x = _fit(rng, mutate(rng, y[o:o + xl], div * 0.6, div * 0.2, div * 0.2), xl, rand_seq)
        return x, y
    if kind == "lowcx":                 # low complexity on both sides, drawn apart
        return low_complexity(rng, xl), low_complexity(rng, yl)
    assert kind == "lowcx_cut"          # a low-complexity record and a read cut from it
    src = low_complexity(rng, max(xl, yl) + 64)
    ox, oy = int(rng.integers(0, len(src) - xl + 1)), int(rng.integers(0, len(src) - yl + 1))
    y = src[oy:oy + yl]
    if rng.random() < 0.5:
        y = _fit(rng, mutate(rng, y, 0.02, 0.005, 0.005), yl, low_complexity)
    return src[ox:ox + xl], y


def nw_mid_long_cases(rng, n_mid=132, n_160=36, n_321=30, n_strip=60, n_1000=12, n_max=10, ycap=3000):
    """(igap, egap, X, Y, kind) rows around the NW kernels' switch lengths (one
    strip of the packed kernel: 160; its mid form: 320; a strip of the
    long-read kernels: 640).
    Records: 12 bases, shorter than the read, as long as it, 700, 2000, 3000.
    ycap bounds the reads (the live differential draws smaller sets)."""
    ylens = []
    for k in range(n_mid):
        ylens.append((161, 319, 320, int(rng.integers(162, 319)))[k % 4])
    ylens += [160] * n_160 + [321] * n_321
    ylens += [(639, 640, 641)[k % 3] for k in range(n_strip)]
    ylens += [1000] * n_1000 + [(2999, 3000)[k % 2] for k in range(n_max)]
    ylens = [min(y, ycap) for y in ylens]
    cases = []
    for k, yl in enumerate(ylens):
        kind = NW_KINDS[k % 4]
        xl = (12, int(rng.integers(13, yl)), yl, 700, 2000, 3000)[int(rng.integers(0, 6))]
        ig, eg = NW_GAPS[int(rng.integers(0, len(NW_GAPS)))]
        x, y = nw_pair(rng, kind, xl, yl)
        assert len(x) == xl and len(y) == yl
        cases.append((ig, eg, x, y, kind))
    # ties at their densest: homopolymers and short periods at the switch lengths
    for yl in (161, 320, 321, 640):
        cases.append((-5, -2, "A" * 700, "A" * yl, "lowcx"))
        cases.append((-5, -2, "AC" * 350, "CA" * (yl // 2) + "C" * (yl % 2), "lowcx"))
        cases.append((0, 0, "ACG" * 110, ("GCA" * 220)[:yl], "lowcx"))
    return cases


def ref_nw(cases, timeout=None):
    """The compiled reference's NW, traceback and text for (igap, egap, X, Y, ...)
    rows (oracle/ref_driver.c): one dict per row, the text as bytes."""
    inp = "".join(f"nw {c[0]} {c[1]} {c[2]} {c[3]}\n" for c in cases).encode()
    p = subprocess.run([os.path.join(REF, "ref_driver")], input=inp, stdout=subprocess.PIPE, timeout=timeout)
    assert p.returncode == 0, p.returncode
    out, pos, rows = p.stdout, 0, []
    for c in cases:
        nl = out.index(b"\n", pos)
        f = [int(v) for v in out[pos:nl].split()]
        tl = f[9]
        text = out[nl + 1:nl + 1 + tl]
        pos = nl + 1 + tl + 1
        row = dict(igap=c[0], egap=c[1], X=c[2], Y=c[3], **dict(zip(NW_FIELDS, f[:9])),
                   text_len=tl, text_sha1=hashlib.sha1(text).hexdigest())
        row["_text"] = text
        rows.append(row)
    return rows


# ------------------------------------------------------------------- e2e ---
def reads_from(rng, recs, lens, frac_true, sub, ins, dele):
    """One read per entry of lens: frac_true of them a window of one record
    (over its end where the record is shorter) with the given edits, the rest
    random."""
    reads = []
    for L in lens:
        L = int(L)
        if rng.random() < frac_true:
            rec = recs[int(rng.integers(0, len(recs)))]
            o = int(rng.integers(0, max(1, len(rec) - L + 1)))
            y = _fit(rng, mutate(rng, rec[o:o + L + 8], sub, ins, dele), L, rand_seq)
        else:
            y = rand_seq(rng, L)
        reads.append(y)
    return reads


MIXED_YLENS = (12, 100, 150, 160, 161, 250, 320, 321, 500)


def draw_mid_mixed(rng, n_reads=72, db_bp=24_000):
    """Short, mid and multi-strip reads in one query against records of mixed
    lengths, some shorter than the reads.  -> (records, reads)"""
    recs, total = [], 0
    while total < db_bp:
        L = int(rng.choice([90, 200, 400, 1000, 2000, 3000]))
        recs.append(rand_seq(rng, L))
        total += L
    lens = [MIXED_YLENS[k % len(MIXED_YLENS)] for k in range(n_reads)]
    lens = [lens[i] for i in rng.permutation(n_reads)]
    return recs, reads_from(rng, recs, lens, 0.65, 0.02, 0.004, 0.004)


def draw_dup_records(rng, n_fam=6, n_reads=60):
    """Families of records that share a mutated prefix of 50-600 bases, among
    unrelated ones: a read drawn from a prefix has candidates in several
    records, and the visiting order decides which one is reported.
    -> (records, reads)"""
    recs, prefixes = [], []
    for _ in range(n_fam):
        pre = rand_seq(rng, int(rng.integers(50, 601)))
        prefixes.append(pre)
        for _ in range(int(rng.integers(2, 5))):
            div = float(rng.choice([0.0, 0.01, 0.04]))
            recs.append(mutate(rng, pre, div, div / 4, div / 4) + rand_seq(rng, int(rng.integers(100, 1200))))
        recs.append(rand_seq(rng, int(rng.integers(300, 2000))))
    recs = [recs[i] for i in rng.permutation(len(recs))]
    reads = []
    for k in range(n_reads):
        r = rng.random()
        if r < 0.55:                    # from a shared prefix
            pre = prefixes[int(rng.integers(0, n_fam))]
            L = int(rng.integers(40, min(len(pre), 320) + 1))
            o = int(rng.integers(0, len(pre) - L + 1))
            reads.append(mutate(rng, pre[o:o + L], 0.01, 0.002, 0.002) or pre[:40])
        elif r < 0.7:                   # from anywhere in a record
            reads += reads_from(rng, recs, [int(rng.integers(60, 321))], 1.0, 0.01, 0.002, 0.002)
        else:
            reads.append(rand_seq(rng, int(rng.integers(40, 321))))
    return recs, reads
