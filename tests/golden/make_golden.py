#!/usr/bin/env python3
"""Generate the golden vectors under tests/golden/ from the REFERENCE itself.

The reference (Bitlab-UMA/IMSAME) ships no tests, fixtures or golden files
(SURVEY.md section 4), so every parity pin is produced here by running the
reference compiled from its own sources (oracle/Makefile `ref` target ->
oracle/_ref/{IMSAME,revComp,ref_driver}) on synthetic inputs.  Only this
container has /root/reference; the fixtures are committed and travel.

    python tests/golden/make_golden.py        # (re)writes the fixtures

Fixtures (data only -- inputs and the reference's outputs):
  nw_pairs.jsonl.gz   unit NW + backtracking + text (alignmentFunctions.c:210-560)
  ungapped.jsonl.gz   alignmentFromQuickHits outputs incl. the long double e-value
  e2e/<case>/         FASTA inputs + the reference's .align and [INFO] summary
                      for -n_threads 1 (file order) and 2/4/7 (record multisets)
  revcomp/<case>.*    revComp input / output pairs
and, drawn from RNG streams of their own after the ones above (which are
written first and stay byte for byte what they were):
  nw_pairs_mid_long.jsonl.gz   NW around the kernels' switch lengths (160/161,
                      320/321, 639-641, 1000, 2999-3000), low-complexity sides
  ungapped_long.jsonl.gz       walks over reads of 161-320 and 600-2500 bases
  e2e/{mid_reads,mid_mixed,long_reads,lowcomplex,dup_records,params_*}/
                      (db.fa, query.fa and expected.json gzipped: golden_io.e2e_case
                      hands out plain copies)

    python tests/golden/make_golden.py --only-new   # skips the older fixtures

A fixture whose content did not change is left untouched (a gzip member
carries its writing time).
"""
import functools
import gzip
import hashlib
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = os.path.join(REPO, "oracle", "_ref")
sys.path.insert(0, REPO)
from tests.synth import make_reference, make_reads  # noqa: E402
from tests.golden_io import record_multisets  # noqa: E402
from tests import golden_draws as D  # noqa: E402
from tests.golden_draws import rand_seq, mutate  # noqa: E402  (the draws every stream here was recorded with)

def write_gz(path, data):
    """data (bytes) gzipped to path, unless the file already holds them"""
    if os.path.exists(path):
        with gzip.open(path, "rb") as f:
            if f.read() == data:
                return
    with open(path, "wb") as f, gzip.GzipFile(filename="", mode="wb", fileobj=f, mtime=0) as g:
        g.write(data)


def write_plain(path, data):
    if os.path.exists(path) and open(path, "rb").read() == data:
        return
    with open(path, "wb") as f:
        f.write(data)


def build_ref():
    subprocess.run(["make", "-s", "-C", os.path.join(REPO, "oracle"), "ref"], check=True)


# ---------------------------------------------------------------- NW ------
def nw_cases(rng):
    cases = []
    # (xlen range, ylen range, kind, count)
    plan = [
        ((12, 40), (11, 40), "rand", 60),
        ((12, 40), (11, 40), "sim95", 60),
        ((40, 400), (20, 160), "rand", 40),
        ((40, 400), (20, 160), "sim70", 40),
        ((40, 400), (20, 160), "sub95", 40),
        ((1500, 2100), (100, 151), "embed", 30),   # C1/C2-like: read inside a record
        ((100, 160), (100, 160), "sim90", 30),     # C4-like: read vs read
        ((12, 20), (60, 200), "rand", 10),         # xlen < ylen
        ((2990, 3000), (140, 160), "embed", 4),
        ((2999, 3000), (2999, 3000), "sim90", 2),   # maximum sizes
        ((200, 400), (400, 800), "sim70", 6),
    ]
    gaps = [(-5, -2), (-5, -2), (-5, -2), (-1, -1), (-10, -3), (-2, -4), (0, 0), (-20, -1)]
    for (xr, yr, kind, cnt) in plan:
        for _ in range(cnt):
            xl = int(rng.integers(xr[0], xr[1] + 1))
            yl = int(rng.integers(yr[0], yr[1] + 1))
            ig, eg = gaps[int(rng.integers(0, len(gaps)))]
            x = rand_seq(rng, xl)
            if kind == "rand":
                y = rand_seq(rng, yl)
            elif kind == "embed":
                off = int(rng.integers(0, max(1, xl - yl)))
                y = mutate(rng, x[off:off + yl], 0.01, 0.005, 0.005)
                if len(y) < 11:
                    y = rand_seq(rng, yl)
            else:
                pct = int(kind[-2:]) / 100.0
                src = x[:yl] if len(x) >= yl else x + rand_seq(rng, yl - len(x))
                if kind.startswith("sub"):
                    y = mutate(rng, src, 1 - pct, 0, 0)
                else:
                    y = mutate(rng, src, (1 - pct) * 0.6, (1 - pct) * 0.2, (1 - pct) * 0.2)
                if len(y) < 11:
                    y = y + rand_seq(rng, 11)
            cases.append((ig, eg, x[:3000], y[:3000]))
    # hand-made corner cases
    cases += [
        (-5, -2, "A" * 12, "A" * 11),
        (-5, -2, "ACGTACGTACGT", "TTTTTTTTTTTT"),
        (-5, -2, "AAAAAAAAAAAAAAAAAAAAAAAA", "AAAAAAAAAAAA"),
        (-5, -2, "ACGT" * 30, "ACGT" * 10),
        (-5, -2, "ACGTTGCA" * 40, "TGCA" * 20),
        (-1, 0, "ACGTACGTAAAACCCCGGGGTTTT" * 4, "AAAACCCCGGGGTTTT" * 3),
        (3, 1, "ACGTACGTAAAACCCCGGGGTTTT" * 4, "AAAACCCCGGGGTTTT" * 3),  # positive gap scores
    ]
    return cases


def gen_nw(rng):
    cases = nw_cases(rng)
    p = subprocess.Popen([os.path.join(REF, "ref_driver")], stdin=subprocess.PIPE, stdout=subprocess.PIPE)
    inp = "".join(f"nw {ig} {eg} {x} {y}\n" for (ig, eg, x, y) in cases).encode()
    out, _ = p.communicate(inp)
    assert p.returncode == 0
    rows = []
    pos = 0
    for (ig, eg, x, y) in cases:
        nl = out.index(b"\n", pos)
        f = out[pos:nl].split()
        score, bx, by, length, ident, igaps, egaps, hx, hy, tl = [int(v) for v in f]
        text = out[nl + 1:nl + 1 + tl]
        pos = nl + 1 + tl + 1
        row = dict(igap=ig, egap=eg, X=x, Y=y, score=score, bx=bx, by=by, length=length,
                   identities=ident, igaps=igaps, egaps=egaps, head_x=hx, head_y=hy,
                   text_len=tl, text_sha1=hashlib.sha1(text).hexdigest())
        if tl <= 4000:
            row["text"] = text.decode()
        rows.append(row)
    write_gz(os.path.join(HERE, "nw_pairs.jsonl.gz"), "".join(json.dumps(r) + "\n" for r in rows).encode())
    print(f"nw_pairs: {len(rows)}")


# ---------------------------------------------------------- ungapped ------
def kmer_hits(db_recs, q_reads, max_hits):
    """(pos_db, pos_q, read, dbseq) for 12-mer seeds shared by query and DB
    (pos = last base + 1, as the reference's index, IMSAME.c:247)."""
    idx = {}
    off = 0
    for s, rec in enumerate(db_recs):
        for e in range(11, len(rec)):
            idx.setdefault(rec[e - 11:e + 1], []).append((off + e + 1, s))
        off += len(rec)
    qcat = "".join(q_reads)
    qstart = np.cumsum([0] + [len(r) for r in q_reads])
    hits = []
    for r in range(len(q_reads)):
        for p in range(max(11, qstart[r] - 1 + 11), qstart[r + 1]):
            for (pd, s) in idx.get(qcat[p - 11:p + 1], []):
                hits.append((pd, p + 1, r, s))
    return hits[:max_hits]


def gen_ungapped(rng):
    rows = []
    for case in range(6):
        L = [150, 400, 2000, 60, 900, 3000][case]
        nrec = [5, 4, 3, 20, 6, 2][case]
        recs = [rand_seq(rng, int(rng.integers(L // 2, L + 1))) for _ in range(nrec)]
        cat = "".join(recs)
        reads = []
        for k in range(12):
            rl = int(rng.integers(11, 160))
            if k % 3 == 2:
                reads.append(rand_seq(rng, rl))
            else:
                o = int(rng.integers(0, max(1, len(cat) - rl)))
                reads.append(mutate(rng, cat[o:o + rl], [0.0, 0.02, 0.1][k % 3], 0.0, 0.0) or "ACGTACGTACGT")
        hits = kmer_hits(recs, reads, 400)
        # also seeds in odd places: borrowed-base windows and record edges
        p = subprocess.Popen([os.path.join(REF, "ref_driver")], stdin=subprocess.PIPE, stdout=subprocess.PIPE)
        cmd = f"db {len(recs)} " + " ".join(recs) + "\n" + f"q {len(reads)} " + " ".join(reads) + "\n"
        cmd += "".join(f"ug {pd} {pq} {r} {s}\n" for (pd, pq, r, s) in hits)
        out, _ = p.communicate(cmd.encode())
        assert p.returncode == 0
        lines = out.decode().strip().split("\n") if hits else []
        for (pd, pq, r, s), ln in zip(hits, lines):
            xs, ys, tl, ehex, edec = ln.split()
            rows.append(dict(case=case, pos_db=pd, pos_q=pq, read=r, dbseq=s, x_start=int(xs),
                             y_start=int(ys), t_len=int(tl), e_hex=ehex, e_dec=edec))
        write_gz(os.path.join(HERE, f"ungapped_case{case}.json.gz"), json.dumps(dict(db=recs, reads=reads)).encode())
    write_gz(os.path.join(HERE, "ungapped.jsonl.gz"), "".join(json.dumps(r) + "\n" for r in rows).encode())
    print(f"ungapped: {len(rows)}")


# --------------------------------------------------------------- e2e ------
INFO_RE = re.compile(rb"^\[INFO\] (\d+ reads .*|The Jaccard-index is: .*)$", re.M)


def run_ref_imsame(q, d, out, T, extra=(), timeout=600):
    cmd = [os.path.join(REF, "IMSAME"), "-query", q, "-db", d, "-out", out, "-n_threads", str(T), *extra]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout)
    return p.returncode, p.stdout


def split_records(blob):
    """.align -> list of (header, body) using the fixed header shape."""
    parts = re.split(rb"(\(\d+, \d+\) : \d+% \d+% \d+\n \$\$\$\$\$\$\$ \n)", blob)
    return parts


def e2e_case(name, db_text, q_text, Ts=(1, 2, 4, 7), extra=(), packed=False, pin_inputs=False, timeout=600):
    """packed: the case's inputs and expected.json are stored gzipped
    (golden_io.e2e_case unpacks them); the reference runs on a plain copy.
    pin_inputs: a case that already has db.fa and query.fa runs the reference
    on those, and says so where the draw handed in differs (gen_e2e).
    timeout: seconds the reference has for each run; the longest run's wall
    time is returned as meta["ref_wall_s"] (not stored)."""
    d = os.path.join(HERE, "e2e", name)
    os.makedirs(d, exist_ok=True)
    dbp, qp = os.path.join(d, "db.fa"), os.path.join(d, "query.fa")
    if packed:
        write_gz(dbp + ".gz", db_text)
        write_gz(qp + ".gz", q_text)
        dbp, qp = os.path.join("/tmp", f"golden_{name}_db.fa"), os.path.join("/tmp", f"golden_{name}_query.fa")
        write_plain(dbp, db_text)
        write_plain(qp, q_text)
    elif pin_inputs and os.path.exists(dbp) and os.path.exists(qp):
        if open(dbp, "rb").read() != db_text or open(qp, "rb").read() != q_text:
            print(f"e2e {name}: committed inputs kept (a fresh draw differs)")
    else:
        write_plain(dbp, db_text)
        write_plain(qp, q_text)
    meta = dict(extra=list(extra), runs={})
    exp_path = os.path.join(d, "expected.json.gz" if packed else "expected.json")
    old_runs = json.load((gzip.open if packed else open)(exp_path)).get("runs", {}) if os.path.exists(exp_path) else {}
    wall = 0.0
    for T in Ts:
        outp = os.path.join("/tmp", f"golden_{name}_{T}.align")
        t0 = time.time()
        rc, so = run_ref_imsame(qp, dbp, outp, T, extra, timeout)
        wall = max(wall, time.time() - t0)
        blob = open(outp, "rb").read() if os.path.exists(outp) else b""
        heads = sorted(h.decode() for h in re.findall(rb"\(\d+, \d+\) : \d+% \d+% \d+\n", blob))
        run = dict(rc=rc, info=[m.decode() for m in INFO_RE.findall(so)],
                   err=[l.decode() for l in so.split(b"\n") if l.startswith(b"ERR")],
                   headers=heads, align_sha1=hashlib.sha1(blob).hexdigest(), align_len=len(blob))
        if T == 1:
            write_gz(os.path.join(d, "T1.align.gz"), blob)
        else:
            # bodies of different threads may interleave: keep the body multiset
            run["body_sha1s"] = record_multisets(blob)[1]
            # the order in which the threads' records reach the file differs from
            # run to run: a recorded run that differs in nothing else stands
            was = old_runs.get(str(T))
            if was and {**was, "align_sha1": run["align_sha1"]} == run:
                run = was
        meta["runs"][str(T)] = run
        os.remove(outp) if os.path.exists(outp) else None
    (write_gz if packed else write_plain)(exp_path, json.dumps(meta, indent=1).encode())
    if packed:
        os.remove(dbp), os.remove(qp)
    print(f"e2e {name}: " + ", ".join(f"T{T}:{len(meta['runs'][str(T)]['headers'])}" for T in Ts))
    return dict(meta, ref_wall_s=wall)


def fasta(recs, width=80, nl=b"\n", prefix="s"):
    out = []
    for i, r in enumerate(recs):
        out.append(f">{prefix}_{i}".encode() + nl)
        rb_ = r.encode() if isinstance(r, str) else r
        if width:
            for k in range(0, len(rb_), width):
                out.append(rb_[k:k + width] + nl)
        else:
            out.append(rb_ + nl)
    return b"".join(out)


def gen_e2e(rng):
    # These cases draw their reads with tests/synth.py, which has moved on since
    # they were recorded: drawn again, most of their query files would differ
    # and every such case would move.  The committed inputs are the fixture, so
    # the reference runs on those (a case that is not there yet is drawn).
    case = functools.partial(e2e_case, pin_inputs=True)
    # 1) canonical small synthetic (C1-like, scaled down): 100 kbp in 2 kbp records, 200 reads
    ref = make_reference(100_000, 2_000, seed=7)
    reads = make_reads(ref, 200, 150, seed=8)
    case("small_c2like", fasta(ref), fasta(reads, width=0, prefix="read"))
    # 2) 100 bp reads (C1 shape)
    reads = make_reads(ref, 150, 100, seed=9)
    case("small_c1like", fasta(ref), fasta(reads, width=0, prefix="read"))
    # 3) edge cases: N in DB and query, lowercase, multi-line, empty reads, short reads
    ref = make_reference(20_000, 1_000, seed=11)
    recs = [r for r in ref]
    recs[3] = recs[3][:400] + "NNNNN" + recs[3][400:]
    recs[5] = recs[5].lower()
    recs.insert(7, "")                               # empty DB record
    reads = make_reads(ref, 60, 120, seed=12)
    reads[3] = reads[3][:50] + "N" + reads[3][50:]   # N inside a read
    reads[4] = reads[4].lower()
    reads[10] = ""                                    # empty read (not a chunk head for T in 1,2,4,7)
    reads[11] = reads[11][:12]                       # length 12
    reads[12] = reads[12][:13]
    reads[13] = reads[13][:11]
    reads[-1] = reads[-1][:11]                       # last read of length 11
    case("edges", fasta(recs, width=60), fasta(reads, width=50, prefix="read"))
    # 4) borrowed-base case: 2 reads; read 1's first k-mer uses read 0's last base
    # (SURVEY Appendix A Q4): record 0 holds b+read1, record 1 holds b'+read1.
    # T=1: read 1's first k-mer borrows b -> only record 0 matches -> (1, 0).
    # T=2: read 1 is a chunk head -> its first k-mer hits both, LIFO -> (1, 1).
    r1 = rand_seq(rng, 90)
    b = "A"
    x0 = rand_seq(rng, 200) + b + r1 + rand_seq(rng, 200)
    x1 = rand_seq(rng, 200) + "C" + r1 + rand_seq(rng, 200)
    r0 = rand_seq(rng, 40) + b
    case("borrowed", fasta([x0, x1]), fasta([r0, r1], width=0, prefix="read"), Ts=(1, 2))
    # 5) CRLF database (k-mers reset at every '\r')
    ref = make_reference(8_000, 1_000, seed=13)
    reads = make_reads(ref, 30, 100, seed=14)
    case("crlf_db", fasta(ref, width=60, nl=b"\r\n"), fasta(reads, width=0, prefix="read"), Ts=(1, 2))
    # 6) non-default thresholds
    ref = make_reference(30_000, 1_500, seed=15)
    reads = make_reads(ref, 80, 150, seed=16, sub=0.05, ins=0.01, dele=0.01)
    case("params", fasta(ref), fasta(reads, width=0, prefix="read"), Ts=(1, 3),
             extra=("-evalue", "1e-10", "-coverage", "0.8", "-identity", "0.9", "-igap", "3", "-egap", "1"))
    # 7) records of exactly 2999/3000 bp and a 3001 bp record (fatal in the reference)
    x3000 = rand_seq(rng, 3000)
    x2999 = rand_seq(rng, 2999)
    reads = [mutate(rng, x3000[500:650], 0.01, 0, 0), mutate(rng, x2999[100:250], 0.01, 0, 0)]
    case("maxlen", fasta([x3000, x2999]), fasta(reads, width=0, prefix="read"), Ts=(1,))
    x3001 = rand_seq(rng, 3001)
    reads = [mutate(rng, x2999[10:160], 0.01, 0, 0), mutate(rng, x3001[10:160], 0.01, 0, 0),
             mutate(rng, x2999[300:450], 0.01, 0, 0)]
    case("toolong", fasta([x2999, x3001]), fasta(reads, width=0, prefix="read"), Ts=(1,))
    # 8) reads vs reads (C4 shape): both sides 150 bp
    ref = make_reference(50_000, 5_000, seed=17)
    a = make_reads(ref, 120, 150, seed=18)
    b = make_reads(ref, 120, 150, seed=19)
    case("reads_vs_reads", fasta(b, width=0, prefix="m2"), fasta(a, width=0, prefix="m1"))
    # 9) an empty query read placed at a chunk head for T=2 (ref UB: only T=1 recorded)
    ref = make_reference(10_000, 1_000, seed=20)
    reads = make_reads(ref, 10, 100, seed=21)
    reads[5] = ""
    case("empty_not_head", fasta(ref), fasta(reads, width=0, prefix="read"), Ts=(1, 3))


# ------------------------------------------------------------ revcomp ------
def gen_revcomp(rng):
    d = os.path.join(HERE, "revcomp")
    os.makedirs(d, exist_ok=True)
    cases = {
        "basic": b">r1 desc\nACGTNacgtu\nRY*-\r\nAC\n>r2\nGGGG\n>r3\n\n>r4\nUuTt\n",
        "crlf": b">a\r\nACGTT\r\nGG\r\n>b\r\nTTTT\r\n",
        "pre_text": b"junk before\n>x\nAC\n",
        "no_trailing_nl": b">x\nACGTA\n>y\nCCGT",
        "gt_in_header": b">x a>b\nACGT\n>y\nTT\n",
        "empty_header_only": b">only_header",
    }
    big = fasta(make_reference(30_000, 700, seed=22), width=61)
    cases["synthetic"] = big
    for name, data in cases.items():
        inp = os.path.join(d, name + ".in")
        outp = os.path.join(d, name + ".out")
        with open(inp, "wb") as f:
            f.write(data)
        subprocess.run([os.path.join(REF, "revComp"), inp, outp], check=True, stdout=subprocess.DEVNULL)
    print(f"revcomp: {len(cases)}")


# ------------------------------------------------- mid and long reads ------
def gen_nw_mid_long(rng):
    cases = D.nw_mid_long_cases(rng)
    rows = D.ref_nw(cases)
    lines = []
    for r, c in zip(rows, cases):
        text = r.pop("_text")
        r["kind"] = c[4]
        if r["text_len"] <= 4000:
            r["text"] = text.decode()
        lines.append(json.dumps(r) + "\n")
    write_gz(os.path.join(HERE, "nw_pairs_mid_long.jsonl.gz"), "".join(lines).encode())
    ylen = [len(r["Y"]) for r in rows]
    mid = sum(160 < y <= 320 for y in ylen)
    lowcx = sum(r["kind"].startswith("lowcx") for r in rows)
    assert mid >= 120 and lowcx >= 60
    print(f"nw_pairs_mid_long: {len(rows)} rows, reads <= 160: {sum(y <= 160 for y in ylen)}, "
          f"161-320: {mid}, > 320: {sum(y > 320 for y in ylen)}, low-complexity side: {lowcx}, "
          f"positive gap term: {sum(r['igap'] > 0 or r['egap'] > 0 for r in rows)}")


def gen_ungapped_long(rng, per_case=300):
    """Walks far longer than a short read: reads of 161-320 and 600-2500
    bases drawn from records of up to 3000 at 0, 1, 5 and 12 % divergence
    with indels (the diagonal is lost mid-walk), seeds at the buffers' first
    bases, at record and read ends and deep inside; case 3: a periodic
    database (many off-diagonal hits)."""
    rows, kinds = [], {"start": 0, "end": 0, "deep": 0, "other": 0}
    for case in range(5):
        if case == 3:
            u37, u5 = rand_seq(rng, 37), rand_seq(rng, 5)
            recs = [mutate(rng, u37 * 70, 0.03, 0, 0)[:2500], (u5 * 200)[:1000],
                    "".join("AG"[i] for i in rng.integers(0, 2, 1500)), rand_seq(rng, 2000)]
        else:
            recs = [rand_seq(rng, int(rng.integers(lo, 3001))) for lo in ([2600, 1500, 700, 2999, 400, 2000][:3 + case])]
        cat = "".join(recs)
        dend = np.cumsum([len(r) for r in recs])
        reads = []
        for k in range(8):
            L = int(rng.integers(600, 2501)) if k % 2 else int(rng.integers(161, 321))
            div = [0.0, 0.01, 0.05, 0.12][(k // 2) % 4]
            if k == 0:
                o = 0                                   # seeds in the first bases of both buffers
            elif k == 1:
                o = int(dend[1]) - L                    # the read ends where record 1 ends
            else:
                o = int(rng.integers(0, len(cat) - L))
            o = max(o, 0)
            reads.append(mutate(rng, cat[o:o + L], div * 0.6, div * 0.2, div * 0.2))
        hits = kmer_hits(recs, reads, 10 ** 9)
        qend = np.cumsum([len(r) for r in reads])
        groups = {"start": [], "end": [], "deep": [], "other": []}
        for i, (pd, pq, r, s) in enumerate(hits):
            qoff, qrem = pq - 12 - (int(qend[r]) - len(reads[r])), int(qend[r]) - pq
            doff, drem = pd - 12 - (int(dend[s]) - len(recs[s])), int(dend[s]) - pd
            if pq - 12 < 15 or pd - 12 < 15:
                groups["start"].append(i)
            elif qrem < 15 or drem < 15:
                groups["end"].append(i)
            elif min(qoff, qrem, doff, drem) > 64:      # more than 3 chunks of 16 on every side
                groups["deep"].append(i)
            else:
                groups["other"].append(i)
        keep = []
        for g, cap in (("start", 50), ("end", 70), ("deep", 130), ("other", 50)):
            idx = groups[g]
            if len(idx) > cap:
                idx = [idx[j] for j in sorted(rng.choice(len(idx), cap, replace=False))]
            kinds[g] += len(idx)
            keep += idx
        hits = [hits[i] for i in sorted(keep)][:per_case]
        cmd = f"db {len(recs)} " + " ".join(recs) + "\n" + f"q {len(reads)} " + " ".join(reads) + "\n"
        cmd += "".join(f"ug {pd} {pq} {r} {s}\n" for (pd, pq, r, s) in hits)
        p = subprocess.run([os.path.join(REF, "ref_driver")], input=cmd.encode(), stdout=subprocess.PIPE)
        assert p.returncode == 0
        lines = p.stdout.decode().strip().split("\n")
        assert len(lines) == len(hits)
        for (pd, pq, r, s), ln in zip(hits, lines):
            xs, ys, tl, ehex, edec = ln.split()
            rows.append(dict(case=case, pos_db=pd, pos_q=pq, read=r, dbseq=s, x_start=int(xs),
                             y_start=int(ys), t_len=int(tl), e_hex=ehex, e_dec=edec))
        write_gz(os.path.join(HERE, f"ungapped_long_case{case}.json.gz"), json.dumps(dict(db=recs, reads=reads)).encode())
    write_gz(os.path.join(HERE, "ungapped_long.jsonl.gz"), "".join(json.dumps(r) + "\n" for r in rows).encode())
    tl = np.array([r["t_len"] for r in rows])
    assert len(rows) <= 1500 and min(kinds.values()) > 0
    print(f"ungapped_long: {len(rows)} rows {kinds}, walks > 64 bases: {int((tl > 64).sum())}, "
          f"> 320: {int((tl > 320).sum())}, longest {int(tl.max())}")


def e2e_checked(name, recs, reads, Ts, extra=(), share=(0.10, 0.90), max_wall_s=60):
    """e2e_case on records and reads without an empty read (at a chunk head
    one is undefined behaviour in the reference): every run returns 0 and
    accepts a share of the reads inside `share` (None: at least one read
    accepted and one rejected), within max_wall_s seconds per run of the
    reference."""
    assert all(len(r) > 0 for r in reads)
    assert sum(len(r) for r in recs) <= 60_000 and len(reads) <= 120
    meta = e2e_case(name, fasta(recs), fasta(reads, width=0, prefix="read"), Ts=Ts, extra=extra, packed=True,
                    timeout=max_wall_s)
    for T in Ts:
        run = meta["runs"][str(T)]
        assert run["rc"] == 0, (name, T, run["rc"])
        acc = len(run["headers"])
        if share is None:
            assert 0 < acc < len(reads), (name, T, acc)
        else:
            assert share[0] * len(reads) <= acc <= share[1] * len(reads), (name, T, acc, len(reads))
    print(f"    {name}: {len(recs)} records, {sum(len(r) for r in recs)} bp, {len(reads)} reads of "
          f"{min(map(len, reads))}-{max(map(len, reads))} bases, accepted at T=1: {len(meta['runs']['1']['headers'])}, "
          f"the reference's longest run {meta['ref_wall_s']:.2f} s")


def gen_e2e_mid_long(rng):
    # reads of 161-320 bases against 2 kbp records, make_reads' default error rates
    ref = make_reference(24_000, 2_000, seed=101)
    reads = []
    for L in (161, 200, 250, 300, 319, 320):
        reads += make_reads(ref, 10, L, seed=110 + L, frac_true=0.7)
    e2e_checked("mid_reads", ref, reads, (1, 2, 7))
    # short, mid and multi-strip reads in one query
    recs, reads = D.draw_mid_mixed(rng)
    e2e_checked("mid_mixed", recs, reads, (1, 3, 4))
    # reads of 600-2500 bases against 3000-base records
    ref = make_reference(30_000, 3_000, seed=103)
    reads = D.reads_from(rng, ref, rng.integers(600, 2501, 14), 0.7, 0.01, 0.0005, 0.0005)
    e2e_checked("long_reads", ref, reads, (1, 2, 7))
    # low complexity: about half the records periodic or two-letter, reads cut from them
    recs = []
    for k in range(16):
        L = int(rng.integers(500, 1500))
        recs.append(D.low_complexity(rng, L) if k % 2 else rand_seq(rng, L))
    reads = D.reads_from(rng, recs, rng.integers(60, 280, 60), 0.7, 0.01, 0.002, 0.002)
    e2e_checked("lowcomplex", recs, reads, (1, 2, 4), max_wall_s=20)      # (the reference is slow on such databases)
    # records that share mutated prefixes: the visiting order decides
    recs, reads = D.draw_dup_records(rng)
    e2e_checked("dup_records", recs, reads, (1, 3, 7))
    # non-default thresholds and gap costs, reads of 100-320 bases with indels
    for name, extra, share in (
            ("params_strict", ("-coverage", "1", "-identity", "0.5", "-evalue", "10"), None),
            ("params_loose", ("-coverage", "0.01", "-identity", "0.01"), None),
            ("params_gaps", ("-igap", "40", "-egap", "2", "-identity", "0.75", "-coverage", "0.3333"), (0.10, 0.90))):
        ref = make_reference(20_000, 1_000, seed=int(rng.integers(1 << 30)))
        reads = D.reads_from(rng, ref, rng.integers(100, 321, 48), 0.75, 0.03, 0.01, 0.01)
        e2e_checked(name, ref, reads, (1, 3, 7), extra=extra, share=share)


def main():
    build_ref()
    if "--only-new" not in sys.argv[1:]:
        rng = np.random.default_rng(20261015)
        gen_nw(rng)
        gen_ungapped(rng)
        gen_e2e(rng)
        gen_revcomp(rng)
    # (streams of their own: the fixtures above do not move when these change)
    gen_nw_mid_long(np.random.default_rng(2026102101))
    gen_ungapped_long(np.random.default_rng(2026102102))
    gen_e2e_mid_long(np.random.default_rng(2026102103))


if __name__ == "__main__":
    main()
