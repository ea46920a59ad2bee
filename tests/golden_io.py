"""Readers for the committed golden vectors (tests/golden/, made by
tests/golden/make_golden.py from the compiled reference)."""
import gzip
import hashlib
import json
import os
import re

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
HEADER_RE = re.compile(rb"(\(\d+, \d+\) : \d+% \d+% \d+\n \$\$\$\$\$\$\$ \n)")
INFO_RE = re.compile(rb"^\[INFO\] (\d+ reads .*|The Jaccard-index is: .*)$", re.M)


def nw_pairs(stem="nw_pairs"):
    with gzip.open(os.path.join(GOLDEN, stem + ".jsonl.gz"), "rt") as f:
        return [json.loads(l) for l in f]


def nw_pairs_mid_long():
    """NW rows around the kernels' switch lengths (reads of 160 .. 3000
    columns), low-complexity sides and positive gap terms included; the
    schema of nw_pairs() plus the row's `kind`."""
    return nw_pairs("nw_pairs_mid_long")


NW_FIELDS = ("score", "bx", "by", "length", "identities", "igaps", "egaps", "head_x", "head_y")
NW_CLASSES = ("short", "mid", "long")       # reads of <= 160, 161 .. 320 and more columns: one launch each
# the e2e cases at mid and long reads
MID_LONG_E2E = ["mid_reads", "mid_mixed", "long_reads", "lowcomplex", "dup_records",
                "params_strict", "params_loose", "params_gaps"]


def nw_class(row):
    y = len(row["Y"])
    return NW_CLASSES[0 if y <= 160 else 1 if y <= 320 else 2]


def nw_mid_long_groups(cls):
    """{(igap, egap): rows} of the mid/long NW fixture's rows of one class"""
    groups = {}
    for r in nw_pairs_mid_long():
        if nw_class(r) == cls:
            groups.setdefault((r["igap"], r["egap"]), []).append(r)
    return groups


def mid_form_fits(ig, eg, rows):
    """nw16_kernel.hip:nw16_fits for a launch of these rows on the 10-column form"""
    from tests import synth
    xmax, ymax = max(len(r["X"]) for r in rows), max(len(r["Y"]) for r in rows)
    return ig <= 0 and eg <= 0 and ig >= synth.nw16_limit_igap(10, xmax, ymax, eg)


def ungapped_rows(stem="ungapped"):
    with gzip.open(os.path.join(GOLDEN, stem + ".jsonl.gz"), "rt") as f:
        rows = [json.loads(l) for l in f]
    cases = {}
    for c in sorted({r["case"] for r in rows}):
        with gzip.open(os.path.join(GOLDEN, f"{stem}_case{c}.json.gz"), "rt") as f:
            cases[c] = json.load(f)
    return rows, cases


def ungapped_long_rows():
    """Walks over reads of 161-320 and 600-2500 bases, indels included."""
    return ungapped_rows("ungapped_long")


def seqs_arrays(strs):
    cat = np.frombuffer("".join(strs).encode(), dtype=np.uint8).copy()
    starts = np.cumsum([0] + [len(s) for s in strs[:-1]]).astype(np.uint64)
    return cat, starts


def e2e_cases():
    d = os.path.join(GOLDEN, "e2e")
    return sorted(os.listdir(d))


_unpacked = {}


def _unpack(d, name):
    """The mid- and long-read cases keep db.fa, query.fa and expected.json
    gzipped: plain copies in a directory of this process's own."""
    import atexit
    import shutil
    import tempfile
    if name not in _unpacked:
        if not _unpacked:
            _unpacked[None] = tempfile.mkdtemp(prefix="imsame_golden_")
            atexit.register(shutil.rmtree, _unpacked[None], ignore_errors=True)
        out = os.path.join(_unpacked[None], name)
        os.makedirs(out)
        for f in ("db.fa", "query.fa", "expected.json"):
            with gzip.open(os.path.join(d, f + ".gz"), "rb") as src, open(os.path.join(out, f), "wb") as dst:
                dst.write(src.read())
        _unpacked[name] = out
    return _unpacked[name]


def e2e_case(name):
    d = os.path.join(GOLDEN, "e2e", name)
    src = d if os.path.exists(os.path.join(d, "db.fa")) else _unpack(d, name)
    meta = json.load(open(os.path.join(src, "expected.json")))
    t1 = None
    p = os.path.join(d, "T1.align.gz")
    if os.path.exists(p):
        with gzip.open(p, "rb") as f:
            t1 = f.read()
    return dict(dir=d, db=os.path.join(src, "db.fa"), query=os.path.join(src, "query.fa"), meta=meta, t1=t1)


def align_headers(blob):
    """The (read, record, identity %, coverage %, length) of every record of an
    .align file, sorted."""
    return sorted(tuple(int(v) for v in re.findall(rb"\d+", h.split(b"\n")[0])) for h in HEADER_RE.findall(blob))


def headers_of(lines):
    """expected.json's header lines as the tuples of align_headers"""
    return sorted(tuple(int(v) for v in re.findall(r"\d+", h)) for h in lines)


def result_headers(res):
    """What the .align header of every accepted row of a per-read result array
    holds (alignmentFunctions.c:167-168): the tuples of align_headers."""
    out = []
    for r in range(len(res)):
        x = res[r]
        if x["status"] == 1:
            L, yl = int(x["length"]), int(x["ylen"])
            out.append((r, int(x["db_seq"]), min(100, 100 * int(x["identities"]) // L), min(100, 100 * L // yl), yl))
    return sorted(out)


def case_params(make, case):
    """make(**fields) (Oracle.params, Device.params) for an e2e case's
    command-line options; what the case does not set keeps its default."""
    ex = case["meta"]["extra"]
    a = dict(zip(ex[::2], ex[1::2]))
    names = {"-evalue": ("min_e", float), "-coverage": ("min_coverage", float), "-identity": ("min_identity", float),
             "-igap": ("igap", lambda v: -int(v)), "-egap": ("egap", lambda v: -int(v))}
    assert set(a) <= set(names), a
    return make(**{names[k][0]: names[k][1](v) for k, v in a.items()})


def record_multisets(blob):
    """Header and body multisets of an .align file.  With -n_threads > 1 the
    reference's header and body fprintf calls of different threads interleave
    (alignmentFunctions.c:167-168), but each call is atomic: drop the headers,
    and the remainder is a concatenation of bodies, each ending with the only
    empty line it contains (alignmentFunctions.c:270)."""
    heads = sorted(h.decode().split("\n")[0] + "\n" for h in HEADER_RE.findall(blob))
    rest = HEADER_RE.sub(b"", blob)
    bodies, pos = [], 0
    while pos < len(rest):
        e = rest.find(b"\n\n", pos)
        e = len(rest) if e < 0 else e + 2
        bodies.append(hashlib.sha1(rest[pos:e]).hexdigest())
        pos = e
    return heads, sorted(bodies)


def info_lines(stdout):
    return [m.decode() for m in INFO_RE.findall(stdout)]


def err_lines(stdout):
    return [l.decode() for l in stdout.split(b"\n") if l.startswith(b"ERR")]


def check_cli_against_golden(case, T, rc, stdout, align_blob):
    """Assert a CLI run (oracle or product) matches the reference's golden run."""
    exp = case["meta"]["runs"][str(T)]
    assert rc == exp["rc"], (rc, exp["rc"])
    assert err_lines(stdout) == exp["err"]
    assert info_lines(stdout) == exp["info"]
    if T == 1:
        assert align_blob == case["t1"]
    else:
        heads, bodies = record_multisets(align_blob)
        assert heads == exp["headers"]
        assert bodies == exp["body_sha1s"]
