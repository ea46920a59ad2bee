"""The code that decides which candidates reach NW, on repetitive databases:
the device index build (imsame_dev.hip: mark_record_starts, kmer_code_kernel,
dev_scan, kmer_scatter, segsort_small / _big / _huge) and the seed scan's walk
through long buckets and long rejection lists (seed_kernel.hip).

Direct tests: the index read back from the device (Device.index_read) and the
emulator's host index (emu_build_csr) against synth.index_reference, a plain
numpy statement of the reference's rule, array for array.  Pipeline tests:
align results on families of similar records, on a scan that resumes inside a
bucket and on thousands of identical records against the oracle (run with its
rejected-pair memo), every PARITY_FIELDS column exactly."""
import ctypes as C

import numpy as np
import pytest

import imsame_amd
from imsame_amd import PARITY_FIELDS, abi
from tests import synth
from tests.emu_bind import Emu

ACGT = synth.ACGT
COMBOS = [pytest.param(brk, rel, id=f"{'brk' if brk else 'nobrk'}-{'rel' if rel else 'abs'}")
          for brk in (False, True) for rel in (False, True)]


@pytest.fixture(scope="module")
def repdb():
    return synth.make_repetitive_db()


@pytest.fixture(scope="module")
def rep_reference(repdb):
    """(off, ent) of the plain reference, per (brk, relative); computed once"""
    return {(b, r): synth.index_reference(repdb["seq"], repdb["starts"], repdb["brk"] if b else None, r)
            for b in (False, True) for r in (False, True)}


@pytest.fixture(scope="module")
def dev():
    d = imsame_amd.Device(0)
    yield d
    d.close()


def _same_index(got_off, got_ent, ref):
    off, ent = ref
    assert np.array_equal(got_off, off)
    assert got_ent.dtype == ent.dtype and np.array_equal(got_ent, ent)


# ---------------------------------------------------------------------------
# the fixture itself and the reference (CPU)
# ---------------------------------------------------------------------------
def test_repetitive_db_holds_what_it_claims(repdb, rep_reference):
    off, ent = rep_reference[False, False]
    size = np.diff(off.astype(np.int64))
    for n, code in repdb["planted"].items():
        assert size[code] == n
    off_b, _ = rep_reference[True, False]
    size_b = np.diff(off_b.astype(np.int64))
    for n, code in repdb["planted"].items():
        assert size_b[code] == n                     # resets right before / after a copy lose none
    assert size[repdb["brk_code"]] == synth.PLANTED_BRK
    assert size_b[repdb["brk_code"]] == synth.PLANTED_BRK - synth.PLANTED_BRK_CUT
    assert size[0] > 4096                            # poly-A
    assert (size > 4096).sum() >= 4 + 89 and ((size > 32) & (size <= 4096)).sum() >= 10
    lens = np.diff(np.append(repdb["starts"], len(repdb["seq"])).astype(np.int64))
    assert {0, 1, 11, 12, 13} <= set(lens.tolist()) and lens[-1] == 0 and lens.max() <= 3000
    assert ((lens[:-1] == 0) & (lens[1:] == 0)).any()
    # bucket order: descending position, ties impossible
    e = ent[off[0]:off[1]]
    assert (np.diff(e["x"].astype(np.int64)) < 0).all()
    # the bitmap has a reset at every phase of a 32-bit word, at base 0 and in the last 12 bases
    bits = np.flatnonzero(np.unpackbits(repdb["brk"], bitorder="little"))
    assert set(synth.BRK_PHASES) <= set((bits % 32).tolist())
    assert bits[0] == 0 and (bits >= len(repdb["seq"]) - 12).sum() >= 3
    assert len(rep_reference[True, False][1]) < len(ent)


def test_index_reference_on_a_hand_case():
    """the rule on 30 bases worked by hand: two records (the second starts at
    base 14), a reset before base 20"""
    seq = np.frombuffer(b"ACGTACGTACGTAC" + b"GGGGGGGGGGGGGGTT", np.uint8)
    starts = np.array([0, 14], np.uint64)
    off, ent = synth.index_reference(seq, starts)
    # record 0: 12-mers ending at 11, 12, 13; record 1: ending at 25 .. 29
    assert sorted(ent["x"].tolist()) == [12, 13, 14, 26, 27, 28, 29, 30]
    assert ent["record"][ent["x"] <= 14].tolist() == [0, 0, 0] and (ent["record"][ent["x"] > 14] == 1).all()
    g = synth.kmer_code(b"GGGGGGGGGGGG")
    assert ent[off[g]:off[g + 1]]["x"].tolist() == [28, 27, 26]          # descending
    assert synth.kmer_code(b"ACGTACGTACGT") == int("000110110001101100011011", 2)
    brk = np.zeros(4, np.uint8)
    brk[20 // 8] = 1 << (20 % 8)
    _, ent_b = synth.index_reference(seq, starts, brk)                   # 12-mers ending at 20 .. 30 are lost
    assert sorted(ent_b["x"].tolist()) == [12, 13, 14]
    brk[:] = 0
    brk[18 // 8] = 1 << (18 % 8)                                         # the 12-mer of bases 18 .. 29 starts anew
    _, ent_c = synth.index_reference(seq, starts, brk, relative=True)
    assert sorted(ent_c["x"].tolist()) == [12, 13, 14, 30 - 14] and sorted(ent_c["x"].tolist())[-1] == 16


@pytest.mark.parametrize("brk,rel", COMBOS)
def test_emu_csr_matches_reference(repdb, rep_reference, brk, rel):
    off, ent = Emu.load().build_csr(repdb["seq"], repdb["starts"], repdb["brk"] if brk else None, ent_abs=not rel)
    _same_index(off, ent, rep_reference[brk, rel])


def test_emu_csr_small_databases():
    emu = Emu.load()
    for seq, starts in ((b"", []), (b"", [0]), (b"ACGTACGTACG", [0]), (b"ACGTACGTACGT", [0]), (b"ACGTACGTACGTA", [0, 13])):
        seq = np.frombuffer(seq, np.uint8)
        off, ent = emu.build_csr(seq, np.array(starts, np.uint64))
        _same_index(off, ent, synth.index_reference(seq, np.array(starts, np.uint64)))
        assert len(ent) == max(0, len(seq) - 11)


# ---------------------------------------------------------------------------
# the device index (GPU)
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("brk,rel", COMBOS)
def test_device_index_matches_reference(dev, repdb, rep_reference, brk, rel, monkeypatch):
    if rel:
        monkeypatch.setenv("IMSAME_ENT_REL", "1")
    dev.index(repdb["seq"], repdb["starts"], repdb["brk"] if brk else None)
    off, ent, ent_abs = dev.index_read()
    assert ent_abs == (not rel)
    _same_index(off, ent, rep_reference[brk, rel])


@pytest.mark.gpu
def test_device_index_small_databases(dev):
    for seq, starts in ((b"", []), (b"", [0]), (b"ACGTACGTACG", [0]), (b"ACGTACGTACGT", [0]), (b"ACGTACGTACGTA", [0, 13])):
        seq = np.frombuffer(seq, np.uint8)
        dev.index(seq, np.array(starts, np.uint64))
        off, ent, ent_abs = dev.index_read()
        assert ent_abs
        _same_index(off, ent, synth.index_reference(seq, np.array(starts, np.uint64)))
        assert len(ent) == max(0, len(seq) - 11)


@pytest.mark.gpu
def test_device_index_after_a_larger_one(dev, repdb, rep_reference):
    """the buffers of a larger random database are reused: stale offsets,
    codes, fill counters, big-bucket list and entries"""
    ref, rst = synth.make_reference_arr(4_000_000, 2_000, seed=71)
    dev.index(ref, rst)
    off, ent, _ = dev.index_read()
    assert len(ent) > len(rep_reference[True, False][1])
    dev.index(repdb["seq"], repdb["starts"], repdb["brk"])
    off, ent, _ = dev.index_read()
    _same_index(off, ent, rep_reference[True, False])


@pytest.mark.gpu
def test_device_index_read_errors(repdb):
    L = imsame_amd.lib()
    with imsame_amd.Device(0) as d:
        with pytest.raises(imsame_amd.ImsameError) as e:
            d.index_read()
        assert e.value.code == abi.IMSAME_E_STATE
        d.index(repdb["seq"][:5000], repdb["starts"][repdb["starts"] < 5000])
        off, ent, _ = d.index_read()
        n, ab = C.c_uint64(), C.c_int(-1)
        small = np.full(len(ent) - 1, 0xEE, dtype=np.uint64)
        rc = L.imsame_dev_index_read(d._h, None, small.ctypes.data, len(small), C.byref(n), C.byref(ab))
        assert rc == abi.IMSAME_E_ARG and n.value == len(ent) and ab.value == 1
        assert (small == 0xEE).all()                                  # nothing copied


# ---------------------------------------------------------------------------
# pipeline on repetitive databases against the oracle
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def memo_oracle(oracle):
    """the oracle with its rejected-pair memo: identical results (NW is a pure
    function of the pair), without re-running a rejected record at each hit"""
    oracle.lib.or_last_nw.restype = C.c_uint64
    oracle.lib.or_set_memo_rejected(1)
    yield oracle
    oracle.lib.or_set_memo_rejected(0)


class _EmuBackend:
    name = "emu"

    def __init__(self):
        self.emu = Emu.load()

    def align(self, db, dbs, q, qs, p, T):
        rc, res, _, st = self.emu.align(db, dbs, q, qs, p, T)
        assert rc == 0
        return res, st


class _GpuBackend:
    name = "gpu"

    def __init__(self, dev):
        self.dev = dev

    def align(self, db, dbs, q, qs, p, T):
        self.dev.index(db, dbs)                     # (IMSAME_ENT_REL is read here)
        self.dev.set_query(q, qs)
        res, _, st = self.dev.align(n_threads=T, params=p)
        return res, st


def _reads(rng, src, n, L, sub):
    out = []
    for _ in range(n):
        o = int(rng.integers(0, len(src) - L + 1))
        out.append(synth._substitute(rng, src[o:o + L], sub))
    return out


FAM_IDENTITY = 0.95


@pytest.fixture(scope="module")
def families(memo_oracle):
    """Families of similar records (synth.make_families_db): a read of one
    member passes the e-value on its siblings, runs NW on them and rejects
    them (min_identity 0.95; siblings differ in ~19 % of their bases) -- more
    rejections per read than the memo's MEMO = 16 records and the SPEC_MAX = 8
    candidates of a round.  450 members in the two large families: at 10 %
    substitutions a sibling shares a given 12-mer with a 1 %-read of a member
    with probability 0.9^12 x 0.9^12 x 0.99^12 = 0.07 and the read's own member
    hits nearly every window, so only the siblings of the first window or two
    come before it: 40 members would give about 3 distinct NW per read, 260
    gave 12 by the oracle, 450 give 25.
    Reads of 150 bases:
      low     from each large family's lowest-positioned member (the last of every bucket), 1 % substitutions
      mid     from a middle member
      none    from the family sequence with 8 % substitutions: no member is
              accepted and every window is scanned.  From the family of 20
              (more than MEMO) for both backends; from a large family for the
              device alone: past its 16 memo entries the scan re-aligns the
              other ~430 members at every window they hit, ~1500 NW and ~160
              rounds per read, 18 s per read in the emulator
    and a few random reads.  Returns {backend: (db, dbs, q, qs, {T: expected})}."""
    db, dbs, fam, where = synth.make_families_db()
    rng = np.random.default_rng(516)
    member = lambda r: db[int(dbs[r]):int(dbs[r]) + 300]          # noqa: E731
    cls, reads = [], []
    for f in (0, 1):
        mid = int(where[f][len(where[f]) // 2])
        for name, src, n, own in (("low", member(where[f][0]), 8, int(where[f][0])), ("mid", member(mid), 4, mid)):
            reads += _reads(rng, src, n, 150, 0.01)
            cls += [(name, own)] * n
    reads += _reads(rng, fam[2], 2, 150, 0.08)
    cls += [("none", -1)] * 2
    reads += _reads(rng, fam[0], 1, 150, 0.08) + _reads(rng, fam[1], 1, 150, 0.08)
    cls += [("none_big", -1)] * 2
    for _ in range(4):
        reads.append(ACGT[rng.integers(0, 4, 150)])
        cls.append(("random", -1))
    order = rng.permutation(len(reads))
    reads, cls = [reads[k] for k in order], [cls[k] for k in order]
    p = memo_oracle.params(min_identity=FAM_IDENTITY)

    def query(sel):
        return np.concatenate([reads[k] for k in sel]), np.arange(0, 150 * len(sel), 150, dtype=np.uint64)

    def nw_per_read(name):
        sel = [k for k, c in enumerate(cls) if c[0] == name]
        q, qs = query(sel)
        rc, _, _ = memo_oracle.align(db, dbs, q, qs, p, 1)
        assert rc == 0
        return int(memo_oracle.lib.or_last_nw()) / len(sel)

    out = {}
    for be in ("emu", "gpu"):
        sel = [k for k, c in enumerate(cls) if be == "gpu" or c[0] != "none_big"]
        kind = np.array([cls[k][0] for k in sel])
        own = np.array([cls[k][1] for k in sel])
        q, qs = query(sel)
        exp = {}
        for T in (1, 4):
            rc, exp[T], _ = memo_oracle.align(db, dbs, q, qs, p, T)
            assert rc == 0
            e = exp[T]
            for name in ("low", "mid"):
                m = kind == name
                assert (e["status"][m] == 1).all() and np.array_equal(e["db_seq"][m], own[m].astype(np.uint64)), name
            assert (e["status"][(kind == "none") | (kind == "none_big")] == 0).all()
        out[be] = (db, dbs, q, qs, exp)
    nw_low, nw_none, nw_big = nw_per_read("low"), nw_per_read("none"), nw_per_read("none_big")
    print(f"families: distinct NW per read: low {nw_low:.1f}, none {nw_none:.1f}, none_big {nw_big:.1f}")
    assert nw_low > 16, nw_low
    assert nw_none > 16 and nw_big > 16, (nw_none, nw_big)
    return out


# (environment, params flags) of each variant
FAM_VARIANTS = {
    "default": ({}, 0),
    "L1": ({"IMSAME_SEED_L": "1"}, 0),
    "L4": ({"IMSAME_SEED_L": "4"}, 0),
    "L16": ({"IMSAME_SEED_L": "16"}, 0),
    "L64": ({"IMSAME_SEED_L": "64"}, 0),
    "budget1": ({"IMSAME_SEED_BUDGET": "1"}, 0),
    "budget3": ({"IMSAME_SEED_BUDGET": "3"}, 0),
    "spec1-1": ({"IMSAME_SPEC": "1", "IMSAME_SPEC_WEAK": "1"}, 0),
    "spec2-8": ({"IMSAME_SPEC": "2", "IMSAME_SPEC_WEAK": "8"}, 0),
    "spec8-8": ({"IMSAME_SPEC": "8", "IMSAME_SPEC_WEAK": "8"}, 0),
    "entrel": ({"IMSAME_ENT_REL": "1"}, 0),
    "nw16": ({}, imsame_amd.FLAG_NW16),
    "nw32": ({}, imsame_amd.FLAG_NW32),
}
FAM_EMU = ("default", "L1", "L16", "budget1", "spec1-1")       # the variants the emulator finishes in seconds


def _run_families(be, oracle, families, variant, T, monkeypatch):
    db, dbs, q, qs, exp = families[be.name]
    env, flags = FAM_VARIANTS[variant]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    got, st = be.align(db, dbs, q, qs, oracle.params(min_identity=FAM_IDENTITY, flags=flags), T)
    print(f"families[{be.name}-{variant}-T{T}]: rounds {st.rounds}, NW {st.n_nw}")
    for f in PARITY_FIELDS:
        assert np.array_equal(got[f], exp[T][f]), (f, np.flatnonzero(got[f] != exp[T][f])[:8])


@pytest.mark.parametrize("T", [1, 4])
@pytest.mark.parametrize("variant", FAM_EMU)
def test_families_emu(memo_oracle, families, variant, T, monkeypatch):
    _run_families(_EmuBackend(), memo_oracle, families, variant, T, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("T", [1, 4])
@pytest.mark.parametrize("variant", list(FAM_VARIANTS))
def test_families_gpu(dev, memo_oracle, families, variant, T, monkeypatch):
    _run_families(_GpuBackend(dev), memo_oracle, families, variant, T, monkeypatch)


@pytest.fixture(scope="module")
def resume(memo_oracle):
    """synth.make_resume_db: the oracle accepts the highest-positioned copy for
    every read of the tiling, after rejecting a junction record first for the
    reads that start on one"""
    db, dbs, reads, first, n = synth.make_resume_db()
    q = np.concatenate(reads)
    qs = np.arange(0, len(q), 150, dtype=np.uint64)
    exp = {}
    for T in (1, 4):
        rc, exp[T], _ = memo_oracle.align(db, dbs, q, qs, None, T)
        assert rc == 0
        assert (exp[T]["status"][:12] == 1).all() and (exp[T]["db_seq"][:12] == first + n - 1).all()
    sel = reads[0:12:2]
    rc, _, _ = memo_oracle.align(db, dbs, np.concatenate(sel), np.arange(0, 150 * len(sel), 150, dtype=np.uint64), None, 1)
    assert rc == 0 and int(memo_oracle.lib.or_last_nw()) >= 2 * len(sel)
    return db, dbs, q, qs, exp


RESUME_VARIANTS = ("default", "L4", "L16", "L64", "spec1-1", "budget1", "entrel")


def _run_resume(be, oracle, resume, variant, T, monkeypatch):
    db, dbs, q, qs, exp = resume
    for k, v in FAM_VARIANTS[variant][0].items():
        monkeypatch.setenv(k, v)
    got, st = be.align(db, dbs, q, qs, oracle.params(), T)
    _same(got, exp[T])


@pytest.mark.parametrize("T", [1, 4])
@pytest.mark.parametrize("variant", RESUME_VARIANTS)
def test_resume_inside_a_bucket_emu(memo_oracle, resume, variant, T, monkeypatch):
    _run_resume(_EmuBackend(), memo_oracle, resume, variant, T, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("T", [1, 4])
@pytest.mark.parametrize("variant", RESUME_VARIANTS + ("L1",))
def test_resume_inside_a_bucket_gpu(dev, memo_oracle, resume, variant, T, monkeypatch):
    _run_resume(_GpuBackend(dev), memo_oracle, resume, variant, T, monkeypatch)


@pytest.fixture(scope="module")
def copies(memo_oracle, repdb):
    """Reads on the repetitive database at default params.  Every copy of the
    5000-fold record gives the same NW row, so db_seq alone tells which copy
    the scan visited first: the reference's is the highest-positioned one.
      copy    150 bases of the tiled 100-base record, 1 % substitutions
      polya, dinuc, tiled   reads that lie in those records
      planted a true read of a unique record whose first (or 70th .. 82nd) 12
              bases are the 12-mer planted 4097 / 8193 times: the scan walks,
              and with a budget pauses in, a bucket of thousands of hits that
              fail the e-value
    and 10 % random reads.  No read rejects every copy of a huge bucket."""
    db, dbs = repdb["seq"], repdb["starts"]
    rng = np.random.default_rng(616)
    rec = lambda r: db[int(dbs[r]):(int(dbs[r + 1]) if r + 1 < len(dbs) else len(db))]     # noqa: E731
    u0, un, _ = repdb["unique"]
    tiled_copy = np.tile(repdb["copy_unit"], 4)
    reads, kind = [], []
    for _ in range(40):
        reads += _reads(rng, tiled_copy, 1, 150, 0.01)
        kind.append("copy")
    for name, r, n in (("polya", repdb["polya"], 12), ("dinuc", repdb["dinuc"], 8), ("tiled", repdb["tiled"], 8)):
        reads += _reads(rng, rec(r), n, 150, 0.01)
        kind += [name] * n
    for n in (4097, 8193):
        w = np.frombuffer(repdb["words"][n], np.uint8)
        for k in range(12):
            y = _reads(rng, rec(u0 + int(rng.integers(0, un))), 1, 150, 0.01)[0]
            at = 0 if k % 2 == 0 else 70
            y[at:at + 12] = w
            reads.append(y)
            kind.append("planted")
    for _ in range(len(reads) // 9):
        reads.append(ACGT[rng.integers(0, 4, 150)])
        kind.append("random")
    order = rng.permutation(len(reads))
    reads, kind = [reads[k] for k in order], np.array([kind[k] for k in order])
    q = np.concatenate(reads)
    qs = np.arange(0, len(q), 150, dtype=np.uint64)
    exp = {}
    last_copy = repdb["copy_first"] + synth.COPY_N - 1
    for T in (1, 4):
        rc, exp[T], _ = memo_oracle.align(db, dbs, q, qs, None, T)
        assert rc == 0
        e = exp[T]
        m = kind == "copy"
        assert (e["status"][m] == 1).all() and (e["db_seq"][m] == last_copy).all()
        m = kind == "polya"
        assert (e["status"][m] == 1).all() and (e["db_seq"][m] == repdb["polya"] + 2).all()
        for name in ("dinuc", "tiled"):
            m = kind == name
            assert (e["status"][m] == 1).all() and (e["db_seq"][m] == repdb[name]).all()
        m = kind == "planted"
        # (a few are accepted before their origin, on a record of the walked bucket: a weak e-value
        # pass whose NW reaches identity 0.5)
        assert (e["status"][m] == 1).all() and ((e["db_seq"][m] >= u0) & (e["db_seq"][m] < u0 + un)).sum() >= 18
    return db, dbs, q, qs, exp


def _same(got, exp):
    for f in PARITY_FIELDS:
        assert np.array_equal(got[f], exp[f]), (f, np.flatnonzero(got[f] != exp[f])[:8])


@pytest.mark.gpu
@pytest.mark.parametrize("T", [1, 4])
@pytest.mark.parametrize("variant", ["default", "L1", "L16", "budget1", "entrel"])
def test_copies_gpu(dev, copies, variant, T, monkeypatch):
    db, dbs, q, qs, exp = copies
    for k, v in FAM_VARIANTS[variant][0].items():
        monkeypatch.setenv(k, v)
    got, st = _GpuBackend(dev).align(db, dbs, q, qs, dev.params(), T)
    print(f"copies[{variant}-T{T}]: rounds {st.rounds}, NW {st.n_nw}")
    _same(got, exp[T])


@pytest.mark.gpu
@pytest.mark.parametrize("slice_bases", [150_000, 100_000])
def test_copies_sliced_gpu(dev, copies, slice_bases):
    """the 5000 copies (500 kbp) cut into several slices: the first accepted
    pair across slices is the highest slice's (LIFO order across slices)"""
    db, dbs, q, qs, exp = copies
    dev.set_query(q, qs)
    for T in (1, 4):
        got, _, _, ns = dev.align_sliced(db, dbs, slice_bases, n_threads=T)
        assert ns >= len(db) // slice_bases and ns >= 4
        _same(got, exp[T])


@pytest.mark.gpu
def test_copies_db_shards_min_merge_gpu(dev, copies):
    """test_gpu.py:test_db_shards_min_merge_matches_whole's merge over 3
    shards of the repetitive database"""
    from imsame_amd.dist import db_shard_records, merge_shard_results
    db, dbs, q, qs, exp = copies
    dev.set_query(q, qs)
    world = 3
    for T in (1, 4):
        parts = []
        for rank in range(world):
            lo, hi = db_shard_records(dbs, len(db), rank, world)
            base = int(dbs[lo])
            end = int(dbs[hi]) if hi < len(dbs) else len(db)
            dev.index(db[base:end], dbs[lo:hi] - np.uint64(base))
            res, win, _ = dev.align_windows(len(db), n_threads=T)
            parts.append((res, win, lo))
        _same(merge_shard_results(parts), exp[T])
