"""Canonical synthetic inputs.

numpy PCG64, iid uniform ACGT reference cut into fixed-length records;
"Illumina-like" reads: 90 % sampled uniformly from the reference
concatenation (record boundaries may be crossed) with 1 % substitutions (to a
different base), 0.05 % insertions, 0.05 % deletions; 10 % iid random reads.

Array forms return (seq: uint8[ACGT bytes], starts: uint64[n]) -- the exact
shape of the reference loaders' output (IMSAME.c:194-371) -- so large
workloads never go through Python strings.
"""
import numpy as np

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def make_reference_arr(total, rec_len, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    seq = ACGT[rng.integers(0, 4, total, dtype=np.uint8)]
    starts = np.arange(0, total, rec_len, dtype=np.uint64)
    return seq, starts


def make_reference(total, rec_len, seed):
    seq, starts = make_reference_arr(total, rec_len, seed)
    b = seq.tobytes().decode()
    return [b[s:s + rec_len] for s in starts.tolist()]


def _mutate_rows(rng, src, L, sub, ins, dele):
    """src: (n, L+pad) uint8 windows -> (n, L) reads with substitutions and
    (rare) indels; indel reads are re-built individually."""
    n, W = src.shape
    src = src.copy()
    # substitutions to a different base
    m = rng.random((n, W)) < sub
    if m.any():
        codes = np.searchsorted(ACGT, src[m])
        src[m] = ACGT[(codes + rng.integers(1, 4, codes.shape[0])) % 4]
    out = src[:, :L].copy()
    # indels: a deleted source base emits nothing, an insertion emits a random
    # base before its source base; rows are then cut to L (padded if short)
    ev = rng.random((n, W))
    rows = np.flatnonzero((ev < ins + dele).any(axis=1))
    if len(rows):
        e = ev[rows]
        keep = e >= dele
        insb = keep & (e < dele + ins)
        emit = keep.astype(np.int64) + insb
        pos = np.cumsum(emit, axis=1)                          # one past this base's slot
        buf = ACGT[rng.integers(0, 4, (len(rows), 2 * W + 1), dtype=np.uint8)]
        rr = np.broadcast_to(np.arange(len(rows))[:, None], e.shape)
        buf[rr[keep], (pos - 1)[keep]] = src[rows][keep]
        out[rows] = buf[:, :L]
    return out


def make_reads_arr(ref_seq, n, L, seed, sub=0.01, ins=0.0005, dele=0.0005, frac_true=0.9):
    """ref_seq: uint8 concatenation.  Returns (seq uint8[n*L], starts uint64[n])."""
    rng = np.random.Generator(np.random.PCG64(seed))
    pad = 8
    is_true = rng.random(n) < frac_true
    reads = np.empty((n, L), dtype=np.uint8)
    nt = int(is_true.sum())
    if nt:
        off = rng.integers(0, len(ref_seq) - (L + pad), nt)
        idx = off[:, None] + np.arange(L + pad)[None, :]
        reads[is_true] = _mutate_rows(rng, ref_seq[idx], L, sub, ins, dele)
    nr = n - nt
    if nr:
        reads[~is_true] = ACGT[rng.integers(0, 4, (nr, L), dtype=np.uint8)]
    starts = np.arange(0, n * L, L, dtype=np.uint64)
    return reads.reshape(-1), starts


def make_long_reads_arr(ref_seq, n, L, seed, sub=0.05, ins=0.025, dele=0.025, frac_true=0.9, chunk=1000):
    """C5's ONT-like long reads (5 % substitutions, 2.5 %
    insertions, 2.5 % deletions), generated `chunk` reads at a time so
    100k x 10 kbp stays within a few hundred MB of scratch.  Returns
    (seq uint8[n*L], starts uint64[n])."""
    rng = np.random.Generator(np.random.PCG64(seed))
    pad = int(L * dele * 1.5) + 64                    # deletions consume source bases
    out = np.empty((n, L), dtype=np.uint8)
    for c0 in range(0, n, chunk):
        m = min(chunk, n - c0)
        is_true = rng.random(m) < frac_true
        blk = ACGT[rng.integers(0, 4, (m, L), dtype=np.uint8)]
        nt = int(is_true.sum())
        if nt:
            off = rng.integers(0, len(ref_seq) - (L + pad), nt)
            idx = off[:, None] + np.arange(L + pad)[None, :]
            blk[is_true] = _mutate_rows(rng, ref_seq[idx], L, sub, ins, dele)
        out[c0:c0 + m] = blk
    return out.reshape(-1), np.arange(0, n * L, L, dtype=np.uint64)


def make_reads(ref_records, n, L, seed, sub=0.01, ins=0.0005, dele=0.0005, frac_true=0.9):
    cat = np.frombuffer("".join(ref_records).encode(), dtype=np.uint8)
    seq, starts = make_reads_arr(cat, n, L, seed, sub, ins, dele, frac_true)
    b = seq.tobytes().decode()
    return [b[s:s + L] for s in starts.tolist()]


def to_fasta(seq, starts, prefix, width=80):
    """Array form -> FASTA bytes (LF, `>prefix_<i>` headers)."""
    b = seq.tobytes()
    ends = list(starts[1:].tolist()) + [len(b)]
    out = []
    for i, (s, e) in enumerate(zip(starts.tolist(), ends)):
        out.append(f">{prefix}_{i}\n".encode())
        if width:
            for k in range(s, e, width):
                out.append(b[k:min(e, k + width)] + b"\n")
        else:
            out.append(b[s:e] + b"\n")
    return b"".join(out)


def write_fasta(path, seq, starts, prefix, width=80):
    with open(path, "wb") as f:
        f.write(to_fasta(seq, starts, prefix, width))




def make_genome_pool(n_genomes, genome_bp, seed):
    """C4's shared pool: n iid uniform genomes."""
    rng = np.random.Generator(np.random.PCG64(seed))
    return [ACGT[rng.integers(0, 4, genome_bp, dtype=np.uint8)] for _ in range(n_genomes)]


def make_metagenome_arr(pool, abundance, n, L, seed, sub=0.01, ins=0.0005, dele=0.0005, rc_frac=0.5):
    """n reads of length L drawn from the pool's genomes with the given
    abundance vector, Illumina-like errors, a fraction from the reverse
    strand.  Returns (seq uint8[n*L], starts uint64[n])."""
    rng = np.random.Generator(np.random.PCG64(seed))
    ab = np.asarray(abundance, dtype=np.float64)
    who = rng.choice(len(pool), size=n, p=ab / ab.sum())
    out = np.empty((n, L), np.uint8)
    for g in range(len(pool)):
        rows = np.flatnonzero(who == g)
        if not len(rows):
            continue
        s, _ = make_reads_arr(pool[g], len(rows), L, int(rng.integers(1 << 62)), sub, ins, dele, frac_true=1.0)
        s = s.reshape(len(rows), L)
        flip = rng.random(len(rows)) < rc_frac
        s[flip] = s[flip][:, ::-1]
        lut = np.zeros(256, np.uint8)
        lut[np.frombuffer(b"ACGT", np.uint8)] = np.frombuffer(b"TGCA", np.uint8)
        s[flip] = lut[s[flip]]
        out[rows] = s
    return out.reshape(-1), np.arange(0, n * L, L, dtype=np.uint64)


def adversarial_long_pairs():
    """Long pairs near the packed long kernel's size limit (nwp_fits: records
    and reads up to ~13.9 kbp at igap 5, egap 2) where its int16 frames are
    stressed most: scores climbing 4 per row over 12 kbp, tandem and
    dinucleotide repeats (long runs of equal maxima, ties in every column
    max), a 3 kbp deletion, homopolymer runs, a random pair (scores falling),
    and a read longer than its record."""
    rng = np.random.default_rng(77)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    rnd = lambda n: acgt[rng.integers(0, 4, n)]           # noqa: E731
    unit = rnd(37)
    x1 = rnd(13_900)
    rep = np.tile(unit, 376)[:13_900]
    ac = np.tile(np.frombuffer(b"AC", dtype=np.uint8), 6950)
    x4 = rnd(13_900)
    hp = np.concatenate([np.full(4000, ord("A"), np.uint8), rnd(5000), np.full(4900, ord("A"), np.uint8)])
    y7 = rnd(13_500)
    pairs = [
        (x1, x1[500:13_000]),                                             # identical 12.5 kbp
        (rep, rep[11:11 + 13_000]),                                       # tandem repeat, shifted
        (ac, np.concatenate([ac[:5000], rnd(1500), ac[:5000]])),          # dinucleotide + insertion
        (x4, np.concatenate([x4[:5000], x4[8000:]])),                     # 3 kbp deletion
        (hp, np.concatenate([np.full(3000, ord("A"), np.uint8), hp[4000:9000], np.full(3000, ord("A"), np.uint8)])),
        (rnd(13_900), rnd(12_000)),                                       # random: falling scores
        (y7[3000:9000].copy(), y7),                                       # read longer than its record
    ]
    return [x.tobytes() for x, _ in pairs], [y.tobytes() for _, y in pairs]


def adversarial_short_pairs(xl, yl):
    """13 short-read pairs at one shape -- every read has yl bases, the
    longest record xl -- built to push the packed int16 kernel's drifting
    terms (nw16_kernel.hip, nw16_fits) to the ends of their range: scores
    that only fall (no match anywhere), that climb 4 per row on the first or
    last diagonal, a read that jumps from the record's head to its tail (one
    gap of xl - yl), tandem and dinucleotide repeats (ties in every column
    maximum), and short records beside long ones in one lockstep wave (rows
    past a record's end are garbage the range proof covers)."""
    rng = np.random.default_rng(177)
    rnd = lambda n: ACGT[rng.integers(0, 4, n)]             # noqa: E731
    full = lambda n, b: np.full(n, ord(b), np.uint8)        # noqa: E731
    x = rnd(xl)
    h = yl // 2
    unit = rnd(7)
    rep = np.tile(unit, xl // 7 + 2)
    assert xl >= yl
    x8 = np.concatenate([rnd(yl), full(xl - yl, "C")])
    y8 = x8[:yl].copy()
    y8[y8 == ord("C")] = ord("G")
    ac = np.frombuffer(b"AC", dtype=np.uint8)
    pairs = [
        (full(xl, "A"), full(yl, "C")),                                        # 1 no match at all
        (x, x[-yl:]),                                                          # 2 the record's tail
        (x, x[:yl]),                                                           # 3 the record's head
        (full(xl, "A"), full(yl, "A")),                                        # 4 every cell a match
        (rnd(12), rnd(yl)),                                                    # 5 lockstep partner: garbage rows
        (rnd(xl), rnd(yl)),                                                    # 6 unrelated
        (rep[:xl], rep[3:3 + yl]),                                             # 7 tandem repeat, shifted by 3
        (x8, y8),                                                              # 8 head with C -> G, then all C
        (np.concatenate([full(xl // 2, "A"), full(xl - xl // 2, "C")]),
         np.concatenate([full(h, "A"), full(yl - h, "C")])),                   # 9 two homopolymer halves
        (np.tile(ac, xl // 2 + 1)[:xl], np.tile(ac, yl // 2 + 1)[:yl]),        # 10 dinucleotide
        (x, np.concatenate([x[:h], x[len(x) - (yl - h):]])),                   # 11 head + tail: one long gap
        (full(13, "A"), full(yl, "A")),                                        # 12 a 13-base record
        (x[:yl].copy(), x[:yl].copy()),                                        # 13 identical, square
    ]
    assert all(len(b) == yl for _, b in pairs) and max(len(a) for a, _ in pairs) == xl
    return [a.tobytes() for a, _ in pairs], [b.tobytes() for _, b in pairs]


def nw16_limit_igap(K, xmax, ymax, egap):
    """The strongest (most negative) open penalty the packed kernel's range
    proof admits for K columns per lane, records <= xmax, reads <= ymax and
    extension penalty egap -- nw16_kernel.hip:nw16_fits's documented bound
    4 ycols + |ig| + |eg| (xmax + 64 + ycols + 2) + 16 <= 8191."""
    ycols = -(-ymax // K) * K
    return -(8191 - 16 - 4 * ycols - abs(egap) * (xmax + 64 + ycols + 2))


# nw16 at the limit of its range proof: (id, environment, K the launch must
# report, xmax, ymax, [(egap, igap at the limit), ...])
NW16_LIMIT_CASES = [
    ("k10_2000x160", {}, 10, 2000, 160, [(0, -7535), (-1, -5309), (-2, -3083), (-3, -857)]),
    ("k5_2000x160", {"IMSAME_NW_K": "5"}, 5, 2000, 160, [(0, -7535), (-1, -5309), (-2, -3083), (-3, -857)]),
    ("k3_2000x150", {"IMSAME_NW_K": "3"}, 3, 2000, 150, [(0, -7575), (-1, -5359), (-2, -3143), (-3, -927)]),
    ("k10_2000x150", {"IMSAME_NW_K19": "0"}, 10, 2000, 150, [(0, -7575), (-1, -5359), (-2, -3143), (-3, -927)]),
    ("k19_2000x150", {}, 19, 2000, 150, [(0, -7567), (-1, -5349), (-2, -3131), (-3, -913)]),
    ("k19_700x150", {}, 19, 700, 150, [(-8, -223)]),
    ("k10_300x160", {}, 10, 300, 160, [(-3, -5957), (-8, -3327)]),
    ("k10_3000x31", {}, 10, 3000, 31, [(-1, -4909), (-2, -1803)]),
]


# ---------------------------------------------------------------------------
# the database index, restated (tests/test_index_repeats.py)
# ---------------------------------------------------------------------------
INDEX_K = 12
INDEX_BUCKETS = 4 ** INDEX_K


def kmer_code(word):
    """code of a 12-mer (bytes / uint8 array): 2 bits per base, A0 C1 G2 T3,
    the first base most significant"""
    c = 0
    for b in np.searchsorted(ACGT, np.frombuffer(bytes(word), dtype=np.uint8)).tolist():
        c = c * 4 + b
    return c


def index_reference(seq, starts, brk=None, relative=False):
    """The 12-mer index by the rule the reference follows (IMSAME.c:229-281):
    for every base p >= 11 the 12-mer ending at p is indexed unless a reset --
    a record start, or a set bit of brk (LSB-first) -- lies before one of the
    bases p-10 .. p.  Its record is the last one whose start is <= p, its
    stored position p + 1 (relative: minus that record's start).  Buckets
    ascend by code; inside a bucket positions descend (the reference's LIFO
    chain).  Returns (off uint64[4^12 + 1], ent {x, record} uint32 pairs)."""
    from imsame_amd.abi import ENT_DTYPE
    seq = np.asarray(seq, dtype=np.uint8)
    st = np.asarray(starts, dtype=np.int64)
    L, K = len(seq), INDEX_K
    off = np.zeros(INDEX_BUCKETS + 1, dtype=np.uint64)
    if L < K:
        return off, np.zeros(0, dtype=ENT_DTYPE)
    reset = np.zeros(L, dtype=bool)
    reset[st[st < L]] = True
    if brk is not None:
        bits = np.unpackbits(np.asarray(brk, dtype=np.uint8), bitorder="little")[:L]
        reset[:len(bits)] |= bits.astype(bool)
    nres = np.concatenate([[0], np.cumsum(reset)])                 # resets among bases [0, i)
    p = np.arange(K - 1, L, dtype=np.int64)
    two = np.searchsorted(ACGT, seq).astype(np.int64)
    code = np.zeros(L - K + 1, dtype=np.int64)
    for t in range(K):
        code = code * 4 + two[t:t + L - K + 1]                     # the 12-mer that starts at p - 11
    keep = nres[p + 1] == nres[p - (K - 2)]                        # no reset at p-10 .. p
    p, code = p[keep], code[keep]
    rec = np.searchsorted(st, p, side="right") - 1
    order = np.lexsort((-p, code))
    p, rec = p[order], rec[order]
    ent = np.zeros(len(p), dtype=ENT_DTYPE)
    ent["x"] = p + 1 - (st[rec] if relative else 0)
    ent["record"] = rec
    off[1:] = np.cumsum(np.bincount(code, minlength=INDEX_BUCKETS))
    return off, ent


def _rand(rng, n):
    return ACGT[rng.integers(0, 4, n)]


def _substitute(rng, y, rate):
    y = y.copy()
    m = rng.random(len(y)) < rate
    y[m] = ACGT[(np.searchsorted(ACGT, y[m]) + rng.integers(1, 4, int(m.sum()))) % 4]
    return y


# copies of the planted 12-mers: both sides of the index sort's limits (32
# entries: insertion sort / bitonic; 4096: LDS / global scratch; padded sizes
# 4096 in LDS, 8192 and 16384 in scratch)
PLANTED_COUNTS = (1, 2, 31, 32, 33, 64, 65, 4095, 4096, 4097, 8192, 8193)
PLANTED_BRK = 48          # one more planted 12-mer: resets inside PLANTED_BRK_CUT of its copies
PLANTED_BRK_CUT = 10
COPY_LEN, COPY_N = 100, 5000
BRK_PHASES = (0, 1, 20, 21, 22, 30, 31)


def make_repetitive_db(seed=2024):
    """One database of ~1.5 Mbp for the index tests: planted 12-mers, repeats,
    record edges and a reset bitmap.  Returns a dict:
      seq, starts, brk        the database (brk: the optional reset bitmap)
      planted                 {copies: code} of the 12-mers planted `copies` times
      brk_code                the 12-mer planted PLANTED_BRK times, PLANTED_BRK_CUT of them cut by brk
      copy_unit, copy_first   the 100-base record repeated COPY_N times, and its first record
      polya, dinuc, tiled     record numbers of the first poly-A, the dinucleotide and the tiled record
      unique                  (first record, record count, record length) of plain random records
      words                   {copies: 12-mer bytes}
    The generator asserts, from index_reference alone, that the buckets hold
    exactly these sizes with and without brk."""
    for attempt in range(64):
        d = _repetitive_db(np.random.default_rng([seed, attempt]))
        if d is not None:
            return d
    raise AssertionError("no layout with exact planted counts")


def _repetitive_db(rng):
    counts = list(PLANTED_COUNTS) + [PLANTED_BRK]
    # distinct 12-mers; the huge buckets' codes ascend with their size, so the
    # build meets them in growing order (its scratch area is regrown)
    codes = np.sort(rng.choice(np.arange(1 << 10, INDEX_BUCKETS - (1 << 10)), len(counts), replace=False))
    words = {}
    for n, c in zip(sorted(counts), codes.tolist()):
        words[n] = ACGT[[(c >> (2 * (INDEX_K - 1 - t))) & 3 for t in range(INDEX_K)]]
    wid = rng.permutation(np.repeat(np.arange(len(counts)), counts))
    wtab = np.stack([words[n] for n in counts])
    units = np.empty((len(wid), 32), dtype=np.uint8)               # 20 random bases, then the 12-mer
    units[:, :20] = _rand(rng, (len(wid), 20))
    units[:, 20:] = wtab[wid]
    parts, lens = [], []                                           # records, in order

    def rec(a):
        parts.append(np.asarray(a, dtype=np.uint8))
        lens.append(len(a))

    # planted zone: records of ragged lengths 13 .. 3000: 0 .. 31 random bases
    # (the copies' positions take every phase of a 32-bit bitmap word), then
    # whole units
    u, word_pos = 0, [[] for _ in counts]
    base = 0
    while u < len(wid):
        k = int(min(len(wid) - u, rng.choice([0, 1, 2, 5, 20, 60, 92], p=[.1, .2, .2, .2, .15, .1, .05])))
        pad = int(rng.integers(13, 32)) if k == 0 else int(rng.integers(0, 32))
        rec(np.concatenate([_rand(rng, pad), units[u:u + k].reshape(-1)]))
        for j in range(k):
            word_pos[wid[u + j]].append(base + pad + 32 * j + 20)  # first base of the copy
        base += lens[-1]
        u += k
    info = {}
    # repeats
    info["polya"] = len(lens)
    for _ in range(3):
        rec(np.full(2000, ord("A"), np.uint8))
    info["dinuc"] = len(lens)
    rec(np.tile(np.frombuffer(b"AC", np.uint8), 750))
    info["tiled"] = len(lens)
    rec(np.tile(_rand(rng, 7), 200))
    unit = _rand(rng, COPY_LEN)
    info["copy_unit"], info["copy_first"] = unit, len(lens)
    for _ in range(COPY_N):
        rec(unit)
    # plain random records (reads' unique origins; resets at every bitmap phase)
    info["unique"] = (len(lens), 60, 700)
    uniq_base = sum(lens)
    for _ in range(60):
        rec(_rand(rng, 700))
    # record edges: 12, 0, 0, 1, 11, 13, 0, 12 bases, a k-mer across two
    # records at every start, then 40 bases and an empty last record
    for n in (12, 0, 0, 1, 11, 13, 0, 12, 40, 0):
        rec(_rand(rng, n))
    seq = np.concatenate(parts)
    starts = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
    L = len(seq)
    assert int(starts[-1]) == L and lens[-2] == 40
    # the reset bitmap
    bit = np.zeros(8 * ((L + 7) // 8), dtype=np.uint8)
    words32 = rng.choice(np.arange(uniq_base // 32 + 1, (uniq_base + 60 * 700) // 32), 700, replace=False)
    bit[words32 * 32 + rng.choice(BRK_PHASES, len(words32))] = 1
    for w, n in enumerate(counts):                 # right before and after planted copies: none is lost
        pos = np.array(word_pos[w])
        if n == PLANTED_BRK:                       # ... and inside: those copies are not indexed
            for k, s in enumerate(pos[:PLANTED_BRK_CUT]):
                bit[s + (1, 5, 11)[k % 3]] = 1
            continue
        some = pos[rng.random(len(pos)) < 0.1] if n > 2 else pos
        bit[some[0::3]] = 1                        # the copy's first base: the reset before it
        bit[some[1::3] + INDEX_K] = 1              # the base after the copy
        bit[some[2::3] - 1] = 1
    bit[0] = 1
    bit[[L - 12, L - 7, L - 1]] = 1
    brk = np.packbits(bit, bitorder="little")
    # the fixture's proof: exact bucket sizes by the plain reference
    sizes = {}
    for b in (None, brk):
        off, _ = index_reference(seq, starts, b)
        size = np.diff(off.astype(np.int64))
        for n in counts:
            want = n - (PLANTED_BRK_CUT if (n == PLANTED_BRK and b is not None) else 0)
            if size[kmer_code(words[n])] != want:
                return None                        # a 12-mer arose by chance elsewhere: draw again
        if b is None:
            assert size[0] == 3 * (2000 - 11)
            ucodes = [kmer_code(unit[t:t + INDEX_K]) for t in range(COPY_LEN - INDEX_K + 1)]
            if len(set(ucodes)) != len(ucodes) or not (size[ucodes] == COPY_N).all():
                return None
        sizes[b is not None] = size
    info.update(seq=seq, starts=starts, brk=brk, words={n: words[n].tobytes() for n in counts},
                planted={n: kmer_code(words[n]) for n in PLANTED_COUNTS}, brk_code=kmer_code(words[PLANTED_BRK]))
    return info


def make_families_db(seed=515, members=(450, 450, 20), length=300, total=300_000, sub=0.10):
    """~300 kbp of 300-base records: one family per entry of `members` (the
    family sequence with each member's own substitutions) scattered among
    random records.  Returns (seq, starts, family sequences, member record
    numbers per family, ascending)."""
    rng = np.random.default_rng(seed)
    n_rec = total // length
    perm = rng.permutation(n_rec)
    recs = _rand(rng, (n_rec, length))
    fam, where, u = [], [], 0
    for m in members:
        fam.append(_rand(rng, length))
        where.append(np.sort(perm[u:u + m]))
        u += m
        for r in where[-1]:
            recs[r] = _substitute(rng, fam[-1], sub)
    return recs.reshape(-1), np.arange(0, n_rec * length, length, dtype=np.uint64), fam, where


def make_resume_db(seed=717, copies=40):
    """A scan that resumes inside a bucket (its cursor's hit rank > 0) while
    the windows next to it hold the record to accept.  A 100-base unit is in
    the database `copies` times back to back; below them lie 70-base records cut
    from the unit's tiling across a junction (phases 89 .. 99), which own the
    12-mers that span two copies -- no copy is indexed with those.  A read of
    the tiling that starts at such a phase meets the 70-base record alone in
    its first windows: it passes the e-value, covers 70 / 150 of the read and
    is rejected, and the scan resumes after that hit.  Seven or fewer windows
    on, the buckets hold every copy, the highest-positioned first: any copy
    would be accepted with the same NW row, so db_seq tells which one the scan
    took first.  Returns (seq, starts, reads, first copy record, copies); reads
    0, 2, .. 10 start at a junction phase, 1, 3, .. 11 three bases before one,
    the last two are random."""
    rng = np.random.default_rng(seed)
    unit = _rand(rng, 100)
    tiling = np.tile(unit, 4)
    recs = [_rand(rng, 300) for _ in range(100)]
    phases = (89, 91, 93, 95, 97, 99)
    recs += [tiling[f:f + 70] for f in phases]
    recs += [tiling[93:93 + 70]] * 8               # nine of phase 93: more than a round's 8 candidates,
                                                   # so a round ends inside their bucket at rank 8
    first = len(recs)
    recs += [unit] * copies
    recs += [_rand(rng, 300) for _ in range(20)]
    lens = [len(r) for r in recs]
    reads = []
    for f in phases:
        for back in (0, 3):                        # the junction record's first own window: the read's first, or its fourth
            y = tiling[f - back:f - back + 150].copy()
            y[90:] = _substitute(rng, y[90:], 0.02)
            reads.append(y)
    reads += [_rand(rng, 150) for _ in range(2)]
    return (np.concatenate(recs), np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64), reads, first, copies)
