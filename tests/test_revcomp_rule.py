"""The rule that makes the windows of imsame_dev_revcomp_stream exact, on the
oracle (no GPU).

reverseComplement.c emits records last first; a record's header runs from its
'>' through the first '\\n', its body to the next '>' at or after the header's
end.  A '>' at p is a CLEAN OPENER when, scanning backwards from p, the first
byte among {'>', '\\n'} is a '\\n', or the file starts: it lies in no header,
and every earlier record ends at or before it.  Cut an image at any set of
clean openers and the whole output is the pieces' outputs, last piece first.
A cut at any other '>' is not exact.  The device code cuts at the first '>'
after a window's first '\\n', which is always a clean opener."""
import numpy as np

ALPHABET = np.frombuffer(b"ACGTacgtNnUuRY*-\r\n\n\n>>", dtype=np.uint8)


def clean_openers(img):
    out = []
    clean = True                   # the file's start counts as a '\n'
    for p, c in enumerate(img):
        if c == 0x3E:
            if clean:
                out.append(p)
            clean = False
        elif c == 0x0A:
            clean = True
    return out


def pieces_last_first(oracle, img, cuts):
    """cuts: ascending clean openers; bytes before the first cut belong to a
    piece of their own only when they hold a record."""
    cuts = sorted(cuts)
    bounds = [0] + cuts + [len(img)]
    parts = [img[a:b] for a, b in zip(bounds[:-1], bounds[1:])]
    return b"".join(oracle.revcomp(p) for p in reversed(parts))


def random_images(n, seed):
    rng = np.random.default_rng(seed)
    for _ in range(n):
        yield ALPHABET[rng.integers(0, len(ALPHABET), int(rng.integers(0, 400)))].tobytes()


def test_cuts_at_clean_openers_are_exact(oracle):
    rng = np.random.default_rng(11)
    checked = 0
    for img in random_images(300, 7):
        whole = oracle.revcomp(img)
        co = clean_openers(img)
        for _ in range(4):
            cuts = [p for p in co if rng.integers(0, 2)]
            assert pieces_last_first(oracle, img, cuts) == whole, (img, cuts)
            checked += 1
        assert pieces_last_first(oracle, img, co) == whole, img
    assert checked == 1200


def test_first_gt_after_first_newline_is_a_clean_opener(oracle):
    """the cut the stream takes in a window [w0, e): whatever precedes w0"""
    for img in random_images(300, 8):
        co = set(clean_openers(img))
        for w0 in range(1, len(img)):
            nl = img.find(b"\n", w0)
            g = img.find(b">", nl + 1) if nl >= 0 else -1
            if g >= 0:
                assert g in co, (img, w0, g)


def test_cut_inside_a_header_differs(oracle):
    img = b">a>b\nAC\n"
    assert clean_openers(img) == [0]
    assert oracle.revcomp(img) == b">b\nGT\n>a>b\nGT\n"
    assert pieces_last_first(oracle, img, [2]) == b">b\nGT\n>a\n"
    # every '>' that is no clean opener, on random images: the cut changes the output
    bad = 0
    for img in random_images(200, 9):
        whole = oracle.revcomp(img)
        co = set(clean_openers(img))
        for p, c in enumerate(img):
            if c == 0x3E and p not in co:
                assert pieces_last_first(oracle, img, [p]) != whole, (img, p)
                bad += 1
    assert bad > 500
