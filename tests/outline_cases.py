"""Masks for the contour / pixel-list kernels of csrc/outline.hip and for analyze.outline_statement, shared by
tests/test_outline_cpu.py and tests/test_outline_gpu.py: the yardstick is analyze.find_contours on the 1-padded mask (padding
subtracted, flipped to (x, y)) and np.argwhere.  Frames are at most 132 x 132.  References are computed once per process."""
import numpy as np

import analyze_post_cases as post

WIDTHS = (1, 31, 32, 33, 64, 65, 132)
HEIGHTS = (1, 2, 3, 132)

_reference_cache = {}


def reference(mask):
    """(contours as float64 (x, y) arrays, pixels as np.argwhere) by the host statement of make_json_results."""
    from caesar_mrcnn_amd import analyze
    mask = np.asarray(mask)
    key = (mask.shape, mask.dtype.str, mask.tobytes())
    if key not in _reference_cache:
        padded = np.zeros((mask.shape[0] + 2, mask.shape[1] + 2), np.uint8)
        padded[1:-1, 1:-1] = mask
        contours = [np.fliplr(v) - 1 for v in analyze.find_contours(padded, 0.5)]
        _reference_cache[key] = (contours, np.argwhere(mask == 1))
    return _reference_cache[key]


def random_mask(h, w, seed, fill=None):
    rng = np.random.default_rng(seed)
    return (rng.uniform(size=(h, w)) < (rng.uniform(0.1, 0.9) if fill is None else fill)).astype(np.uint8)


def size_grid():
    """[(name, mask)]: every width with every height -- random fill; empty and full at every size."""
    out = []
    for w in WIDTHS:
        for h in HEIGHTS:
            fill = 0.5 if h * w < 2000 else 0.12          # the large frames sparse: the yardstick walks every boundary cell in Python
            out.append(("random_%dx%d" % (h, w), random_mask(h, w, 1000 * h + w, fill)))
            out.append(("empty_%dx%d" % (h, w), np.zeros((h, w), np.uint8)))
            out.append(("full_%dx%d" % (h, w), np.ones((h, w), np.uint8)))
    return out


def _blank(h, w):
    return np.zeros((h, w), np.uint8)


def serpentine(h=64, w=65):
    """A one-pixel-wide path that fills the frame: every other row full, joined alternately at the right and the left end."""
    m = _blank(h, w)
    m[0::2, :] = 1
    for k, y in enumerate(range(1, h, 2)):
        m[y, w - 1 if k % 2 == 0 else 0] = 1
    return m


def loop_of(segments):
    """A 1 x b bar, whose single contour has 2 (1 + b) segments, in a frame with a margin."""
    assert segments % 2 == 0 and segments >= 4
    b = segments // 2 - 1
    m = _blank(3, b + 2)
    m[1, 1:1 + b] = 1
    return m


def bent_loop_of(segments, width=130):
    """A one-pixel-wide serpentine of segments / 2 - 1 pixels (a simple path: one contour of 2 (1 + pixels) segments) that fits
    a frame 132 wide: full rows of `width` pixels joined by single pixels, the last row cut to length."""
    assert segments % 2 == 0 and segments >= 4
    left = segments // 2 - 1
    y, k = 1, 0
    m = _blank(2 * (left // (width + 1) + 2) + 1, width + 2)
    while left > 0:
        take = min(width, left)
        if k % 2 == 0:
            m[y, 1:1 + take] = 1
        else:
            m[y, 1 + width - take:1 + width] = 1
        left -= take
        if left > 0:
            m[y + 1, width if k % 2 == 0 else 1] = 1
            left -= 1
        y += 2
        k += 1
    return m


def shapes():
    """[(name, mask)]: the places where the kernels can go wrong."""
    out = []
    for name, (y, x) in (("tl", (0, 0)), ("tr", (0, 64)), ("bl", (4, 0)), ("br", (4, 64))):
        m = _blank(5, 65)
        m[y, x] = 1
        out.append(("corner_" + name, m))
    # two pixels touching only diagonally; the saddle cell (pixel columns x | x + 1) on a word boundary of the pixel words (31 | 32)
    # and of the cell words (30 | 31), in both orientations
    for x in (31, 30, 63):
        m = _blank(4, 70)
        m[1, x] = m[2, x + 1] = 1
        out.append(("diagonal_down_%d" % x, m))
        m = _blank(4, 70)
        m[1, x + 1] = m[2, x] = 1
        out.append(("diagonal_up_%d" % x, m))
    yy, xx = np.indices((20, 70))
    board = ((yy + xx) % 2 == 0).astype(np.uint8)
    out.append(("checkerboard", board))
    out.append(("checkerboard_odd", 1 - board))
    out.append(("checkerboard_thinned", board & random_mask(20, 70, 5, 0.8)))
    ring = _blank(40, 70)
    ring[3:37, 20:68] = 1
    ring[8:32, 25:60] = 0
    ring[14:20, 30:50] = 1                                # an island inside the hole ...
    ring[16:18, 33:40] = 0                                # ... with a hole of its own
    out.append(("ring_island", ring))
    out.append(("serpentine", serpentine()))
    for k in (4, 6, 8):                                   # contour lengths are even: 2^k - 2, 2^k, 2^k + 2 (see test_outline_gpu.py)
        for s in (2 ** k - 2, 2 ** k, 2 ** k + 2):
            out.append(("loop_%d" % s, loop_of(s)))
    # the kernels' own boundaries: 512 threads per source (the strided loops' second trip), 1536 segments (LDS / global workspace)
    for s in (510, 512, 514, 1534, 1536, 1538):
        out.append(("loop_%d" % s, bent_loop_of(s)))
    dots = _blank(33, 67)
    dots[0::2, 0::2] = 1
    out.append(("isolated_pixels", dots))
    frame_hole = np.ones((9, 66), np.uint8)
    frame_hole[4, 31:33] = 0
    out.append(("full_with_hole", frame_hole))
    return out


def blobs(shape, n, seed):
    """n blob-shaped masks with ragged edges, some with holes: discs of analyze_post_cases with random pixels removed at the rim."""
    rng = np.random.default_rng(seed)
    out = []
    for m, _, _ in post.discs(shape, n, seed, rmin=2, rmax=14):
        m = m.copy()
        rim = m & ~(np.roll(m, 1, 0) & np.roll(m, -1, 0) & np.roll(m, 1, 1) & np.roll(m, -1, 1))
        m &= ~(rim & (rng.uniform(size=shape) < 0.3))
        ys, xs = np.nonzero(m)
        if ys.size > 60:
            k = int(rng.integers(0, ys.size))
            m[ys[k] - 1:ys[k] + 1, xs[k] - 1:xs[k] + 2] = False
        out.append(m.astype(np.uint8))
    return out


def pack_sources(masks, seed=None):
    """(pool uint32 [words], desc int32 [n, 6]) of 2-D 0 / 1 masks, each the bitmap of its own box.  With a seed: nonzero x0 / y0,
    junk words before and between the sources (nonzero word_offset), words_per_row larger than needed, and garbage in every
    padding bit (past w in a row's last word, and the spare words)."""
    rng = np.random.default_rng(seed) if seed is not None else None
    words, desc = [], []
    at = 0
    for m in masks:
        m = np.asarray(m) != 0
        h, w = m.shape
        need = (w + 31) // 32
        wpr = need + (int(rng.integers(0, 3)) if rng is not None else 0)
        if rng is not None:
            lead = int(rng.integers(1, 5))
            words.append(rng.integers(0, 2 ** 32, size=lead, dtype=np.uint64).astype(np.uint32))
            at += lead
        bits = np.zeros((h, wpr * 32), bool) if rng is None else rng.uniform(size=(h, wpr * 32)) < 0.5
        bits[:, :w] = m
        rows = np.packbits(bits, axis=-1, bitorder="little").view("<u4").reshape(-1) if h and wpr else np.zeros(0, np.uint32)
        x0, y0 = (int(rng.integers(-50, 5000)), int(rng.integers(-50, 5000))) if rng is not None else (0, 0)
        desc.append((x0, y0, w, h, at, wpr))
        words.append(rows)
        at += rows.size
    pool = np.concatenate(words) if words else np.zeros(0, np.uint32)
    return np.ascontiguousarray(pool, dtype=np.uint32), np.array(desc, np.int32).reshape(-1, 6)


def assert_outlines(got, masks, tag=""):
    """`got`: the dict of Outlines.host(); masks: the sources' masks in order.  Exact equality with the yardstick."""
    n = len(masks)
    sc, co, po = got["source_contours"], got["contour_offsets"], got["pixel_offsets"]
    pts, pix = got["points"], got["pixels"]
    assert sc.shape == (n + 1,) and po.shape == (n + 1,) and sc[0] == 0 and po[0] == 0, tag
    assert pts.dtype == np.float32 and pix.dtype == np.int32 and co.dtype == np.int32
    assert co.shape == (sc[-1] + 1,) and co[0] == 0 and co[-1] == pts.shape[0] and po[-1] == pix.shape[0], tag
    for i, m in enumerate(masks):
        want_c, want_p = reference(m)
        assert sc[i + 1] - sc[i] == len(want_c), (tag, i, sc[i + 1] - sc[i], len(want_c))
        for k, want in enumerate(want_c):
            have = pts[co[sc[i] + k]:co[sc[i] + k + 1]]
            assert have.shape == want.shape and np.array_equal(have.astype(np.float64), want), (tag, i, k, have, want)
        have = pix[po[i]:po[i + 1]]
        assert have.shape == want_p.shape and np.array_equal(have, want_p), (tag, i)
