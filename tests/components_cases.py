"""Scenes for the connected components of bit planes (csrc/components.hip: ops.mask_components / mask_components_split /
mask_row_extents), shared by tests/test_components_cpu.py and tests/test_components_gpu.py, and the host yardstick they are
compared with: analyze.label_components (4-connected) and, for 8-connected labels, the same breadth-first statement over eight
neighbours (its component COUNT is checked against analyze.count_islands).  Every scene is [n, H, W] bool: the planes of one frame.
All but one are at most 97 x 256; the seeded 512 x 512 plane is the size at which the union-find leaves LDS."""
import functools
from collections import deque

import numpy as np

LDS_RUNS = 12288                 # runs of one box up to which the kernel keeps its parent table in LDS


def label_host(mask, connectivity):
    """(labels int32 [H, W], n): components numbered 1..n in raster order of their first pixel."""
    from caesar_mrcnn_amd import analyze
    m = np.asarray(mask) != 0
    if connectivity == 4:
        lab, n = analyze.label_components(m)
        return np.asarray(lab, np.int32), int(n)
    try:
        from scipy import ndimage
        lab, n = ndimage.label(m, structure=np.ones((3, 3), int))
        return np.asarray(lab, np.int32), int(n)
    except ImportError:
        return label_bfs(m, 8)


def label_bfs(m, connectivity):
    """The breadth-first fallback of analyze.label_components, for either neighbourhood."""
    H, W = m.shape
    lab = np.zeros(m.shape, np.int32)
    n = 0
    near = [(-1, 0), (1, 0), (0, -1), (0, 1)] + ([(-1, -1), (-1, 1), (1, -1), (1, 1)] if connectivity == 8 else [])
    for r, c in zip(*np.nonzero(m)):
        if lab[r, c]:
            continue
        n += 1
        lab[r, c] = n
        q = deque([(r, c)])
        while q:
            y, x = q.popleft()
            for dy, dx in near:
                yy, xx = y + dy, x + dx
                if 0 <= yy < H and 0 <= xx < W and m[yy, xx] and not lab[yy, xx]:
                    lab[yy, xx] = n
                    q.append((yy, xx))
    return lab, n


def boxes_of(planes):
    """utils.extract_bboxes of [n, H, W] planes."""
    from caesar_mrcnn_amd import utils
    return utils.extract_bboxes(np.moveaxis(np.asarray(planes, bool), 0, -1))


def label_boxes(labels, n):
    """(count [n], box [n, 4]) of the components of a label map: popcounts and utils.extract_bboxes of labels == k, k = 1..n."""
    count = np.bincount(labels.ravel(), minlength=n + 1)[1:n + 1].astype(np.int32)
    ys, xs = np.nonzero(labels)
    k = labels[ys, xs] - 1
    box = np.zeros((n, 4), np.int64)
    if n:
        box[:, 0] = box[:, 1] = 1 << 30
        np.minimum.at(box[:, 0], k, ys)
        np.minimum.at(box[:, 1], k, xs)
        np.maximum.at(box[:, 2], k, ys + 1)
        np.maximum.at(box[:, 3], k, xs + 1)
    return count, box.astype(np.int32)


def _spiral(n):
    """A one-pixel-wide square spiral with one-pixel gaps: ONE component whose runs are joined only through long chains."""
    m = np.zeros((n, n), bool)
    y, x, dy, dx = 0, 0, 0, 1
    m[0, 0] = True
    while True:
        for _ in range(2):                                       # straight on, else one turn to the right
            ny, nx, ay, ax = y + dy, x + dx, y + 2 * dy, x + 2 * dx
            if 0 <= ny < n and 0 <= nx < n and not m[ny, nx] and not (0 <= ay < n and 0 <= ax < n and m[ay, ax]):
                y, x = ny, nx
                m[y, x] = True
                break
            dy, dx = dx, -dy
        else:
            return m


def _snake(n):
    """Rows 0, 2, 4, ... full, joined alternately at the right and the left end: one component, a chain through every row."""
    m = np.zeros((n, n), bool)
    m[0::2] = True
    for k, y in enumerate(range(1, n, 2)):
        m[y, n - 1 if k % 2 == 0 else 0] = True
    return m


def _comb(n):
    """Teeth in every other column that meet only in the last row (a "U" many times over)."""
    m = np.zeros((n, n), bool)
    m[:, 0::2] = True
    m[n - 1, :] = True
    return m


def _rings():
    m = np.zeros((21, 37), bool)
    m[1:20, 2:35] = True
    m[3:18, 4:33] = False                # a hole ...
    m[6:15, 8:29] = True                 # ... with an island in it ...
    m[8:13, 11:26] = False               # ... that has a hole ...
    m[10, 30:34] = False
    m[10, 17:20] = True                  # ... with an island of its own
    return m


def _seam():
    """Runs that meet across bits 31 | 32 and 63 | 64 of adjacent words, straight and diagonally."""
    m = np.zeros((6, 70), bool)
    m[0, 28:36] = True                   # one run across the seam
    m[2, 30:32] = True
    m[3, 32:34] = True                   # diagonal contact across the seam: joined under 8 only
    m[2, 60:64] = True
    m[3, 63:66] = True                   # straight contact at x = 63, the run goes on into the next word
    m[5, 0] = m[5, 31] = m[5, 32] = m[5, 63] = m[5, 64] = m[5, 69] = True
    return m


def _numbering():
    """Component 2 starts left of component 1 on a later row, component 3 left of both; and what looks like a fourth component
    from row 3 on (two runs that row 5 joins) turns out to be component 1 on the last row."""
    m = np.zeros((7, 40), bool)
    m[0:7, 10] = True                    # 1 runs down column 10 ...
    m[1, 2] = True                       # 2: further left, but later in raster order
    m[3:5, 20] = m[3:5, 30] = True       # two runs of their own ...
    m[5, 20:31] = True                   # ... joined by row 5 ...
    m[6, 10:21] = True                   # ... and with 1 by the last row
    m[4, 0] = True                       # 3
    return m


def _stripes(rows, extra):
    """128 one-pixel columns over `rows` rows of a 256-wide frame: 128 * rows runs; `extra` adds a row with one pixel in an odd
    column (one run more: 4-connected alone, 8-connected it joins the two stripes beside it)."""
    m = np.zeros((rows + (1 if extra else 0), 256), bool)
    m[:rows, 0::2] = True
    if extra:
        m[rows, 1] = True
    return m


@functools.lru_cache(maxsize=None)
def scenes():
    """[(name, planes [n, H, W] bool)]"""
    out = []
    for H in (1, 2):
        for W in (1, 31, 32, 33, 64, 65):
            rng = np.random.default_rng(100 * H + W)
            p = rng.uniform(size=(3, H, W)) < 0.6
            p[1] = True
            p[2, :, 0] = p[2, :, W - 1] = True
            out.append(("w%d_h%d" % (W, H), p))
    out.append(("seam", _seam()[None]))
    diag = np.zeros((2, 2), bool)
    diag[0, 0] = diag[1, 1] = True
    out.append(("diagonal", diag[None]))
    yy, xx = np.mgrid[0:33, 0:33]
    out.append(("checkerboard_33", ((yy + xx) % 2 == 0)[None]))
    out.append(("spiral_comb_40", np.stack([_spiral(40), _comb(40), _snake(40), ~_spiral(40), _comb(40)[::-1]])))
    out.append(("rings", _rings()[None]))
    out.append(("numbering", _numbering()[None]))
    rng = np.random.default_rng(7)
    some = rng.uniform(size=(2, 19, 45)) < 0.45
    out.append(("full_and_empty", np.stack([some[0], np.ones((19, 45), bool), np.zeros((19, 45), bool), some[1]])))
    rng = np.random.default_rng(11)
    mixed = np.zeros((9, 70, 67), bool)
    mixed[0] = rng.uniform(size=(70, 67)) < 0.5
    mixed[1] = rng.uniform(size=(70, 67)) < 0.1
    mixed[2] = mixed[0]                                  # a duplicate
    mixed[3, 20:50, 30:66] = rng.uniform(size=(30, 36)) < 0.7
    mixed[4] = rng.uniform(size=(70, 67)) < 0.9
    mixed[5, 69, 66] = True                              # one pixel in the last corner
    mixed[6] = mixed[3]
    mixed[7, :, 31:33] = True                            # a bar on the word seam
    mixed[8] = ~mixed[4]
    out.append(("mixed_70x67", mixed))
    out.append(("stripes_%d" % LDS_RUNS, _stripes(96, False)[None]))             # the last size with the table in LDS ...
    out.append(("stripes_%d" % (LDS_RUNS + 1), _stripes(96, True)[None]))        # ... and the first with it in the workspace
    rng = np.random.default_rng(2026)
    out.append(("random_512", (rng.uniform(size=(1, 512, 512)) < 0.5)))
    return out


def scene(name):
    return dict(scenes())[name]


@functools.lru_cache(maxsize=None)
def reference(name, connectivity):
    """[(labels, n)] per plane of the scene, computed once and shared: not to be written."""
    return [label_host(p, connectivity) for p in scene(name)]
