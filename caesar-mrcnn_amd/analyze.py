"""Post-processing of ``MaskRCNN.detect`` results into the user-visible artefacts (row f3 of the scope
table): score filter, optional splitting of non-connected masks, merging of connected same-class masks,
selection of the best mask among overlapping ones, JSON and DS9-region output.  Restates
``Analyzer.predict / extract_det_masks / make_json_results / make_ds9_regions`` of mrcnn/analyze.py
(:833-905, :1162-1496, :1866-2030) and mrcnn/graph.py.  Host-side NumPy, except the mask graph of
``extract_det_masks`` -- which masks overlap or touch, and the unions of the merged ones.  Its decisions are written
once (``Analyzer._extract_det_masks``: score filter, graph searches, clique walk, captions) against a mask set with two
implementations behind ``Analyzer.postprocess_device``:

  * ``extract_det_masks_host``    ``_FrameMasks``, the literal statement: ``mask_iou`` and ``are_mask_connected`` (three
                                  labellings) on full frames, pair by pair as the decisions ask for them -- the
                                  CPU-testable statement and the yardstick of the kernels;
  * ``extract_det_masks_device``  ``_PlaneMasks``: the same answers from three launches on bit planes (csrc/maskgraph.hip:
                                  ops.mask_planes_pack / mask_pair_stats / mask_union).

Every device form here and in sfinder.py runs under one policy (``device_or_host``: a form that raised is logged once and
stays off for the process) on one device resolution (``model_device`` / ``model_has_gpu``).

The tester -- ``ModelTester`` and ``Analyzer.inspect_results`` (``get_data``, ``extract_gt_masks``, ``compute_det_mask_pars``,
``compute_performances``; analyze.py:65-406, :715-828, :907-1157, :1502-1861) -- is restated rule for rule as well: true and
detected objects matched by mask IoU, confusion matrix and purity, one table row per true and per detected object.  Its pixel
work, the mask IoU of every (true object, detection) pair and the flux sum under every detection mask, has two implementations
behind ``Analyzer.eval_device``: ``mask_iou`` / ``np.nansum`` on full frames, or one launch each on bit planes
(csrc/maskeval.hip: ops.mask_cross_stats / mask_plane_sums); the matching loops are the same code for both.

Connected components -- the pieces of ``split_masks``, the true masks of ``split_gtmasks``, the islands and hull points of
``compute_det_mask_pars`` -- come from the same planes behind ``Analyzer.components_device`` (csrc/components.hip:
ops.mask_components / mask_components_split / mask_row_extents), else from ``label_components`` / ``count_islands`` /
``row_extreme_points`` on full frames.

Third-party pieces the reference imports and this file restates (absent here, so parity is UNPINNED for
them; the semantics are the published ones):
  * skimage.measure.label(connectivity=1)      -> ``label_components`` (4-connected, raster-order numbering)
  * skimage.measure.find_contours(level=0.5)   -> ``find_contours`` (marching squares, 'low' connectivity)
  * sklearn.metrics.jaccard_score(binary)      -> ``mask_iou``
  * networkx.find_cliques                      -> ``maximal_cliques`` (Bron-Kerbosch with pivoting)
  * regions (DS9 writer)                       -> plain-text DS9 ``polygon`` / ``box`` lines, image coordinates
  * cv.findContours + cv.minAreaRect / boundingRect -> ``min_area_rect`` (hull + calipers), ``utils.extract_bboxes``
  * skimage.measure.label + regionprops (count)   -> ``count_islands`` (8-connected)
"""
import collections
import csv
import functools
import json
import logging
import math
import os
import time
from collections import deque

import numpy as np

from . import draw as overlay
from . import utils

logger = logging.getLogger("mrcnn")

NO_SPLIT_CLASSES = ('galaxy_C2', 'galaxy_C3', 'galaxy', 'extended-multisland')      # analyze.py:1221

NO_SPLIT_CLASSES_GT = ('galaxy_C2', 'galaxy_C3', 'galaxy', 'extended', 'extended-multisland')      # analyze.py:1065

SPLIT_DTYPE = np.where(np.zeros(1, bool), [1], [0]).dtype      # of a piece of split_masks as the host statement makes it


# ---- where the pixel work runs: one device resolution, one failure policy, one plane eligibility --------------------
def model_device(model):
    """The device the model's engine runs on, else torch's current CUDA device (a stand-in model has no engine)."""
    dev = getattr(getattr(model, "engine", None), "dev", None)
    if dev is not None:
        return dev
    import torch
    return torch.device("cuda", torch.cuda.current_device())


def model_has_gpu(model):
    dev = getattr(getattr(model, "engine", None), "dev", None)
    if dev is not None:
        return getattr(dev, "type", "") == "cuda"
    try:
        import torch
        return bool(torch.cuda.is_available())
    except Exception:
        return False


device_forms_failed = set()             # names of the device forms that raised once: this process stays on their host statements


def device_or_host(name, device_form, host_form, refusal=None):
    """``device_form()``, or ``host_form()`` once the form called `name` has failed in this process.  A _hip.HipPathError or an
    OSError (no library) is such a failure: logged once, at ERROR, and remembered in ``device_forms_failed``.  An exception of the
    type `refusal` is no failure: the device form declines this call only, and the next call tries it again.  Whether a call is
    for the device at all (switch, size, a GPU, masks that fit planes) is the caller's business."""
    if name in device_forms_failed:
        return host_form()
    from . import _hip
    try:
        return device_form()
    except (_hip.HipPathError, OSError) as e:
        if refusal is not None and isinstance(e, refusal):
            logger.debug("%s: the host statement takes this call" % e)
        else:
            device_forms_failed.add(name)
            logger.error("%s failed (%s: %s): this and every later call take the host statement ..." % (name, type(e).__name__, e))
    return host_form()


def masks_fit_planes(masks, binary):
    """Can these [H, W] masks become the bit planes of one frame: 2-D, not empty, of one shape, bool or integer.  Planes are made
    with `!= 0`, as mask_iou reads a mask, so the tester's steps (binary=False) take any values.  Whatever hands the masks or their
    values on (binary=True) needs 0 / 1: a lone mask keeps its own values, and make_json_results takes `== 1` for the pixels but
    `> 0.5` for the contours."""
    shape = None
    for m in masks:
        m = np.asarray(m)
        if m.ndim != 2 or m.size == 0 or m.dtype.kind not in "biu" or (shape is not None and m.shape != shape):
            return False
        shape = m.shape
        if binary and m.dtype != np.bool_ and not (int(m.min()) >= 0 and int(m.max()) <= 1):
            return False
    return shape is not None


# ---- restated third-party helpers -----------------------------------------------------------------------
def label_components(mask):
    """4-connected components of a binary mask, numbered 1..n in raster order of their first pixel."""
    m = np.asarray(mask) != 0
    try:
        from scipy import ndimage
        lab, n = ndimage.label(m)
        return lab, int(n)
    except ImportError:
        lab = np.zeros(m.shape, np.int32)
        n = 0
        H, W = m.shape
        for r, c in zip(*np.nonzero(m)):
            if lab[r, c]:
                continue
            n += 1
            lab[r, c] = n
            q = deque([(r, c)])
            while q:
                y, x = q.popleft()
                for yy, xx in ((y - 1, x), (y + 1, x), (y, x - 1), (y, x + 1)):
                    if 0 <= yy < H and 0 <= xx < W and m[yy, xx] and not lab[yy, xx]:
                        lab[yy, xx] = n
                        q.append((yy, xx))
        return lab, n


def mask_iou(a, b):
    a, b = np.asarray(a).astype(bool).ravel(), np.asarray(b).astype(bool).ravel()
    union = np.logical_or(a, b).sum()
    return float(np.logical_and(a, b).sum()) / float(union) if union else 0.0


def masks_touch4(mask1, mask2):
    """True iff some pixel of mask1 equals, or is a 4-neighbour (up, down, left, right) of, some pixel of mask2.  This IS
    ``Analyzer.are_mask_connected``: the 4-connected components of mask1 | mask2 are the connected components of the bipartite
    "touches" graph between the components of mask1 and those of mask2, so their number drops below n1 + n2 exactly when that
    graph has an edge -- no labelling needed.  Diagonal contact alone is no edge.  csrc/maskgraph.hip computes this on bit
    planes."""
    a, b = np.asarray(mask1) != 0, np.asarray(mask2) != 0
    d = b.copy()
    d[1:] |= b[:-1]
    d[:-1] |= b[1:]
    d[:, 1:] |= b[:, :-1]
    d[:, :-1] |= b[:, 1:]
    return bool((a & d).any())


def pack_mask_planes(masks):
    """[H, W, n] masks (nonzero = set) -> bit planes [n, H, ceil(W / 32)] uint32: pixel x is bit x & 31 of word x >> 5, least
    significant bit first; the bits past W are zero.  The NumPy statement of ops.mask_planes_pack's layout."""
    m = np.moveaxis(np.asarray(masks) != 0, -1, 0)
    n, H, W = m.shape
    wpr = (W + 31) // 32
    padded = np.zeros((n, H, wpr * 32), bool)
    padded[:, :, :W] = m
    return np.ascontiguousarray(np.packbits(padded, axis=-1, bitorder="little")).view("<u4").reshape(n, H, wpr)


def unpack_mask_planes(words, W):
    """Bit planes [n, H, wpr] (32-bit words) -> [n, H, W] uint8 of 0 / 1."""
    w = np.ascontiguousarray(words).view("<u4")
    n, H, wpr = w.shape
    return np.unpackbits(w.view(np.uint8).reshape(n, H, wpr * 4), axis=-1, bitorder="little")[:, :, :W]


def find_contours(arr, level=0.5):
    """Iso-contours of a 2-D array by marching squares: list of [n, 2] (row, col) arrays, closed contours
    repeat their first point.  Squares are visited in raster order; segments keep the higher values on
    their left; ambiguous saddles connect the low corners (skimage default ``fully_connected='low'``)."""
    a = np.asarray(arr, dtype=np.float64)
    H, W = a.shape
    segs = []

    def frac(v0, v1):
        return (level - v0) / (v1 - v0)

    hi = a > level
    case = (hi[:-1, :-1] * 1 + hi[:-1, 1:] * 2 + hi[1:, :-1] * 4 + hi[1:, 1:] * 8)
    for r, c in zip(*np.nonzero((case != 0) & (case != 15))):
        ul, ur, ll, lr = a[r, c], a[r, c + 1], a[r + 1, c], a[r + 1, c + 1]
        k = case[r, c]
        top = (float(r), c + frac(ul, ur)) if (k & 1) != ((k >> 1) & 1) else None
        bottom = (r + 1.0, c + frac(ll, lr)) if ((k >> 2) & 1) != ((k >> 3) & 1) else None
        left = (r + frac(ul, ll), float(c)) if (k & 1) != ((k >> 2) & 1) else None
        right = (r + frac(ur, lr), c + 1.0) if ((k >> 1) & 1) != ((k >> 3) & 1) else None
        table = {1: [(top, left)], 2: [(right, top)], 3: [(right, left)], 4: [(left, bottom)], 5: [(top, bottom)],
                 6: [(right, top), (left, bottom)], 7: [(right, bottom)], 8: [(bottom, right)],
                 9: [(top, left), (bottom, right)], 10: [(bottom, top)], 11: [(bottom, left)], 12: [(left, right)],
                 13: [(top, right)], 14: [(left, top)]}
        segs.extend(table[int(k)])

    contours, starts, ends, nxt = {}, {}, {}, 0
    for p, q in segs:
        if p == q:
            continue
        tail, tail_num = starts.pop(q, (None, None))
        head, head_num = ends.pop(p, (None, None))
        if tail is not None and head is not None:
            if tail is head:
                head.append(q)                                  # closes the contour
            elif tail_num > head_num:
                head.extend(tail)
                contours.pop(tail_num, None)
                starts[head[0]] = (head, head_num)
                ends[head[-1]] = (head, head_num)
            else:
                tail.extendleft(reversed(head))
                contours.pop(head_num, None)
                starts[tail[0]] = (tail, tail_num)
                ends[tail[-1]] = (tail, tail_num)
        elif tail is None and head is None:
            new = deque((p, q))
            contours[nxt] = new
            starts[p] = (new, nxt)
            ends[q] = (new, nxt)
            nxt += 1
        elif head is None:
            tail.appendleft(p)
            starts[p] = (tail, tail_num)
        else:
            head.append(q)
            ends[q] = (head, head_num)
    return [np.array(c) for _, c in sorted(contours.items())]


# Marching-squares edges of a cell: top, left, bottom, right.  Start (p) and end (q) edge of the first segment of every case of the
# table in find_contours; a saddle's second segment runs left -> bottom (case 6) or bottom -> right (case 9).
_EDGE_T, _EDGE_L, _EDGE_B, _EDGE_R = 0, 1, 2, 3
_SEG_P = np.array([0, 0, 3, 3, 1, 0, 3, 3, 2, 0, 2, 2, 1, 0, 1, 0])
_SEG_Q = np.array([0, 1, 0, 1, 2, 2, 0, 2, 3, 1, 0, 1, 3, 3, 0, 0])
_EDGE_DX2 = np.array([-1, -2, -1, 0])        # twice the offset of an edge's midpoint from (c, r), mask coordinates
_EDGE_DY2 = np.array([-2, -1, 0, -1])


def outline_statement(mask):
    """(contours, pixels) of ONE 2-D mask of 0 / 1: what ``make_json_results`` takes from ``find_contours`` on the zero-padded
    mask and from ``np.argwhere``, stated without the sequential stitching -- the definition of csrc/outline.hip's results.
    contours: list of float64 [L + 1, 2] arrays of (x, y), pixel centres at integers, in find_contours' order and starting
    point; pixels: int64 [K, 2] of (y, x) in raster order.

      1. cells (r, c) of the padded mask in raster order, corners mask[r - 1 .. r, c - 1 .. c]; a cell's segments in the order of
         find_contours' table (a saddle has two): segment k of cell (r, c) has index 2 * (r * cols + c) + k;
      2. every crossing point lies on one grid edge shared by two cells, so it ends one segment and starts one: succ(s) is the
         segment that starts where s ends, and on a padded mask every contour is a cycle of succ;
      3. contours are ordered by the smallest index of their cycle;
      4. with `last` the largest index of the cycle, the contour is p(succ(last)), p(succ^2(last)), ..., p(last), q(last);
      5. level 0.5 between 0 and 1 puts every crossing at an edge's midpoint: coordinates are multiples of 0.5, exact.
    Not a fast path: the cycles are walked in Python."""
    m = np.asarray(mask)
    if m.ndim != 2:
        raise ValueError("outline_statement: one 2-D mask, got shape %r" % (m.shape,))
    h, w = m.shape
    pixels = np.argwhere(m == 1)
    hi = np.zeros((h + 2, w + 2), bool)
    hi[1:-1, 1:-1] = m > 0.5
    case = hi[:-1, :-1] * 1 + hi[:-1, 1:] * 2 + hi[1:, :-1] * 4 + hi[1:, 1:] * 8
    rr, cc = np.nonzero((case != 0) & (case != 15))
    kk = case[rr, cc]
    cell = np.repeat(np.arange(rr.size), 1 + ((kk == 6) | (kk == 9)))         # rule 1: raster order, saddles twice
    second = np.zeros(cell.size, bool)
    second[1:] = cell[1:] == cell[:-1]
    r, c, k = rr[cell], cc[cell], kk[cell]
    pe = np.where(second, np.where(k == 6, _EDGE_L, _EDGE_B), _SEG_P[k])
    qe = np.where(second, np.where(k == 6, _EDGE_B, _EDGE_R), _SEG_Q[k])
    px2, py2 = 2 * c + _EDGE_DX2[pe], 2 * r + _EDGE_DY2[pe]                      # rule 5: doubled coordinates are integers
    qx2, qy2 = 2 * c + _EDGE_DX2[qe], 2 * r + _EDGE_DY2[qe]
    pkey, qkey = (py2 + 2) * (2 * w + 4) + px2 + 2, (qy2 + 2) * (2 * w + 4) + qx2 + 2
    by_p = np.argsort(pkey)
    succ = by_p[np.searchsorted(pkey[by_p], qkey)] if cell.size else by_p      # rule 2
    contours, seen = [], np.zeros(cell.size, bool)
    for first in range(cell.size):                                             # rule 3: a cycle is met at its smallest index
        if seen[first]:
            continue
        cycle, s = [first], int(succ[first])
        while s != first:
            cycle.append(s)
            s = int(succ[s])
        cycle = np.array(cycle)
        seen[cycle] = True
        at = int(np.argmax(cycle))                                             # rule 4
        walk = np.roll(cycle, -(at + 1))                                       # succ(last), ..., last
        x2 = np.append(px2[walk], qx2[walk[-1]])
        y2 = np.append(py2[walk], qy2[walk[-1]])
        contours.append(np.stack([x2, y2], axis=1) / 2.0)
    return contours, pixels


def maximal_cliques(adj):
    """All maximal cliques of an undirected graph {node: set(neighbours)} (nodes without edges are absent,
    as in a networkx graph built with add_edge only)."""
    out = []

    def expand(R, P, X):
        if not P and not X:
            out.append(sorted(R))
            return
        pivot = max(P | X, key=lambda u: len(adj[u] & P))
        for v in sorted(P - adj[pivot]):
            expand(R | {v}, P & adj[v], X & adj[v])
            P = P - {v}
            X = X | {v}

    if adj:
        expand(set(), set(adj), set())
    return out


def connected_components(n, edges):
    """mrcnn/graph.py: depth-first components in vertex order, neighbours in insertion order."""
    adj = [[] for _ in range(n)]
    for v, w in edges:
        adj[v].append(w)
        adj[w].append(v)
    seen, cc = [False] * n, []
    for v in range(n):
        if seen[v]:
            continue
        comp = []
        # recursive DFS order of the reference: visit v, then each unvisited neighbour in turn
        def dfs(u):
            seen[u] = True
            comp.append(u)
            for w in adj[u]:
                if not seen[w]:
                    dfs(w)
        dfs(v)
        cc.append(comp)
    return cc


def convex_hull(points):
    """Convex hull of integer points [n, 2] (x, y) by the monotone chain, counter-clockwise in (x, y) axes, collinear points
    dropped; one or two points when the set is one point or lies on one line."""
    pts = sorted(set((int(x), int(y)) for x, y in points))
    if len(pts) <= 2:
        return np.array(pts, dtype=np.float64).reshape(-1, 2)

    def half(seq):
        h = []
        for p in seq:
            while len(h) >= 2 and (h[-1][0] - h[-2][0]) * (p[1] - h[-2][1]) - (h[-1][1] - h[-2][1]) * (p[0] - h[-2][0]) <= 0:
                h.pop()
            h.append(p)
        return h
    lower, upper = half(pts), half(pts[::-1])
    return np.array(lower[:-1] + upper[:-1], dtype=np.float64).reshape(-1, 2)


def row_extreme_points(mask):
    """[2 R, 2] integer points (x, y): the leftmost set pixel of each of the R rows that have one, then the rightmost of each; None
    for an empty mask.  They suffice for the hull of the mask's pixels.  ops.mask_row_extents gives the same columns from bit
    planes (``row_extents_points``)."""
    m = np.asarray(mask) != 0
    ys, xs = np.nonzero(m)
    if ys.size == 0:
        return None
    starts = np.flatnonzero(np.r_[True, ys[1:] != ys[:-1]])         # np.nonzero lists the pixels row by row
    ends = np.r_[starts[1:], ys.size] - 1
    return np.concatenate([np.stack([xs[starts], ys[starts]], 1), np.stack([xs[ends], ys[ends]], 1)])


def row_extents_points(extents, y1):
    """row_extreme_points from the [rows, 2] (leftmost, rightmost) table of ops.mask_row_extents for a box that starts at row y1."""
    extents = np.asarray(extents).reshape(-1, 2)
    rows = np.flatnonzero(extents[:, 0] >= 0)
    if rows.size == 0:
        return None
    ys = rows + int(y1)
    return np.concatenate([np.stack([extents[rows, 0], ys], 1), np.stack([extents[rows, 1], ys], 1)]).astype(np.int64)


def min_area_rect(mask):
    """``min_area_rect_of_points`` of the mask's ``row_extreme_points``; None for an empty mask."""
    points = row_extreme_points(mask)
    return None if points is None else min_area_rect_of_points(points)


def min_area_rect_of_points(points):
    """((cx, cy), (w, h), angle) of the minimum-area enclosing rectangle of a mask's set pixels, given as integer points (x, y)
    that hold the hull's vertices (``row_extreme_points``), in coordinate measure (a single
    pixel is 0 x 0, an a x b block is (a - 1) x (b - 1)).  Stands for cv.findContours(RETR_EXTERNAL,
    CHAIN_APPROX_SIMPLE) followed by cv.minAreaRect on the merged contours (analyze.py:1562-1617), UNPINNED: that is the rectangle
    of the convex hull of the pixels' integer coordinates -- the outer contours hold every hull vertex, holes and collinear
    points never reach the hull.  Rotating calipers in float64: a minimum-area rectangle has a side along a hull edge, so for
    every edge the hull's extent along and across it is taken and the first smallest area kept.  The angle follows OpenCV >= 4.5.1:
    in (0, 90], the rotation of the side reported as the width from the x axis; nothing reads it."""
    hull = convex_hull(points)
    if len(hull) == 1:
        return (float(hull[0, 0]), float(hull[0, 1])), (0.0, 0.0), 90.0
    best = None
    for k in range(len(hull) if len(hull) > 2 else 1):
        e = hull[(k + 1) % len(hull)] - hull[k]
        u = e / math.hypot(e[0], e[1])
        along, across = hull @ u, hull @ np.array([-u[1], u[0]])
        w, h = float(along.max() - along.min()), float(across.max() - across.min())
        if best is None or w * h < best[0]:
            ca, cc = 0.5 * (along.max() + along.min()), 0.5 * (across.max() + across.min())
            best = (w * h, (float(ca * u[0] - cc * u[1]), float(ca * u[1] + cc * u[0])), w, h, math.degrees(math.atan2(u[1], u[0])))
    _, centre, w, h, angle = best
    angle %= 180.0                                   # a side's direction has no sign ...
    if angle > 90.0:                                 # ... and the other side's direction is 90 degrees off: swap the sides
        angle, w, h = angle - 90.0, h, w
    elif angle == 0.0:
        angle, w, h = 90.0, h, w
    return centre, (w, h), angle


def count_islands(bmap):
    """Number of 8-connected components of a binary map: len(regionprops(skimage.measure.label(bmap))) (analyze.py:1567-1572;
    label's default connectivity is the array's rank), UNPINNED.  Counted on the crop to the map's bounding box."""
    m = np.asarray(bmap) != 0
    ys, xs = np.nonzero(m)
    if ys.size == 0:
        return 0
    m = m[ys.min():ys.max() + 1, xs.min():xs.max() + 1]
    try:
        from scipy import ndimage
        return int(ndimage.label(m, structure=np.ones((3, 3), int))[1])
    except ImportError:
        seen = np.zeros(m.shape, bool)
        H, W = m.shape
        n = 0
        for r, c in zip(*np.nonzero(m)):
            if seen[r, c]:
                continue
            n += 1
            seen[r, c] = True
            q = deque([(r, c)])
            while q:
                y, x = q.popleft()
                for yy in range(max(y - 1, 0), min(y + 2, H)):
                    for xx in range(max(x - 1, 0), min(x + 2, W)):
                        if m[yy, xx] and not seen[yy, xx]:
                            seen[yy, xx] = True
                            q.append((yy, xx))
        return n


# ---- the two mask sets of Analyzer._extract_det_masks -----------------------------------------------------------
# What the decision body asks of either: pair_stats(ii, jj) -> (iou, connected), indexable by the pair's position; union(comps)
# -> the set of the merged masks; box(k) -> (y1, x1, y2, x2) as utils.extract_bboxes; final(keep) -> the arrays of masks_final;
# sync() at a phase's end.  box and final are asked of a union.
@functools.lru_cache(maxsize=256)
def _pairs_below(n):
    """All (i, j), i < j < n, in the order of the reference's double loop, as two index arrays (shared: not to be written)."""
    return np.triu_indices(n, 1)


class _OnDemand(object):
    def __init__(self, answer):
        self.answer = answer

    def __getitem__(self, k):
        return self.answer(k)


class _FrameMasks(object):
    """Full-frame arrays, the reference's statement.  Nothing is computed before it is asked for, so the body's short-circuits
    decide how many mask_iou and are_mask_connected calls (three labellings each) a frame costs."""

    def __init__(self, an, masks):
        self.an, self.masks = an, masks

    def sync(self):
        pass

    def pair_stats(self, ii, jj):
        m, ii, jj = self.masks, ii.tolist(), jj.tolist()
        return (_OnDemand(lambda k: mask_iou(m[ii[k]], m[jj[k]])), _OnDemand(lambda k: self.an.are_mask_connected(m[ii[k]], m[jj[k]])))

    def union(self, comps):
        out = []
        for comp in comps:
            merged = self.masks[comp[0]]                          # a lone mask stays the array it came as
            for index in comp[1:]:
                merged = self.an.merge_masks(merged, self.masks[index])
            out.append(merged)
        return _FrameMasks(self.an, out)

    def box(self, k):
        return utils.extract_bboxes(np.asarray(self.masks[k]).astype(bool)[:, :, None])[0]

    def final(self, keep):
        return [self.masks[k] for k in keep]


class _PlaneMasks(object):
    """Bit planes on the device (ops.MaskPlanes): mask k is plane index[k]; dtypes[k] lists the dtypes of the host statement's
    arrays that went into it.  A whole pair list is answered by one ops.mask_pair_stats launch and one download (which brings
    the planes' counts and boxes along), a union is one ops.mask_union launch, and only the kept planes are downloaded."""

    def __init__(self, an, planes, index, dtypes):
        self.an, self.planes, self.index, self.dtypes = an, planes, np.asarray(index, dtype=np.int32), dtypes
        self.boxes = None

    def sync(self):
        if self.an.postprocess_sync_timing:
            import torch
            torch.cuda.synchronize()

    def pair_stats(self, ii, jj):
        import torch
        from . import ops
        pi, pj = self.index[ii], self.index[jj]
        inter, touch = ops.mask_pair_stats(self.planes, np.stack([pi, pj], axis=1))
        got = torch.cat([inter, touch, self.planes.count, self.planes.box.reshape(-1)]).cpu().numpy().astype(np.int64)
        P, n = ii.size, self.planes.n
        n_inter, count, self.boxes = got[:P], got[2 * P:2 * P + n], got[2 * P + n:].reshape(n, 4)
        union = count[pi] + count[pj] - n_inter
        iou = n_inter / np.maximum(union, 1)                     # mask_iou: float(inter) / float(union), 0.0 for two empty masks
        return iou.tolist(), got[P:2 * P].tolist()

    def union(self, comps):
        from . import ops
        comp_offsets = np.concatenate([[0], np.cumsum([len(comp) for comp in comps])])
        merged = ops.mask_union(self.planes, comp_offsets, self.index[[k for comp in comps for k in comp]])
        return _PlaneMasks(self.an, merged, range(len(comps)), [[d for k in comp for d in self.dtypes[k]] for comp in comps])

    def box(self, k):
        if self.boxes is None:
            self.boxes = self.planes.box.cpu().numpy()
        return self.boxes[k].astype(np.int32)

    def final(self, keep):
        import torch
        from . import ops
        if not keep:
            return []
        p = self.planes
        if len(keep) != p.n:
            ids = torch.as_tensor(keep, device=p.words.device)
            p = ops.MaskPlanes(p.words.index_select(0, ids), p.count.index_select(0, ids), p.box.index_select(0, ids), p.W)
        unpacked = unpack_mask_planes(p.words.cpu().numpy(), p.W)
        # a lone mask keeps its dtype, a merged one has the NumPy result type of mask1 + mask2 over its members
        arrays = [unpacked[k].astype(np.result_type(*self.dtypes[index])) for k, index in enumerate(keep)]
        self.an._final_planes = (p, arrays)                       # make_json_results, draw_results and the tester work on these
        return arrays


# ---- the Analyzer ------------------------------------------------------------------------------------------
class Analyzer(object):
    """Same attribute names and defaults as the reference's Analyzer (analyze.py:560-712) for the
    ``predict`` path."""

    # Fewer detections than this are post-processed on the host even with postprocess_device on: the break-even of
    # tools/analyze_bench.py, once its table has been taken on an MI355X host; 0 = no such size.
    POSTPROCESS_DEVICE_MIN_MASKS = 0

    # The tester's pixel work (compute_performances, compute_det_mask_pars) runs on the device from this many (true object,
    # detection) pairs per image on: the smallest G * D at which tools/tester_bench.py measured the device path ahead of the host
    # statement on an MI355X host.  None = no such run is recorded: the device path stays off by default.
    EVAL_DEVICE_MIN_PAIRS = 9

    # The contours and pixel lists of make_json_results on the device (csrc/outline.hip): off by default.  With the switch on,
    # frames with fewer final masks than RESULTS_DEVICE_MIN_MASKS stay on the host statement: the smallest count at which
    # tools/outline_bench.py measured the device form ahead on an MI355X host (profiles/outline_bench.json).
    RESULTS_DEVICE = False
    RESULTS_DEVICE_MIN_MASKS = 1

    # The overlay of draw_results is rendered on the GPU (csrc/draw.hip) wherever one is there; frames with fewer final masks than
    # this stay on the host statement.  0 = the device takes every frame: tools/draw_bench.py found no mask count at which the
    # host statement is ahead on an MI355X host (profiles/draw_bench.json).
    DRAW_DEVICE_MIN_MASKS = 0

    # Connected components on the GPU (csrc/components.hip): the pieces of split_masks (with postprocess_device), the true masks of
    # split_gtmasks, and the island count and hull points of compute_det_mask_pars (where its device path runs anyway).  Off by
    # default; tools/components_bench.py times it against the host statement (profiles/components_bench.json).
    COMPONENTS_DEVICE = False

    def __init__(self, model, config, dataset=None, gt_data=None, pred_data=None):
        # Off by default: the device path is equal to the host statement value for value (tests/test_analyze_post_gpu.py) but
        # has not been timed against it on an MI355X host yet, and a frame with one to three detections costs the host
        # statement almost nothing.  `postprocess_device = Analyzer.has_gpu(model)` turns it on wherever a GPU is there.
        self.postprocess_device = False
        self.postprocess_device_min_masks = self.POSTPROCESS_DEVICE_MIN_MASKS
        self.postprocess_sync_timing = False     # synchronise after every device phase, so that postprocess_timing splits them
        self.postprocess_timing = {}
        self.results_device = self.RESULTS_DEVICE
        self.results_device_min_masks = self.RESULTS_DEVICE_MIN_MASKS
        self.results_timing = {}
        self.components_device = self.COMPONENTS_DEVICE
        self.components_timing = {}
        # The device tensor behind self.masks, when the model kept it, and the host array it mirrors (both set by predict).
        # The device path uses the tensor only while self.masks IS that array: masks assigned by hand are uploaded.
        self.masks_device = None
        self.masks_device_host = None
        self.model = model
        self.config = config
        self.dataset = dataset
        self.r = None
        self.n_classes = dataset.nclasses if dataset else config.NUM_CLASSES          # analyze.py:592-595
        self.class_names = config.CLASS_NAMES
        self.image = None
        self.image_shape = None              # set by accept_detection: all that is known of an image that stayed on the device
        self.image_id = -1
        self.image_header = None
        self.image_uuid = ''
        self.image_path = self.image_path_base = self.image_path_base_noext = ''
        self.image_metadata = {}
        self.image_xmin = 0
        self.image_ymin = 0
        self.masks = self.boxes = self.class_ids = self.scores = None
        self.nobjects = 0
        self.masks_final, self.class_ids_final, self.class_names_final, self.scores_final = [], [], [], []
        self.bboxes, self.captions, self.bboxes_gt = [], [], []
        # processed ground truth (analyze.py:617-624)
        self.class_names_gt = None
        self.masks_gt_merged, self.class_ids_gt_merged, self.captions_gt = [], [], []
        self.split_gtmasks = False
        self.sidelobes_mixed_or_near_gt_merged = []
        self.remap_classids = False
        self.classid_map = {}
        self.det_obj_pars = []
        self.split_masks = False
        self.merge_overlapped_masks = True
        self.select_best_overlapped_masks = True
        self.split_source_sidelobe = True
        self.merge_overlap_iou_thr = 0.3
        self.results = {}
        self.obj_name_tag = ""
        self.obj_regions = []
        self.score_thr = 0.7
        self.iou_thr = 0.6
        # performance results (analyze.py:651-661)
        self.detobj_scores, self.detobj_ious, self.detobj_gtinfo = [], [], []
        self.confusion_matrix = np.zeros((self.n_classes, self.n_classes))
        self.confusion_matrix_norm = np.zeros((self.n_classes, self.n_classes))
        self.purity = np.zeros((1, self.n_classes))
        self.nobjs_true = np.zeros((1, self.n_classes))
        self.nobjs_det = np.zeros((1, self.n_classes))
        self.nobjs_det_right = np.zeros((1, self.n_classes))
        self.is_gt_obj_detected = []
        # data for external metric tools (analyze.py:711-713): lists the caller owns, one entry appended per inspected image
        self.gt_data = gt_data
        self.pred_data = pred_data
        # The tester's device path (compute_performances_device / compute_det_mask_pars_device): on where a GPU is there AND a
        # break-even has been measured (EVAL_DEVICE_MIN_PAIRS), from that many pairs on; else the host statement.
        self.eval_device = self.EVAL_DEVICE_MIN_PAIRS is not None and Analyzer.has_gpu(model)
        self.eval_device_min_pairs = self.EVAL_DEVICE_MIN_PAIRS or 0
        self.eval_timing = {}
        self._final_planes = None            # (MaskPlanes of masks_final, that list) when extract_det_masks_device made them
        self._eval_planes = {}
        self.outfile = self.outfile_json = self.outfile_ds9 = ""
        # The overlay PNG (draw_results).  `draw` is OFF by default -- the reference's is on (analyze.py:667) -- so
        # that every command writes what it wrote before the overlay existed.
        self.draw = False
        self.draw_shaded_masks = False
        self.draw_class_label_in_caption = False
        self.draw_scale = None               # canvas pixels per frame pixel, an integer >= 1; None: max(1, 1024 // (max(H, W) + 4))
        self.draw_device_min_masks = self.DRAW_DEVICE_MIN_MASKS
        self.draw_timing = {}
        self.class_color_map = dict(overlay.CLASS_COLOR_MAP)           # analyze.py:683-690 plus the names of class_color_map_ds9
        self.write_to_json = True
        self.write_to_ds9 = True
        self.use_polygon_regions = True
        self.class_color_map_ds9 = {'bkg': "black", 'spurious': "red", 'compact': "blue", 'extended': "green",
                                    'extended-multisland': "orange", 'flagged': "magenta",
                                    'sidelobe': "red", 'source': "blue", 'galaxy': "yellow"}

    # ---- mask helpers (analyze.py:2142-2171) ---------------------------------------------------------------
    def merge_masks(self, mask1, mask2):
        mask = mask1 + mask2
        mask[mask > 1] = 1
        return mask

    def extract_mask_connected_components(self, mask):
        return label_components(mask)

    def are_mask_connected(self, mask1, mask2):
        _, n1 = label_components(mask1)
        _, n2 = label_components(mask2)
        _, n = label_components(self.merge_masks(mask1, mask2))
        return n != n1 + n2

    # ---- predict (analyze.py:833-905) ----------------------------------------------------------------------
    def predict(self, image, image_id='', bboxes_gt=[], header=None, xmin=0, ymin=0):
        if self._set_image(image, image_id, header, xmin, ymin) < 0:
            return -1
        r = self.model.detect([self.image], verbose=0)[0]
        kept = getattr(self.model, "last_masks_device", None)      # MaskRCNN keeps the device tensor of its last un-mold
        return self._accept(r, kept[0] if kept else None, bboxes_gt)

    def accept_detection(self, image, r, masks_device=None, image_id='', bboxes_gt=[], header=None, xmin=0, ymin=0):
        """Everything of predict but its model.detect call, for a detection result `r` that is already there (one image of a
        batched detect: the tiled source finder).  `image` is the image or just its shape (h, w[, c]): nothing here reads the
        pixels.  `masks_device`: the device tensor behind r['masks'] when the model kept it, else None."""
        if self._set_image(image, image_id, header, xmin, ymin) < 0:
            return -1
        return self._accept(r, masks_device, bboxes_gt)

    def _set_image(self, image, image_id, header, xmin, ymin):
        if image is None:
            logger.error("No input image given!")
            return -1
        if isinstance(image, (tuple, list)):
            self.image, self.image_shape = None, tuple(int(v) for v in image)
        else:
            self.image, self.image_shape = image, tuple(image.shape)
        self.image_xmin, self.image_ymin = xmin, ymin
        if image_id:
            self.image_id = image_id
        if header:
            self.image_header = header
        return 0

    def _accept(self, r, masks_device, bboxes_gt):
        self.class_names = self.config.CLASS_NAMES
        self.masks, self.boxes, self.class_ids, self.scores = r['masks'], r['rois'], r['class_ids'], r['scores']
        self.nobjects = self.masks.shape[-1]
        self.masks_device = masks_device
        self.masks_device_host = self.masks
        self.results, self.obj_regions = {}, []
        if self.nobjects > 0:
            self.extract_det_masks()
        else:
            self.masks_final, self.class_ids_final, self.class_names_final, self.scores_final = [], [], [], []
            self.bboxes, self.captions = [], []
            logger.warning("No detected object found for image %s ..." % self.image_id)
            return 0
        self.bboxes_gt = bboxes_gt
        if self.draw:                                                     # analyze.py:869-876
            self.draw_results(self.outfile or 'out_' + str(self.image_id) + '.png')
        self.make_json_results()
        if self.write_to_json:
            self.write_json_results(self.outfile_json or 'out_' + str(self.image_id) + '.json')
        self.make_ds9_regions(self.use_polygon_regions)
        if self.write_to_ds9:
            self.write_ds9_regions(self.outfile_ds9 or 'out_' + str(self.image_id) + '.reg')
        return 0

    # ---- extract_det_masks (analyze.py:1162-1496) ----------------------------------------------------------
    @staticmethod
    def has_gpu(model):
        return model_has_gpu(model)

    def _device(self):
        return model_device(self.model)

    def extract_det_masks(self):
        """Score filter, mask splitting, merging and selection: on the GPU's bit planes when ``postprocess_device`` is set
        (default: off, see __init__), there are at least ``postprocess_device_min_masks`` detections and the masks are 0 / 1
        masks (a lone mask is handed on with its own values); else by the host statement.  Both give the same lists."""
        m = np.asarray(self.masks)
        if self.postprocess_device and m.shape[-1] >= self.postprocess_device_min_masks and m.ndim == 3 and \
                masks_fit_planes(np.moveaxis(m, -1, 0), binary=True):
            return device_or_host("extract_det_masks_device", self.extract_det_masks_device, self.extract_det_masks_host)
        return self.extract_det_masks_host()

    def extract_det_masks_host(self):
        """The literal statement: mask_iou and are_mask_connected (three labellings) on full frames, asked pair by pair."""
        self._extract_det_masks(self._frame_masks)

    def _host_pieces(self, wanted):
        """The host statement of "the pieces of these detections": for wanted = [(detection, split it?)] the list [(detection,
        None: its whole mask, or the bool frame of one of its 4-connected components, in label order)] and the number of entries
        each detection gave."""
        dets, pieces = [], []
        for i, split in wanted:
            if not split:
                dets.append((i, None))
                pieces.append(1)
                continue
            labels, ncomp = label_components(self.masks[:, :, i])
            dets.extend((i, labels == k + 1) for k in range(ncomp))
            pieces.append(ncomp)
        return dets, pieces

    def _frame_masks(self, wanted):
        dets, pieces = self._host_pieces(wanted)
        return _FrameMasks(self, [self.masks[:, :, i] if piece is None else np.where(piece, [1], [0]) for i, piece in dets]), pieces

    def extract_det_masks_device(self):
        """The same decisions from three launches on bit planes (_PlaneMasks), every one taken on the host from exact integer
        counts; only the planes that end up in masks_final are downloaded, and they stay on the device as _final_planes."""
        self.postprocess_timing = {"masks": int(self.masks.shape[-1]), "mask_uploads": 0}
        t = self._extract_det_masks(self._plane_masks)
        for name, a, b in zip(("upload_pack", "merge_pairs", "union", "select_pairs", "host_lists", "download_unpack"), t[:-1], t[1:]):
            self.postprocess_timing[name + "_ms"] = round(1e3 * (b - a), 3)

    def _plane_masks(self, wanted):
        """The _PlaneMasks of `wanted` (see _extract_det_masks) and the pieces per detection.  With split_masks the pieces are cut
        on the device (ops.mask_components_split) when ``components_device`` is set, else on the host and uploaded."""
        if self.split_masks and self.components_device:
            from . import ops
            return device_or_host("split_masks_device", lambda: self._plane_pieces_device(wanted),
                                  lambda: self._plane_pieces_host(wanted), refusal=ops.ComponentsUnsupported)
        return self._plane_pieces_host(wanted)

    def _masks_tensor(self):
        """(self.masks as a device tensor of bytes, uploads): the model's own tensor when it is theirs, else one upload."""
        import torch
        kept = self.masks_device
        if kept is not None and self.masks_device_host is self.masks and torch.is_tensor(kept) and kept.is_cuda and \
                tuple(kept.shape) == tuple(self.masks.shape):
            return kept, 0
        m = self.masks if self.masks.dtype == np.bool_ else self.masks != 0
        return torch.from_numpy(np.ascontiguousarray(m).view(np.uint8)).to(self._device()), 1

    def _plane_pieces_host(self, wanted):
        """Packed from the model's own device tensor, else from one upload -- of self.masks, or with split_masks of the masks the
        host statement split."""
        import torch
        from . import ops
        dets, pieces = self._host_pieces(wanted)
        if not dets:
            return None, pieces
        dtypes = [[self.masks.dtype if piece is None else SPLIT_DTYPE] for _, piece in dets]     # of the host statement's arrays
        if self.split_masks:
            index = range(len(dets))
            stack = np.stack([self.masks[:, :, i] != 0 if piece is None else piece for i, piece in dets], axis=-1).view(np.uint8)
            masks_t, uploads = torch.from_numpy(stack).to(self._device()), 1
        else:
            index = [i for i, _ in dets]
            masks_t, uploads = self._masks_tensor()
        self.postprocess_timing["mask_uploads"] = uploads
        return _PlaneMasks(self, ops.mask_planes_pack(masks_t.contiguous()), index, dtypes), pieces

    def _plane_pieces_device(self, wanted):
        """The planes of the wanted detections, packed from the tensor the model kept (else one upload of self.masks), followed by
        the planes of their components (ops.mask_components, 4-connected, and mask_components_split): a detection that is not
        split is its own plane, one that is becomes its pieces in label order.  No mask is labelled or uploaded piece by piece."""
        import torch
        from . import ops
        t0 = time.perf_counter()
        masks_t, uploads = self._masks_tensor()
        self.postprocess_timing["mask_uploads"] = uploads
        planes = ops.mask_planes_pack(masks_t.contiguous())
        ids = torch.as_tensor([i for i, _ in wanted], device=planes.words.device)
        whole = ops.MaskPlanes(planes.words.index_select(0, ids), planes.count.index_select(0, ids), planes.box.index_select(0, ids), planes.W)
        parts, offs = ops.mask_components_split(ops.mask_components(whole, 4))
        index, dtypes, pieces = [], [], []
        for k, (_, split) in enumerate(wanted):
            if split:
                first, last = whole.n + int(offs[k]), whole.n + int(offs[k + 1])
                index.extend(range(first, last))
                dtypes.extend([[SPLIT_DTYPE]] * (last - first))
                pieces.append(last - first)
            else:
                index.append(k)
                dtypes.append([self.masks.dtype])
                pieces.append(1)
        self.components_timing["split_masks_ms"] = round(1e3 * (time.perf_counter() - t0), 3)
        self.components_timing["split_pieces"] = int(offs[-1])
        if not index:
            return None, pieces
        both = ops.MaskPlanes(torch.cat([whole.words, parts.words]), torch.cat([whole.count, parts.count]),
                              torch.cat([whole.box, parts.box]), whole.W)
        return _PlaneMasks(self, both, index, dtypes), pieces

    def _extract_det_masks(self, mask_set):
        """extract_det_masks, rule for rule in the order of the reference, on a mask set (_FrameMasks or _PlaneMasks) that answers
        the pixel questions.  ``mask_set(wanted)`` builds it from wanted = [(detection, is it to be split into its connected
        pieces)] and says how many masks each detection became (a whole mask: 1; a split one: its components in label order).
        Returns the times at the borders of the device form's phases."""
        clock = time.perf_counter
        t = [clock()]
        self.masks_final, self.class_ids_final, self.class_names_final, self.scores_final = [], [], [], []
        self.bboxes, self.captions = [], []
        self._final_planes = None
        sel = [i for i in range(self.boxes.shape[0]) if not self.scores[i] < self.score_thr]
        order = np.argsort([self.scores[i] for i in sel])[::-1]

        wanted = [(sel[index], bool(self.split_masks and self.class_names[self.class_ids[sel[index]]] not in NO_SPLIT_CLASSES))
                  for index in order]
        if not wanted:
            return t
        masks_det, pieces = mask_set(wanted)
        class_ids_det, scores_det = [], []
        for (i, _), count in zip(wanted, pieces):
            class_ids_det.extend([self.class_ids[i]] * count)
            scores_det.extend([self.scores[i]] * count)
        N = len(class_ids_det)
        if N == 0:
            return t
        masks_det.sync()
        t.append(clock())

        thr = self.merge_overlap_iou_thr
        if self.merge_overlapped_masks:                                 # class equality, then IoU, then contact
            ii, jj = _pairs_below(N)
            cls = np.asarray(class_ids_det)
            same = cls[ii] == cls[jj]
            ii, jj = ii[same], jj[same]
            iou, connected = masks_det.pair_stats(ii, jj)
            edges = []
            for k, (i, j) in enumerate(zip(ii.tolist(), jj.tolist())):
                if iou[k] < thr:
                    continue
                if connected[k]:
                    edges.append((i, j))
            comps, class_ids_merged, scores_merged = connected_components(N, edges), [], []
            for comp in comps:
                class_ids_merged.append(class_ids_det[comp[-1]])
                score_avg = 0
                for index in comp:
                    score_avg += scores_det[index]
                scores_merged.append(score_avg * (1. / len(comp)))
        else:
            comps, class_ids_merged, scores_merged = [[k] for k in range(N)], list(class_ids_det), list(scores_det)
        masks_det.sync()
        t.append(clock())
        masks_merged = masks_det.union(comps)
        masks_det.sync()
        t.append(clock())

        n_final = len(comps)
        is_selected = [True] * n_final
        if self.select_best_overlapped_masks:                           # contact, then IoU only for source / sidelobe pairs
            ii, jj = _pairs_below(n_final)
            iou, connected = masks_merged.pair_stats(ii, jj)
            adj = {}
            for k, (i, j) in enumerate(zip(ii.tolist(), jj.tolist())):
                if not connected[k]:
                    continue
                label_i, label_j = self.class_names[class_ids_merged[i]], self.class_names[class_ids_merged[j]]
                sidelobe_other = (label_i == 'spurious') != (label_j == 'spurious')
                if self.split_source_sidelobe and sidelobe_other and iou[k] < thr:
                    continue
                adj.setdefault(i, set()).add(j)
                adj.setdefault(j, set()).add(i)
            cliques = maximal_cliques(adj)
            best = []
            for clique in cliques:
                max_score, max_index = -1, -1
                for index in clique:
                    if scores_merged[index] > max_score:
                        max_score, max_index = scores_merged[index], index
                best.append((max_score, max_index))
            for k in sorted(range(len(cliques)), key=lambda k: best[k][0], reverse=True):
                for index in cliques[k]:
                    if index != best[k][1] and is_selected[index]:
                        is_selected[index] = False
        masks_det.sync()
        t.append(clock())

        keep = []
        for index in range(n_final):
            if not is_selected[index]:
                continue
            bbox = masks_merged.box(index)
            if bbox[1] >= bbox[3] or bbox[0] >= bbox[2]:
                logger.warning("Invalid det bbox(%d,%d,%d,%d), skip it ..." % (bbox[1], bbox[3], bbox[0], bbox[2]))
                continue
            keep.append(index)
            label = self.class_names[class_ids_merged[index]]
            self.class_ids_final.append(class_ids_merged[index])
            self.class_names_final.append(label)
            self.scores_final.append(scores_merged[index])
            self.bboxes.append(bbox)
            self.captions.append("{} {:.2f}".format(label, scores_merged[index]))
        t.append(clock())
        self.masks_final = masks_merged.final(keep)
        t.append(clock())
        return t

    # ---- the tester's path (analyze.py:715-828, :907-1157, :1502-1861) ----------------------------------------
    def set_image_path(self, path):
        self.image_path = path
        self.image_path_base = os.path.basename(self.image_path)
        self.image_path_base_noext = os.path.splitext(self.image_path_base)[0]

    def get_data(self):
        """analyze.py:724-828: image, detections (class ids remapped on request) and ground truth of self.image_id."""
        if not self.dataset:
            logger.error("No dataset present!")
            return -1
        self.image = self.dataset.load_image(self.image_id)
        self.image_path_base = os.path.basename(self.image_path)
        self.image_path_base_noext = os.path.splitext(self.image_path_base)[0]
        self.image_uuid = self.dataset.image_uuid(self.image_id)
        self.image_metadata = self.dataset.image_metadata(self.image_id)
        r = self.model.detect([self.image], verbose=0)[0]
        self.class_names = self.dataset.class_names
        self.masks, self.boxes, self.class_ids, self.scores = r['masks'], r['rois'], r['class_ids'], r['scores']
        self.nobjects = self.masks.shape[-1]
        kept = getattr(self.model, "last_masks_device", None)
        self.masks_device = kept[0] if kept else None
        self.masks_device_host = self.masks
        if self.remap_classids and self.classid_map:                                     # :760-776
            class_ids_remapped = []
            for class_id in self.class_ids:
                if class_id in self.classid_map:
                    class_ids_remapped.append(self.classid_map[class_id])
                else:
                    logger.error("Requested to remap class_id=%d but not found in map keys!" % class_id)
                    return -1
            self.class_ids = class_ids_remapped
        self.class_names_gt = self.dataset.class_names
        self.masks_gt = self.dataset.load_gt_masks(self.image_id, binary=False)
        self.class_ids_gt = self.dataset.image_info[self.image_id]["class_ids"]
        self.sidelobes_mixed_or_near_gt = self.dataset.image_info[self.image_id]['sidelobes_mixed_or_near']
        self.labels_gt, self.captions_gt = [], []
        for item in self.class_ids_gt:                                                   # (the colours of :805 are for plots only)
            label = self.class_names_gt[item]
            self.labels_gt.append(label)
            self.captions_gt.append(label)
        self.objs_gt = self.dataset.load_gt_obj_info(self.image_id)
        if not self.objs_gt:
            logger.warning("gt object info list is empty (hint: no object in this image or input data not in json format)...")
        return 0

    def inspect_results(self, image_id, image_path):
        """analyze.py:907-1034: get_data -> extract_gt_masks -> extract_det_masks -> compute_det_mask_pars ->
        compute_performances, with the appends to gt_data / pred_data in between; plots stay out of scope."""
        self.image_id = image_id
        self.image_path = image_path
        if self.get_data() < 0:
            logger.error("Failed to set data from provided dataset!")
            return -1
        self.extract_gt_masks()
        gt_data_for_image = []
        for i, (bbox_gt, label) in enumerate(zip(self.bboxes_gt, self.captions_gt)):
            if not self.dataset.consider_sources_near_mixed_sidelobes:
                if self.sidelobes_mixed_or_near_gt_merged[i] == 1:
                    continue
            gt_instance = bbox_gt.tolist()
            gt_instance.append(label)
            gt_data_for_image.append(gt_instance)
        self.gt_data.append(gt_data_for_image)
        if self.nobjects > 0:
            self.extract_det_masks()
        else:
            logger.warning("No detected object found for image %s ..." % self.image_path_base)
        if self.nobjects > 0:
            self.compute_det_mask_pars()
        pred_data_for_image = []
        for bbox_pred, label_score in zip(self.bboxes, self.captions):
            pred_object = bbox_pred.tolist()
            pred_object.append(label_score.split(' ')[0])
            pred_object.append(float(label_score.split(' ')[1]))
            pred_data_for_image.append(pred_object)
        self.pred_data.append(pred_data_for_image)
        self.compute_performances()
        if self.draw:                                                     # analyze.py:1018-1023
            self.draw_results('out_' + self.image_path_base_noext + '_id' + str(self.image_uuid) + '.png')
        return 0

    def extract_gt_masks(self):
        """analyze.py:1039-1155: the true masks as they are, or (split_gtmasks) split into connected pieces and the touching
        pieces of one class merged again; then their boxes and captions.  With ``split_gtmasks`` and ``components_device`` the
        pieces, the contact tests and the unions are done on bit planes (``extract_gt_masks_device``) where a GPU is there and the
        true masks are 0 / 1 frames; else, and for every other setting, by the host statement."""
        m = np.asarray(self.masks_gt)
        if self.split_gtmasks and self.components_device and m.ndim == 3 and m.shape[-1] > 0 and Analyzer.has_gpu(self.model) and \
                masks_fit_planes(np.moveaxis(m, -1, 0), binary=True):
            from . import ops
            return device_or_host("extract_gt_masks_device", self.extract_gt_masks_device, self.extract_gt_masks_host,
                                  refusal=ops.ComponentsUnsupported)
        return self.extract_gt_masks_host()

    def extract_gt_masks_device(self):
        """extract_gt_masks_host with split_gtmasks, on bit planes: the true masks are packed once; component 1 of every mask that
        is split comes from ops.mask_components_split(first_only) and stands ncomp times in the list, as the reference has it;
        same-class pairs are tested with mask_pair_stats' touch (== are_mask_connected); the groups are merged by mask_union,
        whose boxes are bboxes_gt.  A true mask that ends up alone and whole is handed on as the array it came as."""
        import torch
        from . import ops
        t0 = time.perf_counter()
        masks_gt, dtype = self.masks_gt, self.masks_gt.dtype
        K = masks_gt.shape[-1]
        planes, _ = self._planes_of([masks_gt[:, :, k] for k in range(K)])
        handle = ops.mask_components(planes, 4)
        parts, offs = ops.mask_components_split(handle, first_only=True)
        ncomp = handle.ncomp_host
        index, source, class_ids_gt_det, sidelobes_gt_det = [], [], [], []     # per list entry: its plane, the whole mask it is (or None)
        for k in range(K):
            whole = self.labels_gt[k] in NO_SPLIT_CLASSES_GT
            copies = 1 if whole else int(ncomp[k])
            index.extend([k if whole else K + int(offs[k])] * copies)
            source.extend([k if whole else None] * copies)
            class_ids_gt_det.extend([self.class_ids_gt[k]] * copies)
            sidelobes_gt_det.extend([self.sidelobes_mixed_or_near_gt[k]] * copies)
        N = len(index)
        self.masks_gt_merged, self.class_ids_gt_merged, self.bboxes_gt, self.captions_gt = [], [], [], []
        self.sidelobes_mixed_or_near_gt_merged = []
        self.components_timing["gt_entries"] = N
        if N == 0:
            return
        both = ops.MaskPlanes(torch.cat([planes.words, parts.words]), torch.cat([planes.count, parts.count]),
                              torch.cat([planes.box, parts.box]), planes.W)
        index = np.asarray(index, dtype=np.int32)
        ii, jj = _pairs_below(N)
        cls = np.asarray([int(c) for c in class_ids_gt_det])
        same = cls[ii] == cls[jj]
        ii, jj = ii[same], jj[same]
        edges = []
        if ii.size:
            _, touch = ops.mask_pair_stats(both, np.stack([index[ii], index[jj]], axis=1))
            hit = touch.cpu().numpy() != 0
            edges = list(zip(ii[hit].tolist(), jj[hit].tolist()))
        comps = connected_components(N, edges)
        comp_offsets = np.concatenate([[0], np.cumsum([len(comp) for comp in comps])])
        merged = ops.mask_union(both, comp_offsets, index[[k for comp in comps for k in comp]])
        boxes = merged.box.cpu().numpy()
        alone = [source[comp[0]] if len(comp) == 1 else None for comp in comps]
        need = [c for c in range(len(comps)) if alone[c] is None]
        unpacked = {}
        if need:
            ids = torch.as_tensor(need, device=merged.words.device)
            frames = unpack_mask_planes(merged.words.index_select(0, ids).cpu().numpy(), merged.W)
            unpacked = {c: frames[q].astype(dtype) for q, c in enumerate(need)}
        for c, comp in enumerate(comps):
            self.masks_gt_merged.append(masks_gt[:, :, alone[c]] if alone[c] is not None else unpacked[c])
            self.class_ids_gt_merged.append(class_ids_gt_det[comp[-1]])               # class and flag of the last member
            self.sidelobes_mixed_or_near_gt_merged.append(sidelobes_gt_det[comp[-1]])
            self.bboxes_gt.append(boxes[c].astype(np.int32))
            self.captions_gt.append(self.class_names_gt[self.class_ids_gt_merged[c]])
        self._eval_planes["gt"] = (merged, self.masks_gt_merged)          # compute_performances_device works on these
        self.components_timing["gt_masks_ms"] = round(1e3 * (time.perf_counter() - t0), 3)

    def extract_gt_masks_host(self):
        """The literal statement: every true mask labelled, are_mask_connected (three labellings) for all pairs of pieces."""
        self.masks_gt_merged, self.class_ids_gt_merged, self.bboxes_gt, self.captions_gt = [], [], [], []
        self.sidelobes_mixed_or_near_gt_merged = []
        if self.split_gtmasks:
            masks_gt_det, class_ids_gt_det, sidelobes_gt_det = [], [], []
            for k in range(self.masks_gt.shape[-1]):
                mask_gt, label_gt = self.masks_gt[:, :, k], self.labels_gt[k]
                if label_gt in NO_SPLIT_CLASSES_GT:                                       # :1065
                    masks_gt_det.append(mask_gt)
                    class_ids_gt_det.append(self.class_ids_gt[k])
                    sidelobes_gt_det.append(self.sidelobes_mixed_or_near_gt[k])
                    continue
                component_labels_gt, ncomponents_gt = self.extract_mask_connected_components(mask_gt)
                for i in range(ncomponents_gt):
                    # As the reference has it (:1075): component 1 on EVERY iteration, not component i + 1 -- a mask of k
                    # components yields k copies of its first component (which the merge below joins into one again).
                    extracted_mask = np.zeros(mask_gt.shape, dtype=mask_gt.dtype)
                    extracted_mask[np.where(component_labels_gt == 1)] = 1
                    masks_gt_det.append(extracted_mask)
                    class_ids_gt_det.append(self.class_ids_gt[k])
                    sidelobes_gt_det.append(self.sidelobes_mixed_or_near_gt[k])
            N = len(masks_gt_det)
            edges = []
            for i in range(N):
                for j in range(i + 1, N):
                    connected = self.are_mask_connected(masks_gt_det[i], masks_gt_det[j])
                    if connected and class_ids_gt_det[i] == class_ids_gt_det[j]:
                        edges.append((i, j))
            for comp in connected_components(N, edges):
                merged_mask = masks_gt_det[comp[0]]
                for index in comp[1:]:
                    merged_mask = self.merge_masks(merged_mask, masks_gt_det[index])
                self.masks_gt_merged.append(merged_mask)
                self.class_ids_gt_merged.append(class_ids_gt_det[comp[-1]])               # class and flag of the last member
                self.sidelobes_mixed_or_near_gt_merged.append(sidelobes_gt_det[comp[-1]])
        else:
            for k in range(self.masks_gt.shape[-1]):
                self.masks_gt_merged.append(self.masks_gt[:, :, k])
                self.class_ids_gt_merged.append(self.class_ids_gt[k])
                self.sidelobes_mixed_or_near_gt_merged.append(self.sidelobes_mixed_or_near_gt[k])
        for i in range(len(self.masks_gt_merged)):
            mask = self.masks_gt_merged[i]
            mask_expanded = np.zeros([mask.shape[0], mask.shape[1], 1], dtype=bool)
            mask_expanded[:, :, 0] = mask
            self.bboxes_gt.append(utils.extract_bboxes(mask_expanded)[0])
            self.captions_gt.append(self.class_names_gt[self.class_ids_gt_merged[i]])

    # -- where the pixel work of the two steps below runs
    def _eval_on_device(self):
        if not self.eval_device or len(self.masks_gt_merged) * len(self.masks_final) < max(self.eval_device_min_pairs, 1):
            return False
        return masks_fit_planes(list(self.masks_final) + list(self.masks_gt_merged), binary=False)

    def _planes_of(self, masks, key=None):
        """(MaskPlanes, uploads) of a list of [H, W] masks: the planes extract_det_masks_device left on the device when `masks` is
        the very list they were made for (0 uploads), else one stack, upload and pack.  Under a key (the tester's "gt" and
        "final") the planes are remembered while the list is the same object."""
        have = self._eval_planes.get(key)
        if have is not None and have[1] is masks:
            return have[0], 0
        if self._final_planes is not None and self._final_planes[1] is masks:
            planes, uploads = self._final_planes[0], 0
        else:
            import torch
            from . import ops
            stack = np.ascontiguousarray(np.stack([np.asarray(m) != 0 for m in masks], axis=-1))
            planes, uploads = ops.mask_planes_pack(torch.from_numpy(stack.view(np.uint8)).to(self._device())), 1
        if key is not None:
            self._eval_planes[key] = (planes, masks)
        return planes, uploads

    def _eval_planes_of(self, key, masks):
        planes, uploads = self._planes_of(masks, key)
        if uploads:
            self.eval_timing["mask_uploads"] = self.eval_timing.get("mask_uploads", 0) + uploads
        return planes

    # ---- compute_det_mask_pars (analyze.py:1502-1676) ------------------------------------------------------------
    def compute_det_mask_pars(self):
        """Per detected object: pixel count, flux sum and signal-to-noise on the un-stretched image, upright and minimum-area
        boxes, islands, border flag, sizes in beams.  The per-mask pixel count, box and flux sum come from
        ``compute_det_mask_pars_device`` (ops.mask_plane_sums on bit planes) when the device path is on, else from full frames;
        with ``components_device`` that path also brings the island counts (ops.mask_components, 8-connected) and the hull points
        of the minimum-area box (ops.mask_row_extents); everything after them is the same host code."""
        from . import fits
        logger.info("Reading 2D origin image data from file %s ..." % self.image_path)
        res = fits.read_fits(self.image_path, stretch=False, normalize=False, convertToRGB=False, to_uint8=False,
                             stretch_biascontrast=False)
        if res is None:
            return -1
        data = res[0]
        if data.ndim != 2:
            logger.error("Image size needed for computing morph pars should be =2 and not %d!" % data.ndim)
            return -1
        if self._eval_on_device() and data.dtype == np.float32 and len(self.masks_final) > 0 and \
                tuple(data.shape) == tuple(np.asarray(self.masks_final[0]).shape):
            pixel_sums = device_or_host("compute_det_mask_pars_device", lambda: self.compute_det_mask_pars_device(data),
                                        lambda: self.compute_det_mask_pars_host(data))
        else:
            pixel_sums = self.compute_det_mask_pars_host(data)
        return self._det_mask_pars_from(data, *pixel_sums)

    def compute_det_mask_pars_host(self, data):
        """(npix, boxes, Stot) of masks_final from full frames."""
        npix, boxes, stot = [], [], []
        for mask in self.masks_final:
            mask = np.asarray(mask)
            cond = np.logical_and(np.isfinite(mask), mask != 0)
            npix.append(int(np.count_nonzero(cond)))
            # float64 sum of the float32 pixels (the reference's np.nansum accumulates in the image's own float32: DESIGN.md 4.9)
            stot.append(float(np.nansum(data[cond], dtype=np.float64)))
            boxes.append(utils.extract_bboxes((mask != 0)[:, :, None])[0])
        return npix, boxes, stot

    def compute_det_mask_pars_device(self, data):
        """(npix, boxes, Stot) of masks_final from the bit planes: counts and boxes as _pack / _union left them, the flux sums from
        one ops.mask_plane_sums launch over the image, uploaded once."""
        import torch
        from . import ops
        t0 = time.perf_counter()
        planes = self._eval_planes_of("final", self.masks_final)
        img_t =torch.from_numpy(np.ascontiguousarray(data)).to(planes.words.device)
        sums = ops.mask_plane_sums(img_t, planes)
        n = planes.n
        if self.components_device:
            shape = device_or_host("det_mask_shape_device", lambda: self._det_mask_shape_device(planes), lambda: None,
                                   refusal=ops.ComponentsUnsupported)
            if shape is not None:
                ints, islands, points = shape
                stot = sums.cpu().numpy()
                self.eval_timing["det_mask_pars_ms"] = round(1e3 * (time.perf_counter() - t0), 3)
                return ints[:n].tolist(), list(ints[n:5 * n].reshape(n, 4)), stot.tolist(), islands, points
        ints = torch.cat([planes.count, planes.box.reshape(-1)]).cpu().numpy()
        stot = sums.cpu().numpy()
        self.eval_timing["det_mask_pars_ms"] = round(1e3 * (time.perf_counter() - t0), 3)
        return ints[:n].tolist(), list(ints[n:].reshape(n, 4)), stot.tolist()

    def _det_mask_shape_device(self, planes):
        """(ints, islands, points) of the final planes: the counts and boxes compute_det_mask_pars_device reads anyway, the
        8-connected component count of every plane (count_islands) and the row_extreme_points of every plane (None for an empty
        one), all from ONE download.  The workspace is sized from self.bboxes, the boxes extract_det_masks left for these very
        masks; the download brings the planes' own boxes along, and only if the two differ is the work done again from those."""
        import torch
        from . import ops
        n = planes.n
        host = np.asarray(self.bboxes, dtype=np.int32).reshape(-1, 4) if len(self.bboxes) == n else planes.box.cpu().numpy()
        for attempt in range(2):
            handle = ops.mask_components(planes, 8, boxes_host=host)
            extents, row_offsets = ops.mask_row_extents(planes, boxes_host=host)
            ints = torch.cat([planes.count, planes.box.reshape(-1), handle.ncomp, extents.reshape(-1)]).cpu().numpy()
            boxes = ints[n:5 * n].reshape(n, 4)
            if np.array_equal(boxes, host):
                break
            host = np.ascontiguousarray(boxes, dtype=np.int32)
        else:
            raise ops.ComponentsUnsupported("the planes' boxes changed between two downloads")
        islands = ints[5 * n:6 * n].tolist()
        ext = ints[6 * n:].reshape(-1, 2)
        points = [row_extents_points(ext[row_offsets[k]:row_offsets[k + 1]], boxes[k, 0]) for k in range(n)]
        self.components_timing["det_mask_shape_downloads"] = attempt + 1
        return ints, islands, points

    def _det_mask_pars_from(self, data, npix, boxes, stot, islands=None, points=None):
        has_metadata = bool(self.image_metadata)
        if has_metadata:                                                                  # :1510-1524
            md = self.image_metadata
            nx, ny, dx, dy = md["nx"], md["ny"], md["dx"], md["dy"]
            img_bkg, img_rms, bmaj, bmin = md["bkg"], md["rms"], md["bmaj"], md["bmin"]
            beamArea = np.pi * bmaj * bmin / (4 * np.log(2))
            pixelArea = np.abs(dx * dy)
            npixInBeam = beamArea / pixelArea
            beamWidth = np.sqrt(np.abs(bmaj * bmin))
            pixScale = np.sqrt(np.abs(dx * dy))
            beamWidthInPixel = int(math.ceil(beamWidth / pixScale))
        else:
            # The reference goes on to read img_bkg, nx and ny, which it never set: a NameError.  Here the frame's own size
            # stands for nx, ny and the signal-to-noise is the -999 of the branch below.
            ny, nx = data.shape
        self.det_obj_pars = []
        for i in range(len(self.masks_final)):
            name = 'Sdet' + str(i + 1)
            class_name = self.class_names[self.class_ids_final[i]]
            mask = np.asarray(self.masks_final[i])
            npix_tot, Stot = npix[i], stot[i]
            if has_metadata:
                with np.errstate(divide="ignore", invalid="ignore"):
                    Sbkg = img_bkg * npix_tot
                    S = Stot - Sbkg
                    Serr_noise = img_rms * np.sqrt(npix_tot)
                    SNR = np.float64(S) / Serr_noise
            else:
                SNR = -999
            if points is None:
                rect = min_area_rect(mask)
            else:
                rect = None if points[i] is None else min_area_rect_of_points(points[i])
            if rect is None:                                                              # "no contours": :1592-1595
                logger.warning("No contours found for object no. %d, fill empty dict!" % (i + 1))
                self.det_obj_pars.append({})
                continue
            nislands = count_islands(mask) if islands is None else islands[i]
            # cv.boundingRect of the contour points: x, y of the first pixel, w, h up to one past the last -- extract_bboxes
            y1, x1, y2, x2 = (int(v) for v in boxes[i])
            bbox_w, bbox_h = x2 - x1, y2 - y1
            bbox_x, bbox_y = x1 + 0.5 * bbox_w, y1 + 0.5 * bbox_h
            (bbox_min_x, bbox_min_y), (bbox_min_w, bbox_min_h), bbox_min_angle = rect
            at_border_x = (bbox_x - 0.5 * bbox_w <= 0) or (bbox_x + 0.5 * bbox_w >= nx)
            at_border_y = (bbox_y - 0.5 * bbox_h <= 0) or (bbox_y + 0.5 * bbox_h >= ny)
            at_border = at_border_x or at_border_y
            if has_metadata:
                nbeams = float(npix_tot) / float(npixInBeam)
                minSizeVSBeam = float(min(bbox_min_w, bbox_min_h)) / beamWidthInPixel
                maxSizeVSBeam = float(max(bbox_min_w, bbox_min_h)) / beamWidthInPixel
                minSizeVSImg = min(float(bbox_w) / float(nx), float(bbox_h) / float(ny))
                maxSizeVSImg = max(float(bbox_w) / float(nx), float(bbox_h) / float(ny))
            else:
                nbeams = minSizeVSBeam = maxSizeVSBeam = minSizeVSImg = maxSizeVSImg = -999
            self.det_obj_pars.append({
                "Stot": float(Stot), "bbox_angle": float(bbox_min_angle), "bbox_h": float(bbox_min_h), "bbox_w": float(bbox_min_w),
                "bbox_x": float(bbox_min_x), "bbox_y": float(bbox_min_y), "border": int(at_border), "class": class_name,
                "maxsize_beam": maxSizeVSBeam, "maxsize_img_fract": maxSizeVSImg, "minsize_beam": minSizeVSBeam,
                "minsize_img_fract": minSizeVSImg, "name": name, "nbeams": nbeams, "nislands": nislands, "npix": npix_tot,
                "snr": float(SNR)})
        return 0

    # ---- compute_performances (analyze.py:1682-1860) -----------------------------------------------------------------
    def compute_performances(self):
        """Matches true and detected objects by mask IoU and fills the confusion matrix, the purity and the per-object lists.
        The IoUs come from ``compute_performances_device`` (one ops.mask_cross_stats launch) when the device path is on, else
        from ``compute_performances_host`` (mask_iou on full frames per pair); the two loops are the same code."""
        if self._eval_on_device():
            return device_or_host("compute_performances_device", self.compute_performances_device, self.compute_performances_host)
        return self.compute_performances_host()

    def compute_performances_host(self):
        # jaccard_score(masks_final[j].flatten(), masks_gt_merged[i].flatten().astype(bool), average='binary') [3P] == mask_iou
        return self._match_objects(lambda i, j: mask_iou(self.masks_final[j], self.masks_gt_merged[i]))

    def compute_performances_device(self):
        """The intersections of all (true object, detection) pairs from one launch on bit planes; the union is count_gt +
        count_det - inter.  One download; every decision is taken by the loops of _match_objects."""
        import torch
        from . import ops
        t0 = time.perf_counter()
        G, D = len(self.masks_gt_merged), len(self.masks_final)
        gt = self._eval_planes_of("gt", self.masks_gt_merged)
        det = self._eval_planes_of("final", self.masks_final)
        inter = ops.mask_cross_stats(gt, det)
        got = torch.cat([inter.reshape(-1), gt.count, det.count]).cpu().numpy().tolist()
        count_gt, count_det = got[G * D:G * D + G], got[G * D + G:]
        self.eval_timing["performances_ms"] = round(1e3 * (time.perf_counter() - t0), 3)

        def iou(i, j):
            n_inter = got[i * D + j]
            union = count_gt[i] + count_det[j] - n_inter
            return float(n_inter) / float(union) if union else 0.0
        return self._match_objects(iou)

    def _match_objects(self, iou_of):
        """The two loops of compute_performances, rule for rule; ``iou_of(i, j)`` is the mask IoU of true object i and detection j."""
        self.confusion_matrix = np.zeros((self.n_classes, self.n_classes))
        self.confusion_matrix_norm = np.zeros((self.n_classes, self.n_classes))
        self.purity = np.zeros((1, self.n_classes))
        self.nobjs_true = np.zeros((1, self.n_classes))
        self.nobjs_det = np.zeros((1, self.n_classes))
        self.nobjs_det_right = np.zeros((1, self.n_classes))
        self.detobj_classids, self.detobj_class_names, self.detobj_gtinfo = [], [], []
        self.is_gt_obj_detected = []
        self.is_det_obj_matching_to_gt_obj, self.is_det_obj_matching_to_gt_obj_sameclass = [], []
        self.matchobj_classids, self.matchobj_class_names, self.matchobj_ious = [], [], []
        # (detobj_scores and detobj_ious are NOT reset, as in the reference: they grow with every call on one Analyzer)

        # true objects -> detections (:1703-1769)
        for i in range(len(self.bboxes_gt)):
            if not self.dataset.consider_sources_near_mixed_sidelobes:
                if self.sidelobes_mixed_or_near_gt_merged[i] == 1:
                    continue
            bbox_gt = self.bboxes_gt[i]
            class_id_gt = self.class_ids_gt_merged[i]
            self.nobjs_true[0][class_id_gt] += 1
            obj_info_gt = {}
            if self.objs_gt and not self.split_gtmasks:
                obj_info_gt = self.objs_gt[i]
            index_best, iou_best, score_best = -1, 0, 0
            for j in range(len(self.bboxes)):
                score, bbox = self.scores_final[j], self.bboxes[j]
                if bbox[1] >= bbox[3] or bbox[0] >= bbox[2]:
                    logger.warning("Invalid det bbox (%d,%d,%d,%d) in image %s when computing IOU among boxes, skip it..." % (
                        bbox[1], bbox[3], bbox[0], bbox[2], self.image_path))
                    continue
                if bbox_gt[1] >= bbox_gt[3] or bbox_gt[0] >= bbox_gt[2]:
                    logger.warning("Invalid gt bbox (%d,%d,%d,%d) in image %s when computing IOU among boxes, skip it..." % (
                        bbox_gt[1], bbox_gt[3], bbox_gt[0], bbox_gt[2], self.image_path))
                    continue
                mask_iou_ = iou_of(i, j)
                if mask_iou_ >= self.iou_thr and mask_iou_ >= iou_best:              # `>=`: of equal candidates the LAST wins
                    index_best, iou_best, score_best = j, mask_iou_, score
            if obj_info_gt:
                self.detobj_gtinfo.append(obj_info_gt)
            if index_best == -1:
                self.detobj_scores.append(-999)
                self.detobj_ious.append(-999)
                self.detobj_classids.append(-999)
                self.detobj_class_names.append("not-detected")
                self.is_gt_obj_detected.append(0)
            else:
                class_id_det = self.class_ids_final[index_best]
                self.confusion_matrix[class_id_gt][class_id_det] += 1
                self.detobj_scores.append(score_best)
                self.detobj_ious.append(iou_best)
                self.detobj_classids.append(class_id_det)
                self.detobj_class_names.append(self.class_names[class_id_det])
                self.is_gt_obj_detected.append(1)

        for i in range(self.n_classes):                                                  # :1773-1780
            norm = self.nobjs_true[0][i]
            if norm <= 0:
                continue
            for j in range(self.n_classes):
                self.confusion_matrix_norm[i][j] = self.confusion_matrix[i][j] / norm

        # detections -> true objects (:1783-1834); no sidelobe skip here
        for j in range(len(self.bboxes)):
            bbox = self.bboxes[j]
            class_id = self.class_ids_final[j]
            self.nobjs_det[0][class_id] += 1
            index_best, iou_best = -1, 0
            for i in range(len(self.bboxes_gt)):
                bbox_gt = self.bboxes_gt[i]
                if bbox[1] >= bbox[3] or bbox[0] >= bbox[2]:
                    continue
                if bbox_gt[1] >= bbox_gt[3] or bbox_gt[0] >= bbox_gt[2]:
                    continue
                mask_iou_ = iou_of(i, j)
                if mask_iou_ >= self.iou_thr and mask_iou_ >= iou_best:
                    index_best, iou_best = i, mask_iou_
            if index_best != -1:
                class_id_gt = self.class_ids_gt_merged[index_best]
                self.is_det_obj_matching_to_gt_obj.append(1)
                self.matchobj_classids.append(class_id_gt)
                self.matchobj_class_names.append(self.class_names[class_id_gt])
                self.matchobj_ious.append(iou_best)
                if class_id == class_id_gt:                                              # only a match of the same class is "right"
                    self.nobjs_det_right[0][class_id] += 1
                    self.is_det_obj_matching_to_gt_obj_sameclass.append(1)
                else:
                    self.is_det_obj_matching_to_gt_obj_sameclass.append(0)
            else:
                self.is_det_obj_matching_to_gt_obj.append(0)
                self.is_det_obj_matching_to_gt_obj_sameclass.append(0)
                self.matchobj_classids.append(-999)
                self.matchobj_class_names.append("not-matched")
                self.matchobj_ious.append(-999)

        for j in range(self.n_classes):                                                  # :1836-1840
            if self.nobjs_det[0][j] <= 0:
                continue
            self.purity[0][j] = self.nobjs_det_right[0][j] / self.nobjs_det[0][j]

        for title, value in (("NOBJ TRUE", self.nobjs_true), ("NOBJ DET", self.nobjs_det), ("NOBJ DET CORRECTLY", self.nobjs_det_right),
                             ("CLASSIFICATION MATRIX (not normalized)", self.confusion_matrix),
                             ("CLASSIFICATION MATRIX (normalized)", self.confusion_matrix_norm), ("PRECISION (or PURITY)", self.purity)):
            print("== SAMPLE %s ==" % title)
            print(value)

    # ---- JSON (analyze.py:1866-1955) -----------------------------------------------------------------------
    def _results_masks_ok(self):
        """The device forms of make_json_results and draw_results work on bit planes: 0 / 1 masks of one shape."""
        return masks_fit_planes(self.masks_final, binary=True)

    def make_json_results(self):
        """The result dictionary: contours and pixel lists on the GPU (``make_json_results_device``) when ``results_device`` is
        set (default: off), a GPU is there, there are at least ``results_device_min_masks`` final masks and they are 0 / 1
        masks of one shape; else by the host statement.  Both give the same dictionary, value for value."""
        self.results_timing = {}
        if self.results_device and len(self.masks_final) >= max(self.results_device_min_masks, 1) and Analyzer.has_gpu(self.model) \
                and self._results_masks_ok():
            return device_or_host("make_json_results_device", self.make_json_results_device, self.make_json_results_host)
        return self.make_json_results_host()

    def _results_from(self, outline_of):
        """The result dictionary; ``outline_of(i)`` gives the pixels [(y, x)] and the vertexes [[(x, y)]] of final mask i, as
        lists in mosaic coordinates."""
        xmin, ymin = self.image_xmin, self.image_ymin
        ny, nx = (self.image.shape if self.image is not None else self.image_shape)[:2]
        results = {"image_id": self.image_id, "objs": []}
        for i in range(len(self.masks_final)):
            class_id = int(self.class_ids_final[i])
            y1, x1, y2, x2 = [int(v) for v in self.bboxes[i]]
            at_edge = (x1 <= 0 or x1 >= nx - 1 or x2 <= 0 or x2 >= nx - 1 or
                       y1 <= 0 or y1 >= ny - 1 or y2 <= 0 or y2 >= ny - 1)
            pixels, vertexes = outline_of(i)
            results["objs"].append({
                "name": 'S' + str(i + 1) + "_" + self.obj_name_tag,
                "x1": xmin + x1, "x2": xmin + x2, "y1": ymin + y1, "y2": ymin + y2,
                "class_id": class_id, "class_name": self.class_names[class_id],
                "score": float(self.scores_final[i]), "pixels": pixels, "vertexes": vertexes, "edge": bool(at_edge)})
        self.results = results

    def make_json_results_device(self):
        """make_json_results_host with find_contours and np.argwhere of all final masks replaced by one ops.mask_plane_outlines
        call on the frame's bit planes -- those extract_det_masks_device left on the device, else one upload and pack of
        masks_final -- and one download."""
        from . import ops
        clock = time.perf_counter
        t0 = clock()
        timing = {"masks": len(self.masks_final), "mask_uploads": 0}
        planes, timing["mask_uploads"] = self._planes_of(self.masks_final)
        t1 = clock()
        got = ops.mask_plane_outlines(planes).host()
        t2 = clock()
        sc, co, po = got["source_contours"].tolist(), got["contour_offsets"].tolist(), got["pixel_offsets"].tolist()
        points = got["points"].astype(np.float64) + np.array([self.image_xmin, self.image_ymin])
        pixels_all = got["pixels"].astype(np.int64) + np.array([self.image_ymin, self.image_xmin])
        self._results_from(lambda i: (pixels_all[po[i]:po[i + 1]].tolist(),
                                      [points[co[k]:co[k + 1]].tolist() for k in range(sc[i], sc[i + 1])]))
        t3 = clock()
        for name, a, b in (("planes", t0, t1), ("outlines_download", t1, t2), ("host_lists", t2, t3)):
            timing[name + "_ms"] = round(1e3 * (b - a), 3)
        self.results_timing = timing

    def make_json_results_host(self):
        xmin, ymin = self.image_xmin, self.image_ymin

        def outline_of(i):
            mask = np.asarray(self.masks_final[i])
            pixels = (np.argwhere(mask == 1) + np.array([ymin, xmin])).tolist()
            padded = np.zeros((mask.shape[0] + 2, mask.shape[1] + 2), dtype=np.uint8)
            padded[1:-1, 1:-1] = mask
            vertexes = []
            for verts in find_contours(padded, 0.5):
                verts = np.fliplr(verts) - 1                      # drop the padding, (y, x) -> (x, y)
                vertexes.append((verts + np.array([xmin, ymin])).tolist())
            return pixels, vertexes
        self._results_from(outline_of)

    def write_json_results(self, outfile):
        if not self.results:
            logger.warning("Result obj dictionary is empty, nothing to be written...")
            return
        with open(outfile, 'w') as fp:
            json.dump(self.results, fp, indent=2, sort_keys=True)

    # ---- the overlay PNG (analyze.py:2039-2135; the raster of DESIGN.md 4.12) -----------------------------------
    def _draw_scene(self):
        """The scene of draw.render_host / draw.device_tables from what predict / inspect_results left, or None (logged) when
        the frame cannot be drawn."""
        if self.image is None:
            logger.error("The image of %s stayed on the device (only its shape is known here): nothing is drawn ..." % self.image_id)
            return None
        image = np.asarray(self.image)
        shape_cfg = np.asarray(getattr(self.config, "IMAGE_SHAPE", (0, 0, 3))).reshape(-1)
        if image.ndim == 3 and image.shape[2] == 1 and image.dtype == np.uint8 and shape_cfg.size >= 3 and int(shape_cfg[2]) == 1:
            image = np.repeat(image, 3, axis=2)           # a gray-level configuration's uint8 frame: drawn as its three-fold copy
        if image.ndim != 3 or image.shape[2] != 3 or image.shape[0] == 0 or image.shape[1] == 0:
            logger.error("Cannot draw an image of shape %r (need [H, W, 3]): nothing is drawn ..." % (tuple(image.shape),))
            return None
        H, W = image.shape[:2]
        scale = overlay.default_scale(H, W) if self.draw_scale is None else int(self.draw_scale)
        if scale < 1:
            logger.error("Invalid draw_scale %r (need an integer >= 1): nothing is drawn ..." % (self.draw_scale,))
            return None
        masks = [np.asarray(m) for m in self.masks_final]
        if any(m.shape != (H, W) for m in masks):
            logger.error("The final masks are not of the image's shape %r: nothing is drawn ..." % ((H, W),))
            return None
        gt_colours = []
        for i in range(len(self.bboxes_gt)):                              # analyze.py:2066-2070
            label = 'bkg'
            if len(self.class_ids_gt_merged) > 0:
                label = self.class_names[self.class_ids_gt_merged[i]]
            gt_colours.append(self.class_color_map.get(label, overlay.UNKNOWN_COLOUR))
        colours, texts = [], []
        for i in range(len(masks)):
            colour = self.class_color_map.get(self.class_names[self.class_ids_final[i]], overlay.UNKNOWN_COLOUR)
            colours.append(colour)
            y1, x1, y2, x2 = [int(v) for v in self.bboxes[i]]
            if self.draw_class_label_in_caption:
                texts.append((str(self.captions[i]), x1, y1 + 8, overlay.colour8(colour)))
            else:
                texts.append(("{:.2f}".format(self.scores_final[i]), x1 + (x2 - x1) // 2 - 4, y1 - 1, overlay.CAPTION_COLOUR))
        return {"image": image, "scale": scale, "shaded": bool(self.draw_shaded_masks), "masks": masks, "colours": colours,
                "boxes": [[int(v) for v in b] for b in self.bboxes[:len(masks)]], "gt_boxes": [[int(v) for v in b] for b in self.bboxes_gt],
                "gt_colours": gt_colours, "texts": texts}

    def _draw_on_device(self, scene):
        """The device form takes the frame: a GPU is there, the image holds 8-bit values, the masks are 0 / 1 masks (bit planes
        hold nothing else) and there are at least draw_device_min_masks of them."""
        if not Analyzer.has_gpu(self.model) or scene["image"].dtype != np.uint8:
            return False
        n = len(scene["masks"])
        return n >= self.draw_device_min_masks and (n == 0 or self._results_masks_ok())

    def _render_device(self, scene):
        import torch
        from . import ops
        clock = time.perf_counter
        t0 = clock()
        timing = {"masks": len(scene["masks"]), "mask_uploads": 0}
        planes = None
        if scene["masks"]:
            planes, timing["mask_uploads"] = self._planes_of(self.masks_final)
        t1 = clock()
        image =torch.from_numpy(np.ascontiguousarray(scene["image"])).to(self._device())
        canvas = ops.draw_overlay(image, planes, overlay.device_tables(scene), scene["scale"])
        torch.cuda.synchronize(canvas.device)
        t2 = clock()
        out = canvas.cpu().numpy()
        t3 = clock()
        for name, a, b in (("planes", t0, t1), ("render", t1, t2), ("download", t2, t3)):
            timing[name + "_ms"] = round(1e3 * (b - a), 3)
        self.draw_timing = timing
        return out

    def render_results(self, device=None):
        """The overlay of the current frame as a uint8 array [s (H + 4), s (W + 4), 3], without writing a file; None (logged) when
        the frame cannot be drawn.  device: None -- on the GPU where ``draw_results`` would render there, with its fallback; True
        -- the device form, errors raised; False -- the host statement."""
        self.draw_timing = {}
        scene = self._draw_scene()
        if scene is None:
            return None
        if device is True:
            return self._render_device(scene)
        if device is None and self._draw_on_device(scene):
            from .ops import DrawUnsupported                              # this scene only (a tiny frame's default scale is above 64)
            return device_or_host("draw_results_device", lambda: self._render_device(scene), lambda: overlay.render_host(scene),
                                  refusal=DrawUnsupported)
        return overlay.render_host(scene)

    def _write_overlay(self, outfile, device):
        canvas = self.render_results(device)
        if canvas is None:
            return -1
        t0 = time.perf_counter()
        overlay.write_png(outfile, canvas)
        self.draw_timing["encode_ms"] = round(1e3 * (time.perf_counter() - t0), 3)
        return 0

    def draw_results(self, outfile):
        """Write the overlay of the current frame -- the frame, the detected masks' contours (shaded with ``draw_shaded_masks``),
        their boxes and scores, the ground-truth boxes -- as an 8-bit RGB PNG: rendered on the GPU (``draw_results_device``) where
        one is there, else by the host statement; both give the same bytes.  0, or -1 when nothing could be drawn."""
        return self._write_overlay(outfile, None)

    def draw_results_device(self, outfile):
        """draw_results with the canvas composed by ops.draw_overlay in one pass, from the bit planes extract_det_masks_device left
        on the device (else one upload and pack of masks_final), and one download."""
        return self._write_overlay(outfile, True)

    def draw_results_host(self, outfile):
        """draw_results by draw.render_host, the NumPy statement of DESIGN.md 4.12."""
        return self._write_overlay(outfile, False)

    # ---- DS9 regions (analyze.py:1960-2030) ----------------------------------------------------------------
    def make_ds9_regions(self, use_polygon=True):
        """One region line per contour (or the bounding box); DS9 image coordinates are 1-based."""
        self.obj_regions = []
        if not self.results or 'objs' not in self.results:
            logger.warning("No result dictionary was filled or no object detected, no region will be produced...")
            return -1
        for o in self.results['objs']:
            dx, dy = o['x2'] - o['x1'], o['y2'] - o['y1']
            xc, yc = o['x1'] + 0.5 * dx, o['y1'] + 0.5 * dy
            tags = "tag={%s}" % o['class_name'] + (" tag={BORDER}" if o['edge'] else "")
            meta = "# text={%s} %s color=%s" % (o['name'], tags, self.class_color_map_ds9.get(o['class_name'], "green"))
            for contour in o['vertexes']:
                if use_polygon:
                    coords = ",".join("%.4f,%.4f" % (x + 1, y + 1) for x, y in contour)
                    self.obj_regions.append("polygon(%s) %s" % (coords, meta))
                else:
                    self.obj_regions.append("box(%.4f,%.4f,%.4f,%.4f,0) %s" % (xc + 1, yc + 1, dx, dy, meta))
        return 0

    def write_ds9_regions(self, outfile):
        if not self.obj_regions:
            logger.warning("Region list with detected objects is empty, nothing to be written...")
            return
        with open(outfile, 'w') as fp:
            fp.write("# Region file format: DS9\nglobal color=green\nimage\n")
            for line in self.obj_regions:
                fp.write(line + "\n")


# ---- the ModelTester (analyze.py:65-406) -----------------------------------------------------------------------
class ModelTester(object):
    """``run.py test`` of the reference: every image of a dataset through ``Analyzer.inspect_results``, the confusion matrix,
    purity, matched scores and IoUs accumulated, and two tables -- one row per true object (completeness.csv) and one per
    detected object (reliability.csv) -- rewritten after every image.  With ``compute_mAP_metrics`` set, compute_mAP (:408-575)
    follows: the per-image mask AP of the reference, the Pascal-VOC box metrics its vendored tool computes from gt_data /
    pred_data (metrics.py; matched on the GPU) and, when ``metrics_outdir`` names a directory, the input files of the three
    external tools under it."""

    def __init__(self, model, config, dataset):
        self.dataset, self.model, self.config = dataset, model, config
        self.n_max_img = -1
        self.remap_classids = False
        self.classid_map = {}
        self.score_thr = 0.7
        self.iou_thr = 0.6
        self.n_classes = dataset.nclasses
        self.classification_matrix = np.zeros((self.n_classes, self.n_classes))
        self.classification_matrix_norm = np.zeros((self.n_classes, self.n_classes))
        self.purity = np.zeros((1, self.n_classes))
        self.nobjs_true = np.zeros((1, self.n_classes))
        self.nobjs_det = np.zeros((1, self.n_classes))
        self.nobjs_det_right = np.zeros((1, self.n_classes))
        self.detobj_scores, self.detobj_ious = [], []
        self.detobj_scoreMean = self.detobj_scoreStdDev = self.detobj_iouMean = self.detobj_iouStdDev = 0
        self.detobj_gtinfo = []
        self.compute_mAP_metrics = False
        self.mAP = 0
        self.APs = []                         # compute_mAP: mask AP at iou_thr per inspected image; mAP is their mean
        self.voc = None                       # compute_mAP: metrics.voc_metrics(gt_data, pred_data, (0.5, iou_thr))
        self.metrics_outdir = None            # compute_mAP: write the external tools' input files under this directory
        self.sweep_map = False                # compute_mAP: also the second vendored tool's numbers (metrics.sweep_metrics)
        self.sweep = None                     # compute_mAP with sweep_map: the precision / recall sweep and the mAP over IoU 0.50 ... 0.95
        self.inspected = []                   # (image_id, image_path) of the images test() went through
        self.completeness_dict_list, self.reliability_dict_list = [], []
        self.outfilename_completeness = "completeness.csv"
        self.outfilename_reliability = "reliability.csv"
        self.eval_device = None               # None: every Analyzer keeps its own default; True / False: set on each of them
        self.components_device = None         # likewise (Analyzer.components_device)
        self.draw = False                     # every Analyzer draws out_<base>_id<uuid>.png (the reference's always do)

    def test(self):
        """:123-185."""
        nimg = 0
        logger.info("Processing up to %d images " % self.n_max_img)
        gt_data, pred_data = [], []
        self.inspected = []
        for index, image_id in enumerate(self.dataset.image_ids):
            if self.n_max_img > 0 and nimg >= self.n_max_img:
                logger.info("Max number of images to inspect reached, stop here.")
                break
            nimg += 1
            image_path = self.dataset.image_info[index]['path']
            image_path_base = os.path.basename(image_path)
            analyzer = Analyzer(self.model, self.config, self.dataset, gt_data, pred_data)
            analyzer.score_thr = self.score_thr
            analyzer.iou_thr = self.iou_thr
            analyzer.remap_classids = self.remap_classids
            analyzer.classid_map = self.classid_map
            if self.eval_device is not None:
                analyzer.eval_device = self.eval_device
            if self.components_device is not None:
                analyzer.components_device = self.components_device
            analyzer.draw = self.draw
            logger.info("Inspecting results for image %s ..." % image_path_base)
            if analyzer.inspect_results(image_id, image_path) < 0:
                logger.error("Failed to analyze results for image %s ..." % image_path_base)
                continue
            self.inspected.append((image_id, image_path))
            self.update_performances(analyzer)
        logger.info("Computing final performances ...")
        self.compute_performances()
        if self.compute_mAP_metrics:
            logger.info("Computing Mean AveragePrecision (mAP) ...")
            self.compute_mAP(gt_data=gt_data, pred_data=pred_data)
        logger.info("Saving result data to file ...")
        self.save()
        return 0

    def update_performances(self, analyzer):
        """:190-322: sums the image's counters and appends its rows to the two tables, key for key."""
        self.classification_matrix += analyzer.confusion_matrix
        self.nobjs_true += analyzer.nobjs_true
        self.nobjs_det += analyzer.nobjs_det
        self.nobjs_det_right += analyzer.nobjs_det_right
        self.detobj_scores += analyzer.detobj_scores
        self.detobj_ious += analyzer.detobj_ious

        image_path = analyzer.image_path
        image_tel = analyzer.image_metadata["telescope"]
        image_rms = analyzer.image_metadata["rms"]
        image_bkg = analyzer.image_metadata["bkg"]
        class_ids_gt = analyzer.class_ids_gt_merged
        objinfo_gt = analyzer.detobj_gtinfo
        scores_det, ious_det = analyzer.detobj_scores, analyzer.detobj_ious
        class_ids_det, class_names_det = analyzer.detobj_classids, analyzer.detobj_class_names
        is_gt_obj_detected = analyzer.is_gt_obj_detected
        if objinfo_gt:
            if len(class_ids_gt) != len(objinfo_gt):
                logger.warning("classids_gt size is different from objinfo_gt size!")
            rows = []
            try:
                for i in range(len(objinfo_gt)):
                    obj = objinfo_gt[i]
                    maxBeamSize, minBeamSize = obj['maxsize_beam'], obj['minsize_beam']
                    aspectRatio = maxBeamSize / minBeamSize
                    d = collections.OrderedDict()
                    d["img"] = image_path
                    d["telescope"] = image_tel
                    d["img_rms"] = image_rms
                    d["img_bkg"] = image_bkg
                    d["sname"] = obj['name']
                    d["class_id"] = class_ids_gt[i]
                    d["class_name"] = obj['class']
                    d["class_id_det"] = class_ids_det[i]
                    d["class_name_det"] = class_names_det[i]
                    d["detected"] = int(is_gt_obj_detected[i])
                    d["score"] = scores_det[i]
                    d["iou"] = ious_det[i]
                    d["snr"] = float(obj['snr'])
                    d["maxBeamSize"] = float(maxBeamSize)
                    d["aspectRatio"] = float(aspectRatio)
                    d["border"] = int(obj['border'])
                    rows.append(d)
            except IndexError:
                # With the sidelobe switch off the per-object lists skip the flagged objects while the object info does not: the
                # reference indexes them with one counter and raises here.  This image's completeness rows are left out.
                logger.error("Object info and per-object results of image %s have different lengths (sources near or mixed with "
                             "sidelobes are not considered): its completeness rows are left out ..." % image_path)
                rows = []
            self.completeness_dict_list.extend(rows)

        objinfo_det = analyzer.det_obj_pars
        class_ids_det, scores_det = analyzer.class_ids_final, analyzer.scores_final
        if objinfo_det:
            if len(class_ids_det) != len(objinfo_det):
                logger.warning("class_ids_det size is different from objinfo_det size!")
            for i in range(len(objinfo_det)):
                obj_det = objinfo_det[i]
                maxBeamSize, minBeamSize = obj_det['maxsize_beam'], obj_det['minsize_beam']
                aspectRatio = -999
                if minBeamSize > 0:
                    aspectRatio = float(maxBeamSize) / float(minBeamSize)
                d = collections.OrderedDict()
                d["img"] = image_path
                d["telescope"] = image_tel
                d["img_rms"] = image_rms
                d["img_bkg"] = image_bkg
                d["sname"] = obj_det['name']
                d["class_id_det"] = class_ids_det[i]
                d["class_name_det"] = obj_det['class']
                d["class_id"] = analyzer.matchobj_classids[i]
                d["class_name"] = analyzer.matchobj_class_names[i]
                d["matching_gt"] = int(analyzer.is_det_obj_matching_to_gt_obj[i])
                d["score"] = float(scores_det[i])
                d["iou"] = float(analyzer.matchobj_ious[i])
                d["snr"] = float(obj_det['snr'])
                d["maxBeamSize"] = float(maxBeamSize)
                d["aspectRatio"] = float(aspectRatio)
                d["border"] = int(obj_det['border'])
                self.reliability_dict_list.append(d)
        self.save()
        return 0

    def save(self):
        """:328-351: "# " and then csv.DictWriter's header and rows in its default dialect."""
        for rows, filename in ((self.completeness_dict_list, self.outfilename_completeness),
                               (self.reliability_dict_list, self.outfilename_reliability)):
            if rows:
                with open(filename, 'w') as fp:
                    fp.write("# ")
                    dict_writer = csv.DictWriter(fp, rows[0].keys())
                    dict_writer.writeheader()
                    dict_writer.writerows(rows)

    def compute_performances(self):
        """:356-406."""
        for i in range(self.n_classes):
            norm = self.nobjs_true[0][i]
            if norm <= 0:
                continue
            for j in range(self.n_classes):
                self.classification_matrix_norm[i][j] = self.classification_matrix[i][j] / norm
        for j in range(self.n_classes):
            if self.nobjs_det[0][j] <= 0:
                continue
            self.purity[0][j] = self.nobjs_det_right[0][j] / self.nobjs_det[0][j]
        self.detobj_scoreMean = np.mean(self.detobj_scores)
        self.detobj_scoreStdDev = np.std(self.detobj_scores)
        self.detobj_iouMean = np.mean(self.detobj_ious)
        self.detobj_iouStdDev = np.std(self.detobj_ious)
        for title, value in (("NOBJ TRUE", self.nobjs_true), ("NOBJ DET", self.nobjs_det), ("NOBJ DET CORRECTLY", self.nobjs_det_right),
                             ("CLASSIFICATION MATRIX", self.classification_matrix),
                             ("CLASSIFICATION MATRIX (NORM)", self.classification_matrix_norm), ("PRECISION (or PURITY)", self.purity)):
            print("== %s ==" % title)
            print(value)
        print("== DET SCORES ==")
        print("scoreThr=%f, <score>=%f, sigma(score)=%f" % (self.score_thr, self.detobj_scoreMean, self.detobj_scoreStdDev))
        print("== DET IOUs ==")
        print("iouThr=%f, <iou>=%f, sigma(iou)=%f" % (self.iou_thr, self.detobj_iouMean, self.detobj_iouStdDev))

    def compute_mAP(self, gt_data, pred_data):
        """:408-575.  (a) Mask AP at iou_thr of every inspected image (the reference's loop stops after the first one, marked TODO
        there: ``APs[0]`` is its value): load_image_gt, detect, utils.compute_ap -- the [P, G] mask overlaps from the device tensor
        the model kept (metrics.mask_ap) where there is one.  (b) The box metrics of the vendored Pascal-VOC tool at IoU 0.5 and
        iou_thr.  (c) The printed block.  (d) With ``sweep_map``, what the second vendored tool (tarlen5-calculate-mean-ap) computes
        from the same rows -- the curve over every score threshold, the mAP over IoU 0.50 ... 0.95, the per-class APs -- and the
        lines it prints (metrics.sweep_metrics, format_sweep).  (e) The external tools' input files, under ``metrics_outdir`` when
        it is set (the reference writes them into the current directory)."""
        from . import datagen, metrics
        self.APs = []
        for image_id, _ in self.inspected:
            image, image_meta, gt_class_id, gt_bbox, gt_mask = datagen.load_image_gt(self.dataset, self.config, image_id,
                                                                                     use_mini_mask=False)
            r = self.model.detect([image], verbose=0)[0]
            kept = getattr(self.model, "last_masks_device", None)
            AP, _, _, _ = metrics.mask_ap(gt_bbox, gt_class_id, gt_mask, r, kept[0] if kept else None, self.iou_thr)
            self.APs.append(AP)
        self.mAP = np.mean(self.APs) if self.APs else float("nan")
        thresholds = tuple(t for t in (0.5, self.iou_thr) if t > 0)
        self.voc = metrics.voc_metrics(gt_data, pred_data, thresholds)
        print("== Mean AveragePrecision (mAP) ==")
        print("mAP=%f" % self.mAP)
        for res in self.voc["results"]:
            for label in self.voc["classes"]:
                c = res["classes"][label]
                print("VOC IoU>=%.2f class %s: AP=%f (positives=%d, TP=%d, FP=%d)" % (
                    res["threshold"], label, c["AP"], c["total positives"], c["total TP"], c["total FP"]))
            print("VOC IoU>=%.2f mAP=%f" % (res["threshold"], res["mAP"]))
        if self.sweep_map:
            self.sweep = metrics.sweep_metrics(gt_data, pred_data)
            for line in metrics.format_sweep(self.sweep):
                print(line)
        if self.metrics_outdir:
            metrics.write_metric_files(gt_data, pred_data, [path for _, path in self.inspected], self.metrics_outdir)
        return 0
