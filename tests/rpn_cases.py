"""Seeded inputs and oracle-side expectations for the size-, count- and tie-dependent branches of csrc/proposal.hip and
csrc/rpn_targets.hip: NumPy + the CPU oracle only.  tests/test_rpn_cases_cpu.py checks, without a GPU, that every case has the
property it exists for and that a plausibly wrong kernel would change its expected output; tests/test_rpn_counts_gpu.py runs the
same cases through ops.proposals(..., debug=True) and ops.rpn_targets.

ProposalLayer cases are of two kinds.  "random": the generators of test_proposal_layer (scores rounded to three decimals, so ties
occur); the kernel's top-k is compared exactly, its boxes at 2e-6 (expf against np.exp), its NMS exactly against the oracle's NMS
re-run on the kernel's boxes.  "exact": anchors on multiples of 1/128 and zero deltas, so decode and clip are exact in float32 and
every IoU is a correctly rounded quotient of exact operands on both sides -- everything is compared bit for bit with the oracle's
own end-to-end proposal_layer."""
import collections
import functools
import zlib

import numpy as np
import torch

import mrcnn_oracle as orc

RPN_BBOX_STD_DEV = np.array([0.1, 0.1, 0.2, 0.2])
SORT_CAP = 8192                 # csrc/proposal.hip: pre_nms_limit and proposal_count above it are refused
PRE_MIN = 32 * 1024             # multi-workgroup pre-selection from this many anchors on (and A > K)
RT_MAXG = 512                   # csrc/rpn_targets.hip: more GT rows are refused


class ProposalCfg(object):
    """What OracleMaskRCNN.proposal_layer reads from its config."""

    def __init__(self, limit, thr):
        self.PRE_NMS_LIMIT, self.RPN_NMS_THRESHOLD, self.RPN_BBOX_STD_DEV = limit, thr, RPN_BBOX_STD_DEV


def _seed(name):
    return zlib.crc32(name.encode())


# =============================================================================================================================
#  ProposalLayer
# =============================================================================================================================
PCase = collections.namedtuple("PCase", "name kind B A limit count thr scores deltas expect ties builder")
PROPOSAL_CASES = collections.OrderedDict()


def _p(name, kind, B, A, limit=6000, count=1000, thr=0.7, scores="random", deltas="random", expect=None, ties=None, builder=None):
    """expect: "runs_out" (the scan ends at the last chunk with fewer than `count` boxes kept, every image), "hits_count" (every
    image stops at `count`) or None (not asserted).  ties: True when the K-th score has more equals than slots in every image (the
    ordered compaction runs), False when in no image, None when not asserted."""
    assert name not in PROPOSAL_CASES
    PROPOSAL_CASES[name] = PCase(name, kind, B, A, limit, count, thr, scores, deltas, expect, ties, builder)


# 1. tiny K: n is padded to 8, count > K -> every survivor, then zero rows
for _i, _A in enumerate((1, 7, 8, 9)):
    _p("tiny_A%d" % _A, "random", (1, 3)[_i % 2], _A, count=10)
# 2. edges of the 64-wide chunks of the scan and tiles of the suppression matrix; K = 64 < A = 200 is a real selection
for _i, _A in enumerate((63, 64, 65, 127, 128, 129)):
    _p("chunk_A%d" % _A, "random", (3, 1)[_i % 2], _A, count=1000 if _A < 100 else 100, expect="runs_out" if _A < 100 else None)
_p("chunk_K64_of_A200", "random", 2, 200, limit=64, expect="runs_out")
# 3. sort network: n = 512 | 1024 (first LDS stage) | 2048; nwords 64 -> 65 (first use of rem1); SORT_CAP
for _i, _K in enumerate((511, 512, 513, 1023, 1024, 1025)):
    _p("sort_K%d" % _K, "random", (1, 3)[_i % 2], _K + 37, limit=_K)
_p("sort_K4096", "random", 1, 4096 + 37, limit=4096, count=2000)
_p("sort_K4097", "random", 2, 4097 + 37, limit=4097, count=2000)
_p("sort_K8192_A8192", "random", 1, 8192, limit=8192, count=8192, expect="runs_out")
_p("sort_K8192_A9000", "random", 1, 9000, limit=8192, count=2000)
# 4. selection paths: cached (A <= 16 384), uncached single workgroup (< 32 768; 25 575 is a 320 x 320 image), multi-workgroup
#    (>= 32 768), chunk > 4096 (A > 262 144; 409 200 is a 1280 x 1280 image)
for _A, _B in ((1023, 3), (1024, 1), (1025, 2), (16384, 2), (16385, 1), (25575, 2), (32767, 1), (32768, 2), (262144, 1), (262145, 2),
               (409200, 1)):
    _p("path_A%d" % _A, "random", _B, _A, ties=True if _A >= 16384 else None)
# 5. limit == A (no selection: everything is sorted) and limit == A - 1
_p("limit_A6000", "random", 2, 6000)
_p("limit_A6001", "random", 1, 6001)
_p("limit_A32768_K8192", "random", 1, 32768, limit=8192, ties=True)
# 6. ties
_p("ties_equal_A5000", "random", 1, 5000, scores="equal", ties=False)        # K = A: everything taken, order = anchor index
_p("ties_equal_A16368", "random", 2, 16368, scores="equal", ties=True)       # cached: s_base carried over 16 iterations
_p("ties_equal_A20000", "random", 1, 20000, scores="equal", ties=True)       # uncached
_p("ties_two_A16368", "random", 1, 16368, scores="two", ties=True)
_p("ties_two_A20000", "random", 1, 20000, scores="two", ties=True)
_p("ties_two_A40000", "random", 1, 40000, scores="two", ties=True)           # topk_collect_kernel's carry (256-anchor iterations)
_p("ties_zero_one", "random", 3, 7000, scores="zero_one")                    # image 0 all 0.0, image 1 all distinct, image 2 all 1.0
# 8. decode extremes
_p("decode_extremes", "random", 2, 3000, deltas="extreme")

# the last tie taken by the "two" cases: anchor index, stated here and checked in tests/test_rpn_cases_cpu.py.  4912 = 4 * 1024 + 12 * 64
# + 48 and 4904 = 4 * 1024 + 12 * 64 + 40: fifth 1024-anchor iteration of select_sort_decode_kernel, wave 12, lanes 48 and 40.
# 4680 = 4000 + 2 * 256 + 2 * 64 + 40: second workgroup of topk_collect_kernel (chunk = 4000), its third 256-anchor iteration,
# wave 2, lane 40.
TIES_TWO_LAST_TAKEN = {"ties_two_A16368": 4912, "ties_two_A20000": 4904, "ties_two_A40000": 4680}
TIES_TWO_HIGH = {"ties_two_A16368": 1520, "ties_two_A20000": 1500, "ties_two_A40000": 1500}     # anchors above the tie value


def _random_scene(rng, B, A):
    """anchors, foreground scores and deltas as test_proposal_layer draws them"""
    ctr = rng.uniform(0, 1, (A, 2)); sz = np.exp(rng.uniform(np.log(0.02), np.log(0.5), (A, 2)))
    anchors = np.concatenate([ctr - sz / 2, ctr + sz / 2], 1).astype(np.float32)
    fg = np.round(1 / (1 + np.exp(-rng.normal(0, 2, (B, A)))), 3)
    deltas = (rng.standard_normal((B, A, 4)) * 0.5).astype(np.float32)
    return anchors, fg, deltas


def _extreme_deltas(rng, B, A):
    """Scaled deltas (delta * RPN_BBOX_STD_DEV) up to +-20, a third of the anchors in the size terms, a third in the centre terms,
    the rest ordinary.  Never both in one anchor: the float32 corner y2 = (cy - h/2) + h carries the rounding of h, and h = a_h *
    exp(d) differs between expf and np.exp by a few units in its last place -- 2e-6 covers that for h <= ~4 only.  With an
    ordinary centre (inside [-1, 2]) every box higher than 4 has both corners clipped; with an extreme centre and an ordinary
    size the box is small and lies wholly outside the window.  |scaled delta| stays far below 80, where float32 exp overflows
    (inf - inf = NaN in the reference, dropped by the kernel's fminf / fmaxf: see DESIGN.md)."""
    d = rng.standard_normal((B, A, 4)) * 0.5
    kind = rng.integers(0, 3, (B, A))
    big = rng.uniform(-20, 20, (B, A, 4)) / RPN_BBOX_STD_DEV
    big[:, 0, :] = np.array([20, -20, 20, -20]) / RPN_BBOX_STD_DEV          # the ends of the range themselves: anchor 0 in its size
    big[:, 1, :] = -big[:, 0, :]                                            # terms, anchor 1 in its centre terms
    kind[:, 0], kind[:, 1] = 1, 2
    d[..., 2:] = np.where((kind == 1)[..., None], big[..., 2:], d[..., 2:])
    d[..., :2] = np.where((kind == 2)[..., None], big[..., :2], d[..., :2])
    return d.astype(np.float32)


def _grid_boxes(cells, cell, inset):
    """boxes [n,4] in units of 1/128: cell (i, j) of a grid of `cell`-unit squares, shrunk by `inset` on every side"""
    cells = np.asarray(cells)
    y, x = cells[:, 0] * cell, cells[:, 1] * cell
    return np.stack([y + inset, x + inset, y + cell - inset, x + cell - inset], 1).astype(np.float64)


def _exact_from_sorted(rng, boxes_sorted, B=1):
    """Anchors = boxes_sorted / 128 in a shuffled order (so top_idx is no identity), scores (n - position) / 8192: distinct and
    exact in float32, position p of the sorted order holds boxes_sorted[p]."""
    n = boxes_sorted.shape[0]
    assert n < 8192
    perm = rng.permutation(n)                        # anchor perm[p] holds the box of sorted position p
    anchors = np.zeros((n, 4), np.float32)
    anchors[perm] = (boxes_sorted / 128.0).astype(np.float32)
    fg = np.zeros((B, n), np.float64)
    fg[:, perm] = (n - np.arange(n)) / 8192.0
    return anchors, fg


CHAIN = np.array([[64, 0, 96, 32], [64, 4, 96, 36], [64, 8, 96, 40]], np.float64)     # IoU(a,b) = IoU(b,c) = 7/9, IoU(a,c) = 0.6
CHAIN_POSITIONS = {"nms_chain_K200": (10, 70, 130), "nms_chain_K4200": (100, 2000, 4150)}
DISJOINT_COUNTS = (1, 63, 64, 65, 128, 199, 200, 201, 300)


def _b_disjoint(rng):
    cells = [(i, j) for i in range(16) for j in range(16)]
    cells = [cells[i] for i in rng.permutation(256)[:200]]
    return _exact_from_sorted(rng, _grid_boxes(cells, 8, 1))


def _b_clusters(rng):
    cells = [(i, j) for i in range(16) for j in range(16)]
    cells = [cells[i] for i in rng.permutation(256)[:70]]
    return _exact_from_sorted(rng, np.tile(_grid_boxes(cells, 8, 1), (3, 1)))        # sorted order: clusters 0..69, three times


def _b_identical(rng):
    return _exact_from_sorted(rng, np.tile(np.array([[16, 16, 80, 80]], np.float64), (150, 1)))


def _b_overlap(rng):
    n = 300
    h, w = rng.integers(4, 41, n), rng.integers(4, 41, n)
    y1, x1 = rng.integers(0, 129 - h), rng.integers(0, 129 - w)
    boxes = np.stack([y1, x1, y1 + h, x1 + w], 1).astype(np.float64)
    boxes = np.concatenate([boxes, boxes[rng.integers(0, n, 20)]])                     # 20 exact duplicates (IoU == 1)
    return _exact_from_sorted(rng, boxes[rng.permutation(len(boxes))])


def _b_zero_area(rng):
    out = []
    for k in range(20):                                           # pairs of IDENTICAL boxes outside the window: above / left / below / right
        off = [(-48 - k, 10 + k), (20 + k, -40 - k), (130 + k, 30 + k), (50 + k, 129 + k)][k % 4]
        out += [[off[0], off[1], off[0] + 24, off[1] + 24]] * 2
    part = []
    for k in range(20):                                           # across a window edge or corner: clipped
        y1, x1 = [(-10, 8 * k), (8 * k, -12), (118, 6 * k), (6 * k, 116)][k % 4]
        part.append([y1, x1, y1 + 24, x1 + 24])
    n = 120
    h, w = rng.integers(8, 41, n), rng.integers(8, 41, n)
    y1, x1 = rng.integers(0, 129 - h), rng.integers(0, 129 - w)
    inside = np.stack([y1, x1, y1 + h, x1 + w], 1)
    boxes = np.concatenate([np.array(out), np.array(part), inside]).astype(np.float64)
    return _exact_from_sorted(rng, boxes[rng.permutation(len(boxes))])


def _b_chain(rng, K, positions):
    cells = [(i, j) for i in range(64) for j in range(128)]      # unit cells of the upper half; the chain lives in the lower half
    fill = _grid_boxes([cells[i] for i in rng.permutation(len(cells))[:K - 3]], 1, 0)
    boxes = np.zeros((K, 4))
    rest = np.ones(K, bool); rest[list(positions)] = False
    boxes[list(positions)] = CHAIN
    boxes[rest] = fill
    return _exact_from_sorted(rng, boxes)


# 7. NMS counts, exact
for _c in DISJOINT_COUNTS:     # (a) every chunk is "clean": popcount(alive) <= maxk - total with equality (64, 128, 200) and one short (63, 199)
    _p("nms_disjoint_c%d" % _c, "exact", 1, 200, count=_c, builder="disjoint", expect="hits_count" if _c <= 200 else "runs_out")
_p("nms_clusters_c300", "exact", 1, 210, count=300, builder="clusters", expect="runs_out")      # (b), (g): 70 kept, all four chunks scanned
_p("nms_clusters_c50", "exact", 1, 210, count=50, builder="clusters", expect="hits_count")
_p("nms_identical", "exact", 1, 150, count=10, builder="identical", expect="runs_out")          # (c): one survivor
_p("nms_thr0", "exact", 1, 320, thr=0.0, builder="overlap", expect="runs_out")                  # (d)
_p("nms_thr1", "exact", 1, 320, thr=1.0, builder="overlap", expect="runs_out")
_p("nms_zero_area", "exact", 1, 180, builder="zero_area", expect="runs_out")                    # (e)
_p("nms_chain_K200", "exact", 1, 200, builder="chain", expect="runs_out")                       # (f)
_p("nms_chain_K4200", "exact", 1, 4200, count=5000, builder="chain", expect="runs_out")         # (f) through rem1, (g): all 66 chunks

PROPOSAL_RANDOM = [c.name for c in PROPOSAL_CASES.values() if c.kind == "random"]
PROPOSAL_EXACT = [c.name for c in PROPOSAL_CASES.values() if c.kind == "exact"]
# the workspace-reuse sequence (one stream, grow-only buffer): the lower-triangular words of the bit matrix are never written, so
# the later calls find the earlier calls' data in them
PROPOSAL_REUSE_SEQUENCE = ("reuse_A65472", "path_A1023", "sort_K4097", "reuse_A65472")
_p("reuse_A65472", "random", 2, 65472)
# host-side refusals (limit, count): K > SORT_CAP, proposal_count > SORT_CAP
PROPOSAL_REFUSALS = ((9000, 8193, 1000), (9000, 6000, 8193))       # (A, limit, count)


def proposal_inputs(name):
    """-> dict(probs [B,A,2], deltas [B,A,4], anchors [A,4], fg [B,A] float32, K) of a case, as float32 NumPy"""
    c = PROPOSAL_CASES[name]
    seed_name = name.rsplit("_c", 1)[0] if c.builder in ("disjoint", "clusters") else name      # one scene for all its counts
    rng = np.random.default_rng(_seed(seed_name))
    if c.kind == "exact":
        if c.builder == "chain":
            anchors, fg = _b_chain(rng, c.A, CHAIN_POSITIONS[name])
        else:
            anchors, fg = {"disjoint": _b_disjoint, "clusters": _b_clusters, "identical": _b_identical, "overlap": _b_overlap,
                           "zero_area": _b_zero_area}[c.builder](rng)
        deltas = np.zeros((c.B, c.A, 4), np.float32)
    else:
        anchors, fg, deltas = _random_scene(rng, c.B, c.A)
        if c.scores == "equal":
            fg[:] = 0.5
        elif c.scores == "two":
            fg[:] = 0.25
            for b in range(c.B):
                fg[b, rng.permutation(c.A)[:TIES_TWO_HIGH[name]]] = 0.75
        elif c.scores == "zero_one":
            fg[0] = 0.0
            fg[1] = rng.permutation(c.A) / float(c.A - 1)         # distinct in float32 (A < 2^13), 0.0 and 1.0 among them
            fg[2] = 1.0
        if c.deltas == "extreme":
            deltas = _extreme_deltas(rng, c.B, c.A)
    assert anchors.shape == (c.A, 4) and fg.shape == (c.B, c.A)
    probs = np.stack([1 - fg, fg], -1).astype(np.float32)
    return dict(probs=probs, deltas=deltas, anchors=anchors, fg=probs[..., 1], K=min(c.limit, c.A))


@functools.lru_cache(maxsize=2)
def proposal_reference(name):
    """The oracle end to end: (rois [B,count,4], [(top_idx, boxes, keep)] per image)"""
    c = PROPOSAL_CASES[name]
    d = proposal_inputs(name)
    o = orc.OracleMaskRCNN(ProposalCfg(c.limit, c.thr), {})
    return o.proposal_layer(torch.tensor(d["probs"]), torch.tensor(d["deltas"]), d["anchors"], c.count, detail=True)


def threshold_ties(fg, K):
    """(cnt_eq, need_eq) of one image: how many scores equal the K-th largest, and how many of those belong to the top K"""
    v = np.sort(fg)[::-1][K - 1]
    return int((fg == v).sum()), int(K - (fg > v).sum())


def proposal_expected_status(name):
    """{collected, announced, refused} of ops.proposal_status after a healthy call"""
    c = PROPOSAL_CASES[name]
    K = min(c.limit, c.A)
    return (K, K, 0) if (c.A >= PRE_MIN and c.A > K) else (0, 0, 0)


# =============================================================================================================================
#  RPN targets
# =============================================================================================================================
ANCHOR_SCALES, ANCHOR_RATIOS, BACKBONE_STRIDES = (4, 8, 16, 32, 64), [0.5, 1, 2], [4, 8, 16, 32, 64]      # run_py_config's


@functools.lru_cache(maxsize=None)
def pyramid_anchors(S):
    """float64 pixel anchors of an S x S image: A = 258, 1023, 4092, 16 368 at S = 32, 64, 128, 256"""
    return orc.generate_pyramid_anchors(ANCHOR_SCALES, ANCHOR_RATIOS, orc.compute_backbone_shapes(BACKBONE_STRIDES, (S, S)),
                                        BACKBONE_STRIDES, 1)


def _random_gt(rng, S, n, hi):
    boxes = np.zeros((n, 4), np.int32)
    for g in range(n):
        h, w = rng.integers(2, min(hi, S - 1), 2)
        y1, x1 = rng.integers(0, S - h), rng.integers(0, S - w)
        boxes[g] = (y1, x1, y1 + h, x1 + w)
    return boxes, rng.integers(1, 4, n).astype(np.int32)


def _rpn_scene(seed_name, S, G, counts, n_train, hi=90, last_rows=False, keys="uniform"):
    rng = np.random.default_rng(_seed(seed_name))
    anchors = pyramid_anchors(S)
    B, A = len(counts), anchors.shape[0]
    cls = np.zeros((B, G), np.int32); boxes = np.zeros((B, G, 4), np.int32)
    for b, n in enumerate(counts):
        rows = slice(G - n, G) if last_rows else slice(0, n)
        boxes[b, rows], cls[b, rows] = _random_gt(rng, S, n, hi)
    k = rng.uniform(0, 1, (B, A)).astype(np.float32)
    if keys == "equal":
        k[:] = 0.5
    elif keys == "zero":
        k[:] = 0.0
    elif keys == "three":
        k = rng.choice(np.array([0.25, 0.5, 0.75], np.float32), (B, A))
    return dict(S=S, anchors=anchors, gt_cls=cls, gt_boxes=boxes, keys=k, n_train=n_train)


# the exact-threshold scene: the ratio-1 scale-32 anchors of a 256 x 256 image are the squares [c - 16, c + 16]^2, c a multiple of
# 32 -- integer corners, area 1024.  A GT of the same rows, `width` columns wide, of which `overlap` lie inside the anchor:
#   width 36, overlap 28: 896 / 1280 = 0.7 (float64 division of exact operands: the double nearest 0.7, i.e. the literal)
#   width 20, overlap 12: 384 / 1280 = 0.3
# and one pixel either side of both.  (anchor centre y, x; width; overlap)
THRESHOLD_GTS = (("iou_0.7", 32, 64, 36, 28), ("iou_0.7-", 32, 192, 36, 27), ("iou_0.7+", 96, 64, 36, 29),
                 ("iou_0.3", 96, 192, 20, 12), ("iou_0.3-", 160, 64, 20, 11), ("iou_0.3+", 160, 192, 20, 13))


def threshold_anchor_index(cy, cx):
    a = pyramid_anchors(256)
    hit = np.where((a == np.array([cy - 16, cx - 16, cy + 16, cx + 16], np.float64)).all(1))[0]
    assert hit.size == 1
    return int(hit[0])


def _thresholds_scene():
    s = _rpn_scene("thresholds", 256, 8, [0], 2 * 16368)            # n_train above every count: nothing is dropped
    for g, (_, cy, cx, width, overlap) in enumerate(THRESHOLD_GTS):
        x1 = cx + 16 - overlap
        s["gt_boxes"][0, g] = (cy - 16, x1, cy + 16, x1 + width)
        s["gt_cls"][0, g] = 1 + g % 3
    return s


def _empties_scene():
    """[no GT, ordinary, only crowds, ordinary with one crowd]"""
    s = _rpn_scene("empties", 128, 8, [0, 4, 3, 5], 64)
    s["gt_cls"][2, :3] = -1
    s["gt_cls"][3, 1] = -2
    return s


_CAPS_BASE = dict(seed_name="caps", S=128, G=12, counts=[7])
_SMALL32 = dict(seed_name="small_A258", S=32, G=8, counts=[5])
RPN_SCENES = collections.OrderedDict([
    # 1. small A: per-thread chunk of 1, trailing threads with an empty range
    ("small_A258", lambda: _rpn_scene(n_train=64, **_SMALL32)),
    ("small_A1023", lambda: _rpn_scene("small_A1023", 64, 8, [5, 3, 6, 4], 64)),
    ("small_A4092", lambda: _rpn_scene("small_A4092", 128, 12, [7], 64)),
    # 2. G
    ("g1", lambda: _rpn_scene("g1", 64, 1, [1], 64)),
    ("g512_full", lambda: _rpn_scene("g512_full", 64, 512, [512], 256, hi=40)),
    ("g512_last_rows", lambda: _rpn_scene("g512_last_rows", 64, 512, [5], 64, last_rows=True)),
    # 3. n_train
    ("ntrain_1", lambda: _rpn_scene(n_train=1, **_SMALL32)),
    ("ntrain_2", lambda: _rpn_scene(n_train=2, **_SMALL32)),
    ("ntrain_7", lambda: _rpn_scene(n_train=7, **_SMALL32)),
    ("ntrain_512_A258", lambda: _rpn_scene(n_train=512, **_SMALL32)),
    # 4. caps exactly (n_train from the uncapped counts P0, N0 of the scene: rpn_caps_ntrain)
    ("caps_pos_exact", lambda: _rpn_scene(n_train=rpn_caps_ntrain("caps_pos_exact"), **_CAPS_BASE)),
    ("caps_pos_drop1", lambda: _rpn_scene(n_train=rpn_caps_ntrain("caps_pos_drop1"), **_CAPS_BASE)),
    ("caps_neg_exact", lambda: _rpn_scene(n_train=rpn_caps_ntrain("caps_neg_exact"), **_CAPS_BASE)),
    ("caps_neg_drop1", lambda: _rpn_scene(n_train=rpn_caps_ntrain("caps_neg_drop1"), **_CAPS_BASE)),
    # 5. keys
    ("keys_equal", lambda: _rpn_scene("keys", 128, 32, [7, 30], 32, keys="equal")),
    ("keys_zero", lambda: _rpn_scene("keys", 128, 32, [7, 30], 32, keys="zero")),
    ("keys_three_values", lambda: _rpn_scene("keys_three_values", 256, 300, [150], 256, hi=40, keys="three")),
    # 6. exact thresholds
    ("thresholds", _thresholds_scene),
    # 7. no GT, only crowds
    ("empties", _empties_scene),
])
RPN_REUSE_SEQUENCE = ("keys_three_values", "small_A258", "keys_three_values")     # 256^2, 32^2, 256^2: colmax is cleared per call, arg is not
RPN_KEY_TIE_SCENES = ("keys_equal", "keys_zero", "keys_three_values")


def rpn_scene(name):
    return RPN_SCENES[name]()


@functools.lru_cache(maxsize=None)
def rpn_uncapped_counts():
    """(P0, N0) of the caps scene: positives and negatives before any is dropped"""
    s = _rpn_scene(n_train=2 * 4092, **_CAPS_BASE)
    m, _ = rpn_expected_image(s["anchors"], s["gt_cls"][0], s["gt_boxes"][0], s["keys"][0], s["n_train"])
    return int((m == 1).sum()), int((m == -1).sum())


def rpn_caps_ntrain(name):
    P0, N0 = rpn_uncapped_counts()
    assert N0 > P0 + 2 > 4
    return {"caps_pos_exact": 2 * P0,           # P == half: no positive dropped
            "caps_pos_drop1": 2 * P0 - 2,       # half = P0 - 1: exactly one dropped
            "caps_neg_exact": P0 + N0,          # half >= P0, N == n_train - P: no negative dropped
            "caps_neg_drop1": P0 + N0 - 1}[name]   # N one more than that: drop_smallest with drop = 1


def rpn_expected_without_gt(anchors, cls, boxes, keys, n_train):
    """No instance among the GT rows (none at all, or crowds only).  The reference cannot say: np.argmax over an empty axis raises.
    The device kernel extends it the way the engine tests assume ("negatives only"): every anchor that passes the crowd test
    (crowd IoU < 0.001) is a negative candidate, the surplus over n_train is dropped by the keyed draw, no box targets."""
    crowd = boxes[cls < 0]
    ok = np.ones(anchors.shape[0], bool)
    if crowd.shape[0]:
        ok = np.amax(orc.compute_overlaps(anchors, crowd), axis=1) < 0.001
    match = np.zeros(anchors.shape[0], np.int32)
    match[ok] = -1
    ids = np.where(match == -1)[0]
    if len(ids) > n_train:
        match[orc.KeyedChoice(keys).choice(ids, len(ids) - n_train)] = 0
    return match, np.zeros((n_train, 4))


def rpn_expected_image(anchors, cls, boxes, keys, n_train, rng=None):
    """(rpn_match [A], rpn_bbox [n_train,4] float64) of one image"""
    if not (cls > 0).any():
        return rpn_expected_without_gt(anchors, cls, boxes, keys, n_train)
    nz = cls != 0
    return orc.build_rpn_targets(anchors, cls[nz], boxes[nz], n_train, RPN_BBOX_STD_DEV, rng=rng or orc.KeyedChoice(keys))


def rpn_expected(s):
    return [rpn_expected_image(s["anchors"], s["gt_cls"][b], s["gt_boxes"][b], s["keys"][b], s["n_train"])
            for b in range(s["gt_cls"].shape[0])]


def rpn_uncapped_match(s, b):
    """rpn_match of image b before the two draws (n_train above every count)"""
    return rpn_expected_image(s["anchors"], s["gt_cls"][b], s["gt_boxes"][b], s["keys"][b], 2 * s["anchors"].shape[0])[0]
