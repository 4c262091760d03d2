"""Seeded inputs shared by the GPU parity tests and the host-side checks of their preconditions: pure NumPy + the CPU oracle, so
a test that needs no GPU can rebuild exactly what a GPU test feeds its kernel."""
import numpy as np

import mrcnn_oracle as orc


def _rand(rng, *shape, scale=1.0):
    return (rng.standard_normal(shape) * scale).astype(np.float32)


def _random_rois(rng, B, R, zero_tail=0):
    """log-uniform sizes covering all four pyramid levels, some ROIs touching the border."""
    size = np.exp(rng.uniform(np.log(0.01), np.log(0.9), (B, R, 2)))
    ctr = rng.uniform(0, 1, (B, R, 2))
    y1 = np.clip(ctr[..., 0] - size[..., 0] / 2, 0, 1); y2 = np.clip(ctr[..., 0] + size[..., 0] / 2, 0, 1)
    x1 = np.clip(ctr[..., 1] - size[..., 1] / 2, 0, 1); x2 = np.clip(ctr[..., 1] + size[..., 1] / 2, 0, 1)
    rois = np.stack([y1, x1, y2, x2], -1).astype(np.float32)
    if zero_tail:
        rois[:, -zero_tail:] = 0
    return rois


# (NUM_CLASSES, seed, logit scale) of test_detection_layer_class_counts: the flatter the softmax over more classes, the larger
# the scale that still leaves the oracle more than 10 detections with a score >= 0.5
# (tests/test_host_cpu.py::test_class_count_preconditions_of_gpu_cases checks it without a GPU)
DETECTION_CLASS_CASES = [(2, 22, 2.0), (6, 23, 3.0), (17, 24, 4.0)]


def detection_layer_inputs(num_classes, seed, logit_scale):
    """rois [B,R,4], probs [B,R,C] (rounded to two digits: score ties), deltas [B,R,C,4], windows [B,4] of the detection-layer tests."""
    rng = np.random.default_rng(seed)
    B, R, C = 2, 1000, num_classes
    rois = _random_rois(rng, B, R, zero_tail=50)
    lg = _rand(rng, B, R, C, scale=logit_scale)
    probs = np.exp(lg) / np.exp(lg).sum(-1, keepdims=True)
    probs = np.round(probs, 2).astype(np.float32)            # score ties
    deltas = _rand(rng, B, R, C, 4, scale=0.5)
    windows = np.array([[0, 0, 1, 1], [0.1, 0.05, 0.9, 0.95]], np.float32)
    return rois, probs, deltas, windows


def losses_inputs(num_classes, cycle):
    """NumPy operands of the loss tests.  cycle: target classes 1 .. C-1 in turn over the positive rows (every foreground class
    occurs) instead of drawn at random.  One inactive class: with two classes the foreground one -- the random logits leave the
    argmax on the (active) background for about half of the rows, so the normaliser sum(pred_active) stays positive."""
    rng = np.random.default_rng(41)
    B, A, T, C = 2, 4092, 64, num_classes
    d = {}
    d["rpn_match"] = rng.choice([-1, 0, 1], size=(B, A, 1), p=[0.1, 0.85, 0.05]).astype(np.int32)
    maxpos = int((d["rpn_match"] == 1).sum(1).max()) + 5
    d["rpn_bbox_t"] = _rand(rng, B, maxpos, 4)
    d["rpn_logits"] = _rand(rng, B, A, 2, scale=2)
    d["rpn_bbox"] = _rand(rng, B, A, 4, scale=1.5)
    tcls = np.zeros((B, T), np.int32); tcls[:, :20] = rng.integers(1, C, (B, 20))
    if cycle:
        tcls[:, :20] = 1 + np.arange(20) % (C - 1)
        assert set(tcls[0].tolist()) == set(range(C)) and set(tcls[1].tolist()) == set(range(C))
    d["tcls"] = tcls
    d["tbbox"] = _rand(rng, B, T, 4); d["tmask"] = (rng.uniform(0, 1, (B, T, 28, 28)) > 0.5).astype(np.float32)
    active = np.ones((B, C), np.int32); active[:, min(2, C - 1)] = 0
    d["active"] = active
    d["logits"] = _rand(rng, B, T, C, scale=2)
    d["mbbox"] = _rand(rng, B, T, C, 4, scale=1.5)
    mm = rng.uniform(0, 1, (B, T, 28, 28, C)).astype(np.float32); mm[0, 0, 0, :4, :] = [[0.0] * C, [1.0] * C, [1e-9] * C, [0.5] * C]
    d["mmask"] = mm
    d["pred_active"] = active[0][d["logits"].reshape(-1, C).argmax(1)]
    return d


# ---- engine-level scenes (tests/test_engine_gpu.py, tests/test_h16_gpu.py, the smoke run) ----------------------------------------
def _small_cfg(backbone="custom", size=128, mode="training", num_classes=4, **kw):
    from caesar_mrcnn_amd.config import run_py_config
    cfg = run_py_config(num_classes=num_classes, backbone=backbone, imgsize=size, mode=mode)
    cfg.POST_NMS_ROIS_TRAINING = 1500
    cfg.POST_NMS_ROIS_INFERENCE = 200
    cfg.TRAIN_ROIS_PER_IMAGE = 48
    cfg.MAX_GT_INSTANCES = 20
    cfg.RPN_TRAIN_ANCHORS_PER_IMAGE = 64
    cfg.DETECTION_MAX_INSTANCES = 30
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def _scene(cfg, B, seed):
    """Synthetic tiles: noise + bright boxes.  Every GT instance is laid over a (pixel-rounded) anchor of
    scale >= 8 px so that, with RPN deltas kept small, some proposals reach IoU >= 0.5 and the
    detection-target / mask / bbox branches are exercised."""
    rng = np.random.default_rng(seed)
    S = int(cfg.IMAGE_SHAPE[0])
    G = cfg.MAX_GT_INSTANCES
    anchors = orc.generate_pyramid_anchors(cfg.RPN_ANCHOR_SCALES, cfg.RPN_ANCHOR_RATIOS,
                                           orc.compute_backbone_shapes(cfg.BACKBONE_STRIDES, cfg.IMAGE_SHAPE),
                                           cfg.BACKBONE_STRIDES, cfg.RPN_ANCHOR_STRIDE)
    ok = np.where((anchors[:, 0] >= 0) & (anchors[:, 1] >= 0) & (anchors[:, 2] <= S) & (anchors[:, 3] <= S) &
                  ((anchors[:, 2] - anchors[:, 0]) >= 6) & ((anchors[:, 3] - anchors[:, 1]) >= 6))[0]
    images = rng.normal(0, 8, (B, S, S, 3)).astype(np.float32) + 20
    gt_masks = np.zeros((B, S, S, G), bool)
    gt_boxes = np.zeros((B, G, 4), np.int32)
    gt_cls = np.zeros((B, G), np.int32)
    for b in range(B):
        for g in range(G - 4 - b):
            y1, x1, y2, x2 = np.round(anchors[rng.choice(ok)]).astype(int)
            gt_masks[b, y1:y2, x1:x2, g] = True
            gt_masks[b, (y1 + y2) // 2, (x1 + x2) // 2, g] = False
            images[b, y1:y2, x1:x2] += rng.uniform(60, 200)
            gt_boxes[b, g] = [y1, x1, y2, x2]
            gt_cls[b, g] = rng.integers(1, cfg.NUM_CLASSES)
    return images, gt_cls, gt_boxes, gt_masks


def _train_inputs(cfg, B, seed):
    images, gt_cls, gt_boxes, gt_masks = _scene(cfg, B, seed)
    anchors_px = orc.generate_pyramid_anchors(cfg.RPN_ANCHOR_SCALES, cfg.RPN_ANCHOR_RATIOS,
                                              orc.compute_backbone_shapes(cfg.BACKBONE_STRIDES, cfg.IMAGE_SHAPE),
                                              cfg.BACKBONE_STRIDES, cfg.RPN_ANCHOR_STRIDE)
    rng = np.random.RandomState(seed)
    rpn_match = np.zeros((B, anchors_px.shape[0], 1), np.int32)
    rpn_bbox = np.zeros((B, cfg.RPN_TRAIN_ANCHORS_PER_IMAGE, 4), np.float32)
    for b in range(B):
        n = int((gt_cls[b] > 0).sum())
        m, bb = orc.build_rpn_targets(anchors_px, gt_cls[b, :n], gt_boxes[b, :n], cfg.RPN_TRAIN_ANCHORS_PER_IMAGE,
                                      cfg.RPN_BBOX_STD_DEV, rng)
        rpn_match[b, :, 0], rpn_bbox[b] = m, bb
    meta = np.stack([orc.compose_image_meta(b, images[b].shape, images[b].shape, (0, 0) + images[b].shape[:2], 1.0,
                                            np.ones(cfg.NUM_CLASSES, np.int32)) for b in range(B)])
    keys = np.random.default_rng(seed + 1).uniform(0, 1, (B, cfg.POST_NMS_ROIS_TRAINING)).astype(np.float32)
    return [images, meta, rpn_match, rpn_bbox, gt_cls, gt_boxes, gt_masks], keys


def _weights(cfg, seed, damp=None):
    """damp: factor on the BatchNorm gamma that closes every bottleneck branch.  ResNet-101 sums 33 residual branches;
    with unit-scale random branches the activations grow ~2x in variance per block and the RPN saturates (all proposals
    clip to the full tile, no positive ROI): 0.25 keeps the trunk's output in range so that every branch of the training
    graph carries signal."""
    from caesar_mrcnn_amd.params import ParamLayout, init_weights, deconv_gemm_to_keras
    w = init_weights(ParamLayout(cfg), seed=seed, perturb_bn=True)
    if damp is not None:
        for k in w:
            if k.endswith("_branch2c/gamma"):
                w[k] = w[k] * np.float32(damp)
    w["mrcnn_mask_deconv/kernel"] = deconv_gemm_to_keras(w["mrcnn_mask_deconv/kernel"])   # Keras layout at the boundary
    # keep RPN box deltas small so proposals stay near their anchors and some reach IoU >= 0.5 with the GT
    w["rpn_bbox_pred/kernel"] = w["rpn_bbox_pred/kernel"] * np.float32(0.02)
    w["rpn_bbox_pred/bias"] = w["rpn_bbox_pred/bias"] * np.float32(0.02)
    return w


# ---- count-dependent cases: empty sides, boundaries and caps of losses / detection targets / detection layer ------------------------
# (tests/test_counts_gpu.py feeds them to the kernels; tests/test_host_cpu.py checks their preconditions with the oracle alone)
LOSS_GROUP = 32 * 1024          # anchors per register group of rpn_loss_reduce_kernel (RPN_MAXIT slices of 1024 anchors)
LOSS_TOL = dict(rtol=2e-5, atol=1e-6)      # the five losses (tolerances of _losses_case)
GRAD_TOL = dict(rtol=1e-4, atol=1e-7)      # their gradients
LOSS_GRADS = ("rpn_logits", "rpn_bbox", "logits", "mbbox", "mmask")
LOSS_WEIGHTS = [1.0, 0.5, 1.0, 2.0, 1.5]
RANK_CASE_ANCHORS = (33797, 98309)         # two groups, the last of 1029 anchors (a ragged slice); four groups, the last of 5 anchors


def losses_rank_inputs(A, seed=43):
    """The loss operands with A > 32 768 anchors: the positive rank runs through several register groups of the RPN kernel.
    Per image 200 positives and 300 negatives (at most 256 / 512 non-neutral anchors, as build_rpn_targets leaves), every other
    anchor neutral.  Image 0 has no positive in its first group and some in every later one, image 1 some in every group but its
    last, which has none; positives are planted on both sides of every group edge, on anchor 0 and on anchor A - 1 (in the image that may hold them; a
    negative in the other).
    rpn_bbox_t has distinct random rows: a rank that is off by one pairs every later positive with the wrong row."""
    d = losses_inputs(4, False)
    rng = np.random.default_rng(seed)
    B, NPOS, NNEG = 2, 200, 300
    ngroups = -(-A // LOSS_GROUP)
    assert ngroups >= 2
    match = np.zeros((B, A), np.int32)
    edges = sorted({0, A - 1} | {g * LOSS_GROUP - 1 for g in range(1, ngroups)} | {g * LOSS_GROUP for g in range(1, ngroups)})
    for b in range(B):
        groups = range(1, ngroups) if b == 0 else range(0, ngroups - 1)
        planted = [a for a in edges if a // LOSS_GROUP in groups]
        match[b, planted] = 1
        left = NPOS - len(planted)
        for k, g in enumerate(groups):                      # the rest spread evenly over this image's groups, the surplus of a
            lo, hi = g * LOSS_GROUP, min((g + 1) * LOSS_GROUP, A)        # short last group going to the first
            free = np.setdiff1d(np.arange(lo, hi), planted)
            n = min(left // len(groups), len(free) // 2)
            match[b, rng.choice(free, n, replace=False)] = 1
        g = groups[0]
        free = np.where(match[b, g * LOSS_GROUP:(g + 1) * LOSS_GROUP] == 0)[0] + g * LOSS_GROUP
        match[b, rng.choice(free, NPOS - int((match[b] == 1).sum()), replace=False)] = 1
        match[b, [a for a in edges if match[b, a] == 0]] = -1          # negatives on the planted anchors the positives left
        free = np.where(match[b] == 0)[0]
        match[b, rng.choice(free, NNEG - int((match[b] == -1).sum()), replace=False)] = -1
    d["rpn_match"] = match[:, :, None].copy()
    d["rpn_bbox_t"] = _rand(rng, B, NPOS + 5, 4)
    d["rpn_logits"] = _rand(rng, B, A, 2, scale=2)
    d["rpn_bbox"] = _rand(rng, B, A, 4, scale=1.5)
    return d


def rank_case_group_positives(d):
    """[B, groups] positives of every register group of the RPN loss kernel."""
    m = d["rpn_match"][:, :, 0]
    A = m.shape[1]
    return np.array([[int((m[b, g0:g0 + LOSS_GROUP] == 1).sum()) for g0 in range(0, A, LOSS_GROUP)] for b in range(m.shape[0])])


def rpn_bbox_loss_statement(d, shift_group=None, weight=LOSS_WEIGHTS[1]):
    """float64 statement of rpn_bbox_loss (mrcnn/model.py:1140-1170) and of weight * d loss / d rpn_bbox with the ranks written
    out: the k-th positive anchor of an image, in anchor order, is paired with row k of that image's rpn_bbox_t.
    shift_group: the deliberately wrong statement -- ranks of the anchors of that register group one too high (a lost carry)."""
    m = d["rpn_match"][:, :, 0]
    B, A = m.shape
    q, t = d["rpn_bbox"].astype(np.float64), d["rpn_bbox_t"].astype(np.float64)
    grad = np.zeros_like(q)
    total, count = 0.0, 0
    for b in range(B):
        pos = np.where(m[b] == 1)[0]
        rank = np.arange(len(pos))
        if shift_group is not None:
            rank = rank + (pos // LOSS_GROUP == shift_group)
        ok = rank < t.shape[1]
        pos, rank = pos[ok], rank[ok]
        e = q[b, pos] - t[b, rank]
        a = np.abs(e)
        total += np.where(a < 1, 0.5 * a * a, a - 0.5).sum()
        count += len(pos)
        grad[b, pos] = np.where(a < 1, e, np.sign(e))
    if count == 0:
        return 0.0, grad
    return total / (count * 4), grad * (weight / (count * 4))


EMPTY_SIDE_CASES = ("a", "b", "c", "d", "e", "f", "g")


def losses_empty_inputs(case):
    """losses_inputs(4, False) with one side of the losses emptied:
    a  no positive anchor (the positives turned negative)          e  exactly one positive ROI, in the last row
    b  every anchor neutral                                        f  all T rows positive
    c  image 1: every anchor neutral, image 0 unchanged            g  no active class (the class loss is 0 / 0)
    d  no positive ROI"""
    d = losses_inputs(4, False)
    rng = np.random.default_rng(47)
    C = d["logits"].shape[-1]
    m = d["rpn_match"]
    if case == "a":
        m[m == 1] = -1
    elif case == "b":
        m[:] = 0
    elif case == "c":
        m[1] = 0
    elif case == "d":
        d["tcls"][:] = 0
    elif case == "e":
        d["tcls"][:] = 0
        d["tcls"][-1, -1] = 2
    elif case == "f":
        d["tcls"][:] = rng.integers(1, C, d["tcls"].shape)
    elif case == "g":
        d["active"][:] = 0
        d["pred_active"] = d["active"][0][d["logits"].reshape(-1, C).argmax(1)]
    else:
        raise ValueError(case)
    return d


def losses_surplus_inputs():
    """losses_inputs(4, False) with rpn_bbox_t cut to three rows fewer than the image with more positives has: the kernel leaves the
    surplus positives (the last ones in anchor order) out of the box loss and keeps them in the class loss.
    Returns (d, match_box): match_box is rpn_match with the surplus positives set to -1, the match that gives the box loss."""
    d = losses_inputs(4, False)
    m = d["rpn_match"]
    npos = (m[:, :, 0] == 1).sum(1)
    M = int(npos.max()) - 3
    d["rpn_bbox_t"] = np.ascontiguousarray(d["rpn_bbox_t"][:, :M])
    match_box = m.copy()
    for b in range(m.shape[0]):
        pos = np.where(m[b, :, 0] == 1)[0]
        match_box[b, pos[M:], 0] = -1
    return d, match_box


def losses_reference(cfg, d, rpn_match_box=None, weights=LOSS_WEIGHTS):
    """The five oracle losses of the operands d and the gradients of their weighted sum, as NumPy (a gradient of None: zeros).
    rpn_match_box: a second match from which the RPN box loss and its gradient are taken instead (losses_surplus_inputs)."""
    import torch
    o = orc.OracleMaskRCNN(cfg, {})

    def run(match):
        t = {n: torch.tensor(d[n], requires_grad=True) for n in LOSS_GRADS}
        bbox_t = d["rpn_bbox_t"]
        short = int((match[:, :, 0] == 1).sum(1).max()) - bbox_t.shape[1]
        if short > 0:            # the oracle wants a row for every positive; only the (discarded) box loss of the full match reads these
            assert rpn_match_box is not None and match is d["rpn_match"]
            bbox_t = np.concatenate([bbox_t, np.zeros((bbox_t.shape[0], short, 4), np.float32)], 1)
        ls = o.losses(match, bbox_t, t["rpn_logits"], t["rpn_bbox"], d["tcls"], d["tbbox"], d["tmask"], d["active"],
                      t["logits"], t["mbbox"], t["mmask"])
        total = sum(wi * li for wi, li in zip(weights, ls))
        if total.requires_grad:
            total.backward()
        grads = {n: (np.zeros(d[n].shape, np.float32) if t[n].grad is None else t[n].grad.numpy()) for n in LOSS_GRADS}
        return np.array([float(l.detach()) for l in ls]), grads

    ls, grads = run(d["rpn_match"])
    if rpn_match_box is not None:
        ls2, grads2 = run(rpn_match_box)
        ls[1], grads["rpn_bbox"] = ls2[1], grads2["rpn_bbox"]
    return ls, grads


def assert_losses_close(got_losses, got_grads, ref_losses, ref_grads, names=LOSS_GRADS, which=range(5)):
    """The comparison of the loss tests: LOSS_TOL on the losses `which`, GRAD_TOL on the gradients `names`; NaN equals NaN."""
    which = list(which)
    np.testing.assert_allclose(np.asarray(got_losses, np.float64)[which], np.asarray(ref_losses, np.float64)[which], **LOSS_TOL)
    for n in names:
        np.testing.assert_allclose(got_grads[n], ref_grads[n], err_msg="d_" + n, **GRAD_TOL)


def tolerance_fractions(got_losses, got_grads, ref_losses, ref_grads):
    """Worst |got - ref| / (atol + rtol |ref|) over the five losses and over the five gradients (1.0 = at the tolerance)."""
    def frac(g, r, rtol, atol):
        g, r = np.asarray(g, np.float64), np.asarray(r, np.float64)
        ok = np.isfinite(r)
        return float(np.max(np.abs(g[ok] - r[ok]) / (atol + rtol * np.abs(r[ok])))) if ok.any() else 0.0
    return (frac(got_losses, ref_losses, **LOSS_TOL), max(frac(got_grads[n], ref_grads[n], **GRAD_TOL) for n in LOSS_GRADS))


# ---- detection targets ---------------------------------------------------------------------------------------------------------
DT_SCENES = ("sweep", "layout", "thresholds", "scarce", "no_gt", "only_crowds", "zero_proposals", "single", "caps", "equal_keys",
             "zero_keys", "t48", "t512")
DT_MINI_SCENES = ("layout", "thresholds")          # also run with USE_MINI_MASK
LAYOUT_INSTANCES, LAYOUT_CROWD, LAYOUT_DUPLICATE, LAYOUT_DROPPED = (1, 4), 3, 6, 8


def _iou32(a, b):
    """overlaps_graph for two boxes in float32, in the oracle's operation order."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    inter = max(min(a[3], b[3]) - max(a[1], b[1]), np.float32(0)) * max(min(a[2], b[2]) - max(a[0], b[0]), np.float32(0))
    return np.float32(inter / ((a[2] - a[0]) * (a[3] - a[1]) + (b[2] - b[0]) * (b[3] - b[1]) - inter))


def _far_rois(rng, n):
    """boxes inside [0.6, 1]^2: no overlap with anything in [0, 0.55]^2"""
    y1, x1 = rng.uniform(0.6, 0.9, (2, n))
    h, w = rng.uniform(0.02, 0.09, (2, n))
    return np.stack([y1, x1, y1 + h, x1 + w], 1).astype(np.float32)


def _layout_scene(rng, B, R, T, hw, keys=None):
    """GT rows at non-contiguous indices (LAYOUT_*): zero rows 0, 2, 5, 7; instances 1, 4; a crowd 3; row 6 an instance with the box
    of row 4; row 8 a non-zero box of class 0 (dropped by both sides).  Every plane a different random mask, every row its own class
    (the zero rows too: a class without a box is ignored)."""
    G = 9
    gt_boxes = np.zeros((B, G, 4), np.float32)
    gt_cls = np.zeros((B, G), np.int32)
    props = np.zeros((B, R, 4), np.float32)
    for b in range(B):
        boxes = {1: (0.05, 0.05, 0.22, 0.25), 4: (0.30, 0.08, 0.50, 0.24), 3: (0.05, 0.32, 0.25, 0.52), 8: (0.32, 0.32, 0.50, 0.50)}
        for g, bx in boxes.items():
            gt_boxes[b, g] = np.asarray(bx, np.float32) + np.float32(0.01 * b)
        gt_boxes[b, 6] = gt_boxes[b, 4]
        gt_cls[b] = [3, 1, 2, -1, 2, 1, 3, 2, 0]
        near = {1: 30, 4: 30, 3: 25, 8: 25}                              # jittered proposals around each of those boxes
        rows = rng.permutation(R)
        k = 0
        for g, n in near.items():
            props[b, rows[k:k + n]] = np.clip(gt_boxes[b, g] + rng.normal(0, 0.012, (n, 4)), 0, 1).astype(np.float32)
            k += n
        nfar = R - k - 10                                                # ten zero rows stay, somewhere
        props[b, rows[k:k + nfar]] = _far_rois(rng, nfar)
    gt_masks = (rng.uniform(0, 1, (B, hw, hw, G)) < 0.5).astype(np.uint8)
    if keys is None:
        keys = rng.uniform(0, 1, (B, R)).astype(np.float32)
    return dict(props=props, gt_cls=gt_cls, gt_boxes=gt_boxes, gt_masks=gt_masks, keys=keys, T=T)


def detection_target_scene(name, mini=False):
    """Seeded operands of ops.detection_targets / OracleMaskRCNN.detection_targets for the scene `name` (DT_SCENES):
    props [B,R,4], gt_cls [B,G], gt_boxes [B,G,4], gt_masks [B,H,W,G] uint8, keys [B,R], T.  mini: 56 x 56 mini-mask planes."""
    rng = np.random.default_rng(500 + DT_SCENES.index(name))
    hw = 56 if mini else 64
    if name == "sweep":
        # image b holds exactly b positives (copies of a GT box, IoU 1) at random rows; every other proposal is far from every GT
        B, R, G, T = 69, 512, 8, 200
        gt_boxes = np.zeros((B, G, 4), np.float32); gt_cls = np.zeros((B, G), np.int32)
        gt_boxes[:, 0] = (0.05, 0.05, 0.2, 0.25); gt_boxes[:, 1] = (0.3, 0.1, 0.5, 0.2); gt_boxes[:, 2] = (0.1, 0.35, 0.3, 0.5)
        gt_cls[:, :3] = (1, 2, 3)
        props = np.zeros((B, R, 4), np.float32)
        for b in range(B):
            rows = rng.permutation(R)
            props[b, rows[:b]] = gt_boxes[b, rng.integers(0, 3, b)]
            props[b, rows[b:R - 6]] = _far_rois(rng, R - 6 - b)          # six zero rows
        gt_masks = (rng.uniform(0, 1, (B, 32, 32, G)) < 0.5).astype(np.uint8)
        return dict(props=props, gt_cls=gt_cls, gt_boxes=gt_boxes, gt_masks=gt_masks,
                    keys=rng.uniform(0, 1, (B, R)).astype(np.float32), T=T)
    if name in ("layout", "t48", "t512"):
        return _layout_scene(rng, 2, 300, {"layout": 200, "t48": 48, "t512": 512}[name], hw)
    if name == "equal_keys":                                             # selection by lowest row alone
        return _layout_scene(rng, 2, 300, 48, hw, keys=np.full((2, 300), 0.5, np.float32))
    if name == "zero_keys":                                              # keys of exactly 0.0 come first, by lowest row
        keys = rng.uniform(0, 1, (2, 300)).astype(np.float32)
        keys[:, ::3] = 0.0
        return _layout_scene(rng, 2, 300, 48, hw, keys=keys)
    if name == "thresholds":
        # row 0: float32 IoU of exactly 0.5 with the GT -> positive; row 1: its neighbour just below -> negative;
        # rows 2 / 3: IoU with the crowd just above / just below 0.001 -> left out of / taken into the negatives
        B, R, G, T = 1, 24, 4, 200
        gt_boxes = np.zeros((B, G, 4), np.float32); gt_cls = np.zeros((B, G), np.int32)
        gt_boxes[0, 0] = (0, 0, 0.25, 0.25); gt_cls[0, 0] = 1
        gt_boxes[0, 1] = (0.5, 0.5, 0.75, 0.75); gt_cls[0, 1] = -1
        props = np.zeros((B, R, 4), np.float32)
        props[0, 0] = (0, 0, 0.25, 0.125)
        props[0, 1] = (0, 0, 0.25, np.nextafter(np.float32(0.125), np.float32(0)))
        # a 0.25 x 0.25 box reaching h into the crowd from below has IoU h / (0.5 - h): walk y1 float by float over the threshold
        box = lambda y1: np.array([y1, 0.5, y1 + np.float32(0.25), 0.75], np.float32)
        y1 = np.float32(0.75 - 0.0005 / 1.001)
        while _iou32(box(y1), gt_boxes[0, 1]) >= np.float32(0.001):
            y1 = np.nextafter(y1, np.float32(1))
        while _iou32(box(y1), gt_boxes[0, 1]) < np.float32(0.001):
            y1 = np.nextafter(y1, np.float32(0))
        props[0, 2] = box(y1)
        props[0, 3] = box(np.nextafter(y1, np.float32(1)))
        props[0, 4:14] = gt_boxes[0, 0]                                  # ten plain positives: P = 11, 22 negatives wanted
        y1, x1 = rng.uniform(0.3, 0.45, (2, 8))                          # eight plain negatives, clear of GT and crowd; rows 22, 23 zero
        props[0, 14:22] = np.stack([y1, x1, y1 + 0.04, x1 + 0.04], 1).astype(np.float32)
        gt_masks = (rng.uniform(0, 1, (B, hw, hw, G)) < 0.5).astype(np.uint8)
        return dict(props=props, gt_cls=gt_cls, gt_boxes=gt_boxes, gt_masks=gt_masks,
                    keys=rng.uniform(0, 1, (B, R)).astype(np.float32), T=T)
    if name == "scarce":
        # 20 positives ask for 40 negatives; 7 are eligible, the other proposals lie inside the crowd or are zero rows
        B, R, G, T = 1, 100, 4, 200
        gt_boxes = np.zeros((B, G, 4), np.float32); gt_cls = np.zeros((B, G), np.int32)
        gt_boxes[0, 1] = (0.1, 0.1, 0.3, 0.3); gt_cls[0, 1] = 2
        gt_boxes[0, 2] = (0.6, 0.6, 1.0, 1.0); gt_cls[0, 2] = -1
        props = np.zeros((B, R, 4), np.float32)
        rows = rng.permutation(R)
        props[0, rows[:20]] = np.clip(gt_boxes[0, 1] + rng.normal(0, 0.005, (20, 4)), 0, 1).astype(np.float32)
        y1, x1 = rng.uniform(0.35, 0.5, (2, 7))
        props[0, rows[20:27]] = np.stack([y1, x1, y1 + 0.05, x1 + 0.04], 1).astype(np.float32)
        props[0, rows[27:90]] = _far_rois(rng, 63)                       # inside the crowd box
        gt_masks = (rng.uniform(0, 1, (B, hw, hw, G)) < 0.5).astype(np.uint8)
        return dict(props=props, gt_cls=gt_cls, gt_boxes=gt_boxes, gt_masks=gt_masks,
                    keys=rng.uniform(0, 1, (B, R)).astype(np.float32), T=T)
    if name in ("no_gt", "only_crowds", "zero_proposals"):
        s = _layout_scene(rng, 2, 300, 200, hw)
        if name == "no_gt":
            s["gt_boxes"][:] = 0
        elif name == "only_crowds":
            s["gt_cls"] = -np.abs(s["gt_cls"])
        else:
            s["props"][:] = 0
        return s
    if name == "single":                                                 # R = 1: the one proposal is a positive
        B, R, G, T = 2, 1, 3, 200
        gt_boxes = np.zeros((B, G, 4), np.float32); gt_cls = np.zeros((B, G), np.int32)
        gt_boxes[:, 1] = (0.2, 0.3, 0.6, 0.7); gt_cls[:, 1] = (1, 3)
        props = (gt_boxes[:, 1:2] + np.float32([[[0.01, -0.01, 0.0, 0.02]], [[0.0, 0.0, 0.0, 0.0]]])).astype(np.float32)
        gt_masks = (rng.uniform(0, 1, (B, hw, hw, G)) < 0.5).astype(np.uint8)
        return dict(props=props, gt_cls=gt_cls, gt_boxes=gt_boxes, gt_masks=gt_masks,
                    keys=rng.uniform(0, 1, (B, R)).astype(np.float32), T=T)
    if name == "caps":                                                   # R = DT_CAP, G = DT_GCAP, the GT in the last rows
        B, R, G, T = 1, 2048, 512, 200
        gt_boxes = np.zeros((B, G, 4), np.float32); gt_cls = np.zeros((B, G), np.int32)
        gt_boxes[0, 508] = (0.05, 0.32, 0.25, 0.52); gt_cls[0, 508] = -1
        gt_boxes[0, 509] = (0.05, 0.05, 0.22, 0.25); gt_boxes[0, 510] = (0.30, 0.08, 0.50, 0.24); gt_boxes[0, 511] = (0.32, 0.32, 0.5, 0.5)
        gt_cls[0, 509:] = (1, 2, 3)
        props = _far_rois(rng, R)[None].copy()
        rows = rng.permutation(R - 1)
        for k, g in enumerate((508, 509, 510, 511)):
            props[0, rows[k * 40:(k + 1) * 40]] = np.clip(gt_boxes[0, g] + rng.normal(0, 0.012, (40, 4)), 0, 1).astype(np.float32)
        props[0, R - 1] = gt_boxes[0, 511]                               # the last proposal row is a positive of the last GT row
        gt_masks = np.zeros((B, 64, 64, G), np.uint8)
        gt_masks[..., 500:] = (rng.uniform(0, 1, (B, 64, 64, 12)) < 0.5)
        return dict(props=props, gt_cls=gt_cls, gt_boxes=gt_boxes, gt_masks=gt_masks,
                    keys=rng.uniform(0, 1, (B, R)).astype(np.float32), T=T)
    raise ValueError(name)


def detection_target_cfg(T, mini=False):
    from caesar_mrcnn_amd.config import run_py_config
    cfg = run_py_config(num_classes=4)
    cfg.TRAIN_ROIS_PER_IMAGE = T
    cfg.USE_MINI_MASK = mini
    return cfg


_dt_cache = {}


def detection_target_case(name, mini=False):
    """(scene, cfg, per-image oracle results) of a scene, computed once and shared: callers leave the arrays unchanged."""
    if (name, mini) not in _dt_cache:
        s = detection_target_scene(name, mini)
        cfg = detection_target_cfg(s["T"], mini)
        o = orc.OracleMaskRCNN(cfg, {})
        ref = [o.detection_targets(s["props"][b], s["gt_cls"][b], s["gt_boxes"][b], s["gt_masks"][b].astype(bool), s["keys"][b])
               for b in range(s["props"].shape[0])]
        _dt_cache[(name, mini)] = (s, cfg, ref)
    return _dt_cache[(name, mini)]


def roi_rows(rois, box):
    """rows of rois [T,4] equal to box"""
    return np.where((rois == np.asarray(box, np.float32)).all(1))[0]


def check_detection_target_case(name, mini=False):
    """The preconditions of a scene, from the oracle side alone: the counts and the edge each scene is there for.  Returns the
    oracle's (P, N) per image."""
    s, cfg, ref = detection_target_case(name, mini)
    T = s["T"]
    quota = int(T * cfg.ROI_POSITIVE_RATIO)
    counts = [r[4] for r in ref]
    for (rois, cls, tb, tm, (P, N)) in ref:
        assert rois.shape == (T, 4) and P + N <= T and P <= quota
        assert not rois[P + N:].any() and not cls[P:].any() and not tb[P:].any() and not tm[P:].any()
    if name == "sweep":
        assert T == 200 and quota == 66
        assert [c[0] for c in counts] == [min(b, 66) for b in range(69)]
        Ns = [c[1] for c in counts[:67]]
        r = np.float32(1.0 / cfg.ROI_POSITIVE_RATIO)
        assert Ns == [int(np.float32(r * np.float32(P))) - P for P in range(67)]
        # the float32 truncation steps: N = int(P / 0.33) - P gains 2 per positive and a third one each time P / 0.33 passes a whole
        # number, once per 33 positives -- at P = 33 and at P = 66, the two places a quota of 66 leaves room for
        steps = np.diff(Ns)
        assert np.where(steps == 3)[0].tolist() == [32, 65] and set(steps.tolist()) == {2, 3}, steps
        assert (Ns[32], Ns[33], Ns[65], Ns[66]) == (64, 67, 131, 134)
    elif name in ("layout", "t48", "t512", "equal_keys", "zero_keys"):
        for b, (rois, cls, tb, tm, (P, N)) in enumerate(ref):
            assert P >= 15 and N >= 30
            want = {int(s["gt_cls"][b, g]) for g in LAYOUT_INSTANCES}
            assert set(cls[:P].tolist()) == want, (set(cls[:P].tolist()), want)      # never the duplicate's (row 6) or the dropped row's class
            assert tm[:P].any() and (tm[:P] == 0).any()
        if name == "t48":
            assert all(c == (15, 30) for c in counts), counts                       # saturated: the quota binds
        if name in ("layout", "t512"):
            assert all(c[0] < quota for c in counts), counts                        # P below the quota
        if name == "equal_keys":
            assert len(set(s["keys"].reshape(-1).tolist())) == 1
        if name == "zero_keys":
            assert (s["keys"] == 0).sum() >= 100
    elif name == "thresholds":
        rois, cls, tb, tm, (P, N) = ref[0]
        p, gt, crowd = s["props"][0], s["gt_boxes"][0, 0], s["gt_boxes"][0, 1]
        assert _iou32(p[0], gt) == np.float32(0.5) and np.float32(0.49999) < _iou32(p[1], gt) < np.float32(0.5)
        assert np.float32(0.001) <= _iou32(p[2], crowd) < np.float32(0.0010005)
        assert np.float32(0.0009995) < _iou32(p[3], crowd) < np.float32(0.001)
        assert (P, N) == (11, 10)                                        # ten of 22 wanted: rows 1, 3 and the eight plain ones
        assert len(roi_rows(rois[:P], p[0])) == 1 and len(roi_rows(rois[P:P + N], p[1])) == 1
        assert len(roi_rows(rois, p[2])) == 0 and len(roi_rows(rois[P:P + N], p[3])) == 1
    elif name == "scarce":
        assert counts == [(20, 7)], counts
    elif name in ("no_gt", "only_crowds", "zero_proposals"):
        assert all(c == (0, 0) for c in counts), counts
        if name != "zero_proposals":
            assert s["props"].any()
    elif name == "single":
        assert s["props"].shape[1] == 1 and counts == [(1, 0), (1, 0)]
        assert [int(r[1][0]) for r in ref] == [1, 3] and all(r[3][0].any() for r in ref)
    elif name == "caps":
        rois, cls, tb, tm, (P, N) = ref[0]
        assert s["props"].shape[1] == 2048 and s["gt_boxes"].shape[1] == 512
        assert P == 66 and N == T - 66 and set(cls[:P].tolist()) == {1, 2, 3}
    else:
        raise ValueError(name)
    return counts


def layout_compacted_planes(s):
    """The layout scene's GT masks as a kernel that indexed the planes by the compacted GT index would see them: the plane of the
    k-th instance (in row order) moved to that instance's original row."""
    m = s["gt_masks"].copy()
    for b in range(m.shape[0]):
        nz = np.abs(s["gt_boxes"][b]).sum(1) != 0
        inst = np.where(nz & (s["gt_cls"][b] > 0))[0]
        for k, g in enumerate(inst):
            m[b, :, :, g] = s["gt_masks"][b, :, :, k]
    return m


# ---- detection layer -------------------------------------------------------------------------------------------------------------
# (R, candidates per image, DETECTION_MAX_INSTANCES, DETECTION_MIN_CONFIDENCE).  Rows below the candidate count are forced to a
# foreground class, the others to background: nvalid of the kernels is that count exactly (with a confidence threshold: at most).
DETECTION_COUNT_CASES = [
    (1000, (0, 0), 100, 0), (1000, (1, 1), 100, 0), (1000, (63, 63), 100, 0), (1000, (64, 64), 100, 0), (1000, (65, 65), 100, 0),
    (1000, (128, 128), 100, 0), (1000, (129, 129), 100, 0),
    (1000, (0, 65), 100, 0),                 # an empty image next to a two-chunk one in one launch
    (1000, (0, 0), 100, 0.5),                # every ROI background, with the confidence filter on
    (1000, (1000, 1000), 100, 1.01),         # a threshold above every score
    (1, (1, 1), 100, 0), (63, (63, 63), 100, 0),
    (2048, (2048, 2048), 100, 0),            # R = DET_CAP: 32 words per row
    (2048, (2048, 2048), 2048, 0),           # ... and the scan goes through all 32 chunks
    (1000, (129, 129), 200, 0),              # max_instances larger than the survivors: a zero tail
    (1000, (129, 129), 20, 0),               # max_instances smaller: the scan stops in mid-chunk
]


def detection_count_inputs(R, n, seed=21):
    """detection_layer_inputs(4, seed, 2.0) cut (R <= 1000) or repeated with other seeds (R = 2048) to R rows; in image b the first
    n[b] rows are forced to a foreground class (background and best foreground probability swapped), the others to background."""
    parts, have = [], 0
    while have < R:
        parts.append(detection_layer_inputs(4, seed + 100 * len(parts), 2.0))
        have += parts[-1][0].shape[1]
    rois, probs, deltas = (np.ascontiguousarray(np.concatenate([p[i] for p in parts], 1)[:, :R]) for i in range(3))
    windows = parts[0][3]
    for b in range(rois.shape[0]):
        bg = np.where(probs[b, :n[b]].argmax(1) == 0)[0]
        fg = 1 + probs[b, bg, 1:].argmax(1)
        top = probs[b, bg, 0].copy()
        probs[b, bg, 0] = np.minimum(probs[b, bg, fg], top - np.float32(0.01))      # strictly below: a tie would stay background
        probs[b, bg, fg] = top
        probs[b, n[b]:, 0] = 1.0
    return rois, probs, deltas, windows


def detection_candidates(cfg, rois, probs, deltas, window):
    """The refined boxes of one image's candidates (foreground, score >= DETECTION_MIN_CONFIDENCE) in the kernels' order: score
    descending, then ROI index.  Their number is nvalid."""
    cls = probs.argmax(1)
    score = probs[np.arange(len(cls)), cls]
    ok = cls > 0
    if cfg.DETECTION_MIN_CONFIDENCE:
        ok &= score >= cfg.DETECTION_MIN_CONFIDENCE
    idx = np.where(ok)[0]
    idx = idx[np.argsort(-score[idx], kind="stable")]
    d = deltas[idx, cls[idx]] * cfg.BBOX_STD_DEV.astype(np.float32)
    return orc.clip_boxes_np(orc.apply_box_deltas_np(rois[idx], d.astype(np.float32)), window).astype(np.float32)


_det_cache = {}


def detection_count_case(R, n, maxi, minconf):
    """(inputs, cfg, oracle detections per image, nvalid per image) of one DETECTION_COUNT_CASES entry, computed once and shared;
    asserts the case's preconditions from the oracle side."""
    key = (R, n, maxi, minconf)
    if key in _det_cache:
        return _det_cache[key]
    from caesar_mrcnn_amd.config import run_py_config
    cfg = run_py_config(mode="inference", num_classes=4)
    cfg.DETECTION_MAX_INSTANCES, cfg.DETECTION_MIN_CONFIDENCE = maxi, minconf
    inp = detection_count_inputs(R, n)
    rois, probs, deltas, windows = inp
    o = orc.OracleMaskRCNN(cfg, {})
    ref, nvalid = [], []
    for b in range(rois.shape[0]):
        det = o.refine_detections(rois[b], probs[b], deltas[b], windows[b])
        cand = detection_candidates(cfg, rois[b], probs[b], deltas[b], windows[b])
        kept = int((det[:, 4] > 0).sum())
        assert det.shape == (maxi, 6) and kept <= min(len(cand), maxi) and not det[kept:].any()
        if minconf == 0:
            assert len(cand) == n[b], (len(cand), n[b])
        if minconf > 1:
            assert probs.max() < minconf and len(cand) == 0 and n[b] == R
        if maxi == 200:
            assert 0 < kept < maxi                                       # the zero tail
        if maxi == 20:                                                   # the cut: survivors dropped, and inside a chunk of 64
            assert kept == maxi
            last = np.where((cand == det[kept - 1, :4]).all(1))[0]
            assert len(last) == 1 and last[0] % 64 != 63 and last[0] + 1 < len(cand), last
            cfg.DETECTION_MAX_INSTANCES = R
            full = o.refine_detections(rois[b], probs[b], deltas[b], windows[b])
            cfg.DETECTION_MAX_INSTANCES = maxi
            after = [np.where((cand == row[:4]).all(1))[0][0] for row in full[maxi:int((full[:, 4] > 0).sum())]]
            assert after and min(after) // 64 == last[0] // 64, (after[:3], last)      # a survivor of the same chunk is cut
        if (R, maxi) == (2048, 2048):
            assert len(cand) > 31 * 64 and kept > 100                    # 32 chunks, every word of the removed-bit row in use
        if n[b] >= 63 and minconf == 0:
            assert kept >= 10
        ref.append(det)
        nvalid.append(len(cand))
    _det_cache[key] = (inp, cfg, ref, nvalid)
    return _det_cache[key]
