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


