"""Gray-level models and float32 images on the GPU: mrcnn_mold_image_f32 against the host statement (MaskRCNN.mold_inputs and
the graph's float32 cast) bit for bit; the stem convolution at Cin = 1, forward and weight gradient, against the oracle; the
staged inference / training comparison of tests/test_engine_gpu.py on a one-channel model; detect() on float32 and gray images,
device-molded against host-molded; the tiled source finder's batched front end on float32 RGB and gray tiles; run.py --grayimg."""
import glob
import json
import logging
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

import mrcnn_oracle as orc
import sfinder_cases as cases
import sfinder_tiles_cases as tc
from model_cases import _rand, _scene, _small_cfg, _train_inputs, _weights

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

F32 = dict(rtol=2e-4, atol=2e-4)     # tests/test_kernels_gpu.py: fp32 contractions with a different summation order


def _gray_cfg(backbone="custom", size=128, mode="training", channels=1, **kw):
    cfg = _small_cfg(backbone, size, mode=mode, **kw)
    cfg.IMAGE_CHANNEL_COUNT = channels
    cfg.IMAGE_SHAPE = np.array([size, size, channels])
    cfg.MEAN_PIXEL = 0 if channels == 1 else np.array([0.0, 0.0, 0.0])
    return cfg


# ---- mold parity -------------------------------------------------------------------------------------------------------
# (h, w), resize mode, min_dim = max_dim, what the shape is there for
MOLD_SHAPES = [
    ((64, 64), "square", 64, "unscaled, canvas = image"),
    ((40, 33), "square", 64, "scaled to 64 x 53, left pad 5, right pad 6"),
    ((5, 7), "square", 64, "scaled by 64 / 7"),
    ((1, 1), "square", 64, "one pixel to 64 x 64"),
    ((100, 70), "pad64", 64, "unscaled, padded to 128 x 128"),
    ((37, 41), "none", 64, "canvas of 1517 pixels: no multiple of 4, scalar stores"),
    ((70, 90), "square", 128, "scaled, 6300 pixels: several workgroups in the min / max pass"),
    ((200, 150), "square", 128, "scaled DOWN (the image is larger than the canvas)"),
]
MOLD_KINDS = ("range", "positive", "nan")       # positive: the minimum is above 0, so the blend with the zero border clips from below


def _mold_image(shape, C, kind, seed):
    rng = np.random.RandomState(seed)
    img = rng.normal(0.3, 1.5, shape + (C,)).astype(np.float32)          # negative values and values above 1
    img.flat[rng.randint(img.size)] = np.float32(7.25)
    img.flat[rng.randint(img.size)] = np.float32(-3.5)
    if kind == "positive":
        img = (np.abs(img) + np.float32(0.75)).astype(np.float32)
    if kind == "nan":
        img.flat[rng.randint(img.size)] = np.nan                         # a single NaN
    return img


def _mold_cfg(C, mode, dim, mean):
    cfg = _gray_cfg("custom", 128, mode="inference", channels=C)
    cfg.IMAGE_RESIZE_MODE, cfg.IMAGE_MIN_DIM, cfg.IMAGE_MAX_DIM, cfg.IMAGE_MIN_SCALE = mode, dim, dim, 0
    cfg.MEAN_PIXEL = mean
    return cfg


def _molder(cfg, dev):
    """A MaskRCNN without its engine: mold_inputs and _mold_inputs_device read the configuration and the device only."""
    import types
    from caesar_mrcnn_amd.model import MaskRCNN
    m = object.__new__(MaskRCNN)
    m.config, m.engine = cfg, types.SimpleNamespace(dev=dev)
    return m


def _host_statement(model, img):
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        molded, metas, windows = model.mold_inputs([img])
    return np.ascontiguousarray(molded, dtype=np.float32)[0], metas, windows          # _run_graph's cast


def _assert_bits(got, want, tag):
    assert got.shape == want.shape and got.dtype == np.float32 and want.dtype == np.float32, tag
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), (tag, int(gn.sum()), int(wn.sum()))
    g, w = got.view(np.uint32)[~gn], want.view(np.uint32)[~wn]
    assert np.array_equal(g, w), (tag, int((g != w).sum()))


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("shape,mode,dim,why", MOLD_SHAPES)
def test_mold_f32_equals_host_statement(dev, monkeypatch, C, shape, mode, dim, why):
    """ops.mold_image_f32 and MaskRCNN._mold_inputs_device against mold_inputs + the float32 cast: every value that is not NaN
    equal bit for bit, NaN in the same places.  A NaN in a scaled image makes the scaled window NaN throughout (np.clip with NaN
    bounds), the zero padding around it stays (minus the mean); unscaled, the NaN stays where it was.  The source is a host array
    (through _mold_inputs_device), a device tensor, and a device tensor that starts 4 bytes past a 16-byte boundary."""
    from caesar_mrcnn_amd import model as model_mod
    from caesar_mrcnn_amd import ops, utils
    monkeypatch.setattr(model_mod, "DEVICE_MOLD_F32_MIN_PIXELS", 0)
    for kind in MOLD_KINDS:
        for mean in (0, [0.25, -1.5, 103.9][:C]):
            cfg = _mold_cfg(C, mode, dim, mean)
            model = _molder(cfg, dev)
            img = _mold_image(shape, C, kind, 100 * C + len(why))
            want, wmeta, wwin = _host_statement(model, img)
            scale, out_hw, padding, window = utils.resize_plan(img.shape, dim, dim, 0, mode)
            scaled = tuple(out_hw) != shape
            if kind == "positive" and out_hw[0] > shape[0]:                          # up-scaled: the border blends with the zero outside
                raw = utils.resize(img, out_hw, preserve_range=True, clip=False)
                assert float(img.min()) > 0 and bool((raw < float(img.min())).any())  # so the clip from below is in use
            if kind == "nan":
                y1, x1, y2, x2 = window
                if scaled:
                    assert np.isnan(want[y1:y2, x1:x2]).all() and int(np.isnan(want).sum()) == (y2 - y1) * (x2 - x1) * C
                else:
                    assert int(np.isnan(want).sum()) == 1
            tag = (shape, C, kind, mean)
            got = model._mold_inputs_device([img])                                   # host array
            assert got is not None
            _assert_bits(got[0].cpu().numpy()[0], want, tag + ("host array",))
            assert np.array_equal(got[1], wmeta) and np.array_equal(got[2], wwin)
            src = torch.from_numpy(img).to(dev)
            got = model._mold_inputs_device([src])                                   # device tensor
            _assert_bits(got[0].cpu().numpy()[0], want, tag + ("device tensor",))
            canvas = want.shape[:2]
            pool = torch.zeros(img.size + 8, dtype=torch.float32, device=dev)
            pool[1:1 + img.size] = src.reshape(-1)
            off = pool[1:1 + img.size].view(img.shape)
            assert off.data_ptr() % 16 == 4
            sentinel = torch.full((3,) + want.shape, 12345.0, dtype=torch.float32, device=dev)
            out = ops.mold_image_f32(off, out_hw, (padding[0][0], padding[1][0]), canvas, utils.mean_pixel(cfg, C), out=sentinel[1])
            assert out.data_ptr() == sentinel[1].data_ptr()
            res = sentinel.cpu().numpy()
            _assert_bits(res[1], want, tag + ("unaligned source",))
            assert np.all(res[0] == 12345.0) and np.all(res[2] == 12345.0)          # nothing outside the canvas is written
            again = ops.mold_image_f32(src, out_hw, (padding[0][0], padding[1][0]), canvas, utils.mean_pixel(cfg, C))
            assert np.array_equal(again.cpu().numpy().view(np.uint32), res[1].view(np.uint32))     # reproducible, NaN payload included


def test_mold_f32_minmax_is_the_images(dev):
    """The two-stage min / max: a 301 x 301 x 3 source (66 stage-1 workgroups; 271 803 floats, so the last three are the scalar tail
    of the 16-byte loads) that is positive everywhere, with its minimum in the LAST element.  Doubled, the border blends with the
    zero outside and is clipped up to that minimum: the result equals the host's bit for bit only if the tail was reduced."""
    from caesar_mrcnn_amd import ops, utils
    rng = np.random.RandomState(5)
    img = rng.uniform(1, 2, (301, 301, 3)).astype(np.float32)
    img[-1, -1, -1] = 0.9
    img[150, 150, 1] = 9.5
    assert img.size % 4 == 3
    out = ops.mold_image_f32(torch.from_numpy(img).to(dev), (602, 602), (0, 0), (602, 602), [0.0, 0.0, 0.0]).cpu().numpy()
    want = utils.resize(img, (602, 602), preserve_range=True).astype(np.float32)
    assert float(want.min()) == float(np.float32(0.9)) and int((want == np.float32(0.9)).sum()) > 500          # the clipped border
    _assert_bits(out, want, "301 x 301 x 3 doubled")


def test_mold_f32_refusals(dev):
    from caesar_mrcnn_amd import _hip, ops
    img = torch.zeros((6, 6, 3), dtype=torch.float32, device=dev)
    out = torch.full((8, 8, 3), 5.0, dtype=torch.float32, device=dev)
    for bad in (img.to(torch.uint8), img[:, :, 0], img.to(torch.float64), img.permute(1, 0, 2)[:, :4], torch.zeros((6, 6, 5), device=dev)):
        with pytest.raises(ValueError):
            ops.mold_image_f32(bad, (6, 6), (1, 1), (8, 8), 0.0, out=out)
    for out_hw, pad_tl in (((0, 6), (1, 1)), ((6, 6), (3, 1)), ((6, 6), (1, -1)), ((6, 9), (0, 0))):
        with pytest.raises(ValueError):
            ops.mold_image_f32(img, out_hw, pad_tl, (8, 8), 0.0, out=out)
    with pytest.raises(ValueError):
        ops.mold_image_f32(img, (6, 6), (1, 1), (8, 8), [1.0, 2.0], out=out)
    with pytest.raises(_hip.HipPathError):
        ops.mold_image_f32(img.cpu(), (6, 6), (1, 1), (8, 8), 0.0)
    torch.cuda.synchronize()
    assert bool((out == 5.0).all())
    L = _hip.lib()
    assert L.mrcnn_mold_image_f32_workspace_bytes() >= 16 * 1025
    assert L.mrcnn_mold_image_f32(None, 6, 6, 3, 6, 6, 1, 1, 8, 8, None, None, None, 0, None) == -1


# ---- the stem at one input channel ---------------------------------------------------------------------------------------
STEM_CASES = [(1, 9, 9, 16), (1, 9, 9, 64), (2, 37, 41, 16), (2, 37, 41, 64)]      # N, H, W, stem width (custom: 16, ResNet: 64)


@pytest.mark.parametrize("case", STEM_CASES)
def test_stem_conv_cin1(dev, case):
    """conv1 of a gray-level model through the C ABI: 7 x 7, stride 2, pad 3, Cin = 1 -- K = 49 = two K-steps of 32, the second
    17 wide, on the general gather path of conv_fwd.hip and the non-fast path of conv_wgrad.hip.  Forward with bias, frozen BN,
    ReLU and the pre-BN z against the oracle at test_conv_fwd's tolerance; weight gradient, plain and accumulating, against the
    oracle's autograd at test_conv_wgrad_and_dgrad's."""
    from caesar_mrcnn_amd import ops
    N, H, W, Cout = case
    rng = np.random.default_rng(2000 + N + H + W + Cout)
    x = _rand(rng, N, H, W, 1)
    w = _rand(rng, 7, 7, 1, Cout, scale=1.0 / 7.0)
    b = _rand(rng, Cout, scale=0.1)
    xt, wt, bt = (torch.tensor(a, device=dev) for a in (x, w, b))
    y = orc.conv2d_nhwc(torch.tensor(x), torch.tensor(w), torch.tensor(b), 2, (3, 3))
    z_ref = y.clone()
    g, be, mu, var = (torch.tensor(a.astype(np.float32)) for a in (rng.uniform(.5, 1.5, Cout), rng.uniform(-.2, .2, Cout),
                                                                   rng.uniform(-.2, .2, Cout), rng.uniform(.5, 1.5, Cout)))
    y = torch.relu(orc.batchnorm_frozen(y, g, be, mu, var))
    scale, shift, rstd = (torch.empty(Cout, device=dev) for _ in range(3))
    ops.bn_fold(g.to(dev), be.to(dev), mu.to(dev), var.to(dev), scale, shift, rstd)
    z = torch.empty(tuple(y.shape), device=dev)
    out = ops.conv2d(xt, wt, bt, scale, shift, None, 2, (3, 3), 1, 0, z_out=z)
    torch.cuda.synchronize()
    assert tuple(out.shape) == (N, (H + 1) // 2, (W + 1) // 2, Cout)
    torch.testing.assert_close(out.cpu(), y, **F32)
    torch.testing.assert_close(z.cpu(), z_ref, **F32)
    # weight gradient
    xg = torch.tensor(x, requires_grad=True)
    wg = torch.tensor(w, requires_grad=True)
    yy = orc.conv2d_nhwc(xg, wg, None, 2, (3, 3))
    dy = torch.tensor(_rand(rng, *yy.shape))
    yy.backward(dy)
    dyt = dy.to(dev)
    dw = ops.conv2d_wgrad(xt, dyt, (7, 7, 1, Cout), 2, (3, 3))
    torch.cuda.synchronize()
    torch.testing.assert_close(dw.cpu(), wg.grad, rtol=5e-4, atol=5e-4 * float(wg.grad.abs().max()))
    dw2 = ops.conv2d_wgrad(xt, dyt, (7, 7, 1, Cout), 2, (3, 3), dw=dw.clone(), accumulate=True)
    torch.testing.assert_close(dw2.cpu(), 2 * wg.grad, rtol=5e-4, atol=1e-3 * float(wg.grad.abs().max()))


# ---- staged inference and training on a one-channel model (the checks and bars of tests/test_engine_gpu.py) -------------------------
def _close(got, ref, rtol, name):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    scale = max(float(np.abs(ref).max()), 1e-12)
    err = float(np.abs(got - ref).max()) / scale
    assert err <= rtol, "%s: max error %.3g of max |ref| %.3g (allowed %.3g)" % (name, err, scale, rtol)


def test_inference_graph_staged_gray(dev):
    from caesar_mrcnn_amd.model import MaskRCNN
    size = 128
    cfg = _gray_cfg("custom", size, mode="inference")
    w = _weights(cfg, 3)
    assert w["conv1/kernel"].shape == (7, 7, 1, 16)
    model = MaskRCNN("inference", cfg, "/tmp/mrcnn_logs", device=dev, weights=w)
    images, _, _, _ = _scene(cfg, 1, 7)
    image = np.ascontiguousarray(images[0][:, :, :1]).astype(np.float32)
    molded, metas, windows = model.mold_inputs([image])
    molded = molded.astype(np.float32)
    assert molded.shape == (1, size, size, 1)
    win = torch.tensor(orc.norm_boxes(windows.astype(np.float32), molded.shape[1:3]), device=dev)
    out = model.engine.infer(torch.tensor(molded, device=dev), win)
    torch.cuda.synchronize()
    o = orc.OracleMaskRCNN(cfg, w)
    x = torch.tensor(molded)
    area = float(size * size)
    with torch.no_grad():
        pyr = o.fpn(*o.backbone(x))
        _, rp, rb = o.rpn(pyr)
    for i, p in enumerate(pyr):
        _close(out["pyramid"][i].cpu(), p, 1e-3, "P%d" % (i + 2))
    _close(out["rpn_class"].cpu(), rp, 1e-3, "rpn_class")
    _close(out["rpn_bbox"].cpu(), rb, 1e-3, "rpn_bbox")
    anchors = orc.get_anchors(cfg, molded.shape[1:])
    np.testing.assert_array_equal(model.engine.anchors(molded.shape[1:]).cpu().numpy(), anchors)
    rois_ref = o.proposal_layer(out["rpn_class"].cpu(), out["rpn_bbox"].cpu(), anchors, cfg.POST_NMS_ROIS_INFERENCE)
    rois = out["rpn_rois"].cpu().numpy()
    same = np.mean(np.all(np.abs(rois - rois_ref) < 1e-5, axis=-1))
    assert same >= 0.98, same
    gp = [p.cpu() for p in out["pyramid"][:4]]
    with torch.no_grad():
        _, probs, bbox = o.classifier_head(rois, gp, area)
    _close(out["mrcnn_class"].cpu(), probs, 1e-3, "mrcnn_class")
    _close(out["mrcnn_bbox"].cpu(), bbox, 1e-3, "mrcnn_bbox")
    det_ref = o.refine_detections(rois[0], out["mrcnn_class"][0].cpu().numpy(), out["mrcnn_bbox"][0].cpu().numpy(), win[0].cpu().numpy())
    det = out["detections"][0].cpu().numpy()
    np.testing.assert_array_equal(det[:, 4:], det_ref[:, 4:])
    np.testing.assert_allclose(det[:, :4], det_ref[:, :4], atol=2e-6)
    with torch.no_grad():
        masks = o.mask_head(det[None, :, :4], gp, area)
    _close(out["mrcnn_mask"].cpu(), masks, 1e-3, "mrcnn_mask")
    # the public entry point, through the replayed HIP graph: the eager graph's detections
    res = model.detect([image])[0]
    assert set(res) == {"rois", "class_ids", "scores", "masks"}
    assert res["masks"].shape[:2] == image.shape[:2] and res["masks"].shape[2] == res["rois"].shape[0]
    model.use_hip_graph = False
    eager = model.detect([image])[0]
    for k in ("rois", "class_ids", "scores", "masks"):
        assert np.array_equal(res[k], eager[k]), k


def test_training_step_staged_gray(dev):
    """test_training_step_staged on a one-channel model (custom backbone, 128): sampling stage exact, logits / masks / losses and
    every parameter gradient -- conv1/kernel [7, 7, 1, 16] among them -- at that test's bars; then two optimiser steps through the
    launch tape against the same steps issued eagerly (the bars of the float32 case of the replay test)."""
    from caesar_mrcnn_amd.model import MaskRCNN
    size = 128
    cfg = _gray_cfg("custom", size)
    cfg.LOSS_WEIGHTS = dict(cfg.LOSS_WEIGHTS, rpn_bbox_loss=0.7, mrcnn_mask_loss=1.3)
    B = 2
    w = _weights(cfg, 11)
    model = MaskRCNN("training", cfg, "/tmp/mrcnn_logs", device=dev, weights=w)
    inputs, keys = _train_inputs(cfg, B, 5)
    inputs[0] = np.ascontiguousarray(inputs[0][..., :1])
    inputs[1] = np.stack([orc.compose_image_meta(b, inputs[0][b].shape, inputs[0][b].shape, (0, 0) + inputs[0][b].shape[:2], 1.0,
                                                 np.ones(cfg.NUM_CLASSES, np.int32)) for b in range(B)])
    losses = model.train_on_batch(inputs, rand_keys=keys, apply=False, keep_outputs=True)
    torch.cuda.synchronize()
    eng = model.engine
    last = {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in eng.last.items() if k != "pyramid"}
    images, meta, rpn_match, rpn_bbox_t, gt_cls, gt_boxes, gt_masks = inputs
    o = orc.OracleMaskRCNN(cfg, w, requires_grad=True)
    anchors = orc.get_anchors(cfg, images.shape[1:])
    S = float(size)
    gtn = ((gt_boxes.astype(np.float32) - np.array([0, 0, 1, 1], np.float32)) / np.float32(S - 1)).astype(np.float32)
    npos = 0
    for b in range(B):
        r_rois, r_cls, r_bb, r_m, (P, N) = o.detection_targets(last["rpn_rois"][b], gt_cls[b], gtn[b], gt_masks[b], keys[b])
        assert tuple(last["counts"][b]) == (P, N)
        np.testing.assert_array_equal(last["rois"][b], r_rois)
        np.testing.assert_array_equal(last["target_class_ids"][b], r_cls)
        np.testing.assert_allclose(last["target_bbox"][b], r_bb, rtol=1e-5, atol=1e-5)
        np.testing.assert_array_equal(last["target_mask"][b], r_m)
        npos += P
    assert npos > 0, "scene produced no positive ROIs; the mask/bbox losses would be untested"
    forced = {k: last[k] for k in ("rois", "target_class_ids", "target_bbox", "target_mask")}
    ref = o.forward_training(images, rpn_match, rpn_bbox_t.astype(np.float32), gt_cls, gt_boxes, gt_masks,
                             meta[:, 12:].astype(np.int32), anchors, keys, forced=forced)
    _close(last["rpn_class_logits"], ref["rpn_class_logits"].detach(), 1e-3, "rpn_class_logits")
    _close(last["mrcnn_class_logits"], ref["mrcnn_class_logits"].detach(), 1e-3, "mrcnn_class_logits")
    quota = int(cfg.TRAIN_ROIS_PER_IMAGE * cfg.ROI_POSITIVE_RATIO)
    assert eng.sparse_mask_bwd and 0 < quota < cfg.TRAIN_ROIS_PER_IMAGE
    _close(last["mrcnn_mask"][:, :quota], ref["mrcnn_mask"].detach().numpy()[:, :quota], 1e-3, "mrcnn_mask")
    assert not last["mrcnn_mask"][:, quota:].any()
    np.testing.assert_allclose(losses.cpu().numpy(), [float(l.detach()) for l in ref["losses"]], rtol=2e-3, atol=1e-5)
    total = o.total_loss(ref["losses"])
    total.backward()
    eng.apply_gradients(0.0, 0.0, world_size=1)      # lr = 0: only prepares (adds L2) and clips into eng.grads
    torch.cuda.synchronize()
    g = eng.get_weights(grads=True)
    gnorm = float(eng.sumsq.sqrt())
    ref_sq = 0.0
    bad = []
    assert "conv1/kernel" in eng.layout.offsets and g["conv1/kernel"].shape == (7, 7, 1, 16)
    for name in eng.layout.offsets:
        rg = o.w[name].grad
        assert rg is not None, name
        rg = rg.numpy()
        ref_sq += float((rg.astype(np.float64) ** 2).sum())
        scale = max(float(np.abs(rg).max()), 1e-8)
        err = float(np.abs(g[name] - rg).max()) / scale
        if err > 5e-3:
            bad.append((name, err, scale))
    assert not bad, "gradient mismatch (name, rel err, max|ref|): %s" % bad[:8]
    assert float(np.abs(o.w["conv1/kernel"].grad.numpy()).max()) > 0
    np.testing.assert_allclose(gnorm, np.sqrt(ref_sq), rtol=1e-3)
    # two steps through the launch tape against the eager steps
    runs = {}
    for taped in (False, True):
        m2 = MaskRCNN("training", cfg, "/tmp/mrcnn_logs", device=dev, weights=w)
        m2.compile(0.002, 0.9)
        ls = []
        for s in range(2):
            di = m2._to_device(inputs, keys)
            if taped:
                ls.append(m2.engine.step_taped(di, 0.002, 0.9).cpu().numpy().copy())
            else:
                l_ = m2.engine.forward_backward(*di)
                m2.engine.apply_gradients(0.002, 0.9, 1)
                ls.append(l_.cpu().numpy().copy())
        torch.cuda.synchronize()
        runs[taped] = (np.stack(ls), m2.engine.params.cpu().numpy().copy())
    np.testing.assert_allclose(runs[True][0], runs[False][0], rtol=2e-4, atol=1e-5)
    assert np.abs(runs[True][1] - runs[False][1]).max() <= 2e-4 * np.abs(runs[False][1]).max()
    assert not np.array_equal(runs[False][0][0], runs[False][0][1])          # the first step moved the weights


# ---- detect() ---------------------------------------------------------------------------------------------------------
def _blobs(shape, seed, scale=1.0):
    rng = np.random.RandomState(seed)
    im = rng.normal(40, 10, shape)
    im[30:60, 20:70] += 120
    im[70:90, 50:80] += 80
    return (np.clip(im, 0, 255) * scale).astype(np.float32)


def _host_molded_detect(model, image):
    molded, metas, windows = model.mold_inputs([image])
    out = model._run_graph(molded, metas)
    return model._detect_results(out, [tuple(image.shape)], [tuple(molded[0].shape)], windows)[0]


@pytest.fixture(scope="module")
def detect_models(dev):
    from caesar_mrcnn_amd.model import MaskRCNN
    models = {}
    for C in (1, 3):
        cfg = _gray_cfg("custom", 128, mode="inference", channels=C)
        cfg.DETECTION_MIN_CONFIDENCE = 0.0
        models[C] = (MaskRCNN("inference", cfg, "/tmp/mrcnn_logs", device=dev, weights=_weights(cfg, 3)), cfg)
    return models


def test_detect_float32_device_molded_equals_host_molded(dev, detect_models, monkeypatch):
    """detect() on float32 RGB, float32 gray [h, w, 1] and 2-D gray images, as device tensors and as host arrays sent to the
    device molding: rois, class ids, scores and masks equal those of the host-molded path (same graph, bit-equal input).  By
    default a small float32 host array keeps the host molding (model.DEVICE_MOLD_F32_MIN_PIXELS) and a tensor never does."""
    from caesar_mrcnn_amd import model as model_mod
    keys = ("rois", "class_ids", "scores", "masks")
    n = 0
    for C, shapes in ((3, [(128, 128, 3), (100, 90, 3)]), (1, [(128, 128, 1), (100, 90, 1), (100, 90)])):
        model, cfg = detect_models[C]
        for shape in shapes:
            image = _blobs(shape, 2 + len(shape), scale=1.0 if C == 3 else 1.0 / 255.0)
            full = image if image.ndim == 3 else image[:, :, None]
            want = _host_molded_detect(model, full)
            assert want["masks"].shape[:2] == shape[:2]
            n += want["rois"].shape[0]
            assert model._mold_inputs_device([full]) is None                         # below the gate: host molding
            with monkeypatch.context() as mp:
                mp.setattr(model_mod, "DEVICE_MOLD_F32_MIN_PIXELS", 0)
                got_host = model.detect([image])[0]
            got_dev = model.detect([torch.from_numpy(image).to(dev)])[0]
            default = model.detect([image])[0]
            for got in (got_host, got_dev, default):
                for k in keys:
                    assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (shape, k)
        big = _blobs((256, 256, C), 9)
        assert big.shape[0] * big.shape[1] >= model_mod.DEVICE_MOLD_F32_MIN_PIXELS
        molded = model._mold_inputs_device([big])
        assert molded is not None                                                    # at the gate: device molding
        _assert_bits(molded[0].cpu().numpy()[0], _host_statement(model, big)[0], ("256 x 256", C))
        assert model._mold_inputs_device([big.astype(np.float64)]) is None           # float64 keeps the host path
    assert n > 0


def test_detect_refuses_other_channel_counts(dev, detect_models):
    gray, _ = detect_models[1]
    rgb, _ = detect_models[3]
    g, c = _blobs((128, 128, 1), 1), _blobs((128, 128, 3), 1)
    for model, bad in ((gray, c), (rgb, g), (rgb, g[:, :, 0]), (gray, torch.from_numpy(c).to(dev)), (rgb, torch.from_numpy(g).to(dev)),
                       (rgb, c.astype(np.uint8)[:, :, :1]), (gray, np.zeros((128, 128, 2), np.float32))):
        with pytest.raises(ValueError, match="channel"):
            model.detect([bad])
    molded, metas, _ = rgb.mold_inputs([c])
    with pytest.raises(ValueError, match="channel"):
        gray.detect_molded(molded.astype(np.float32), metas)
    # a batch of device tensors has one dtype
    with pytest.raises(ValueError):
        rgb.detect([torch.from_numpy(c).to(dev).to(torch.float64)])


def test_gray_weights_and_checkpoints(dev, detect_models, tmp_path):
    """3-channel weights into a 1-channel model raise, and the message names exclude; with exclude="conv1" they load.  .h5 and
    .npz checkpoints of a 1-channel model round-trip."""
    from caesar_mrcnn_amd import weights_io
    from caesar_mrcnn_amd.model import MaskRCNN
    gray, cfg1 = detect_models[1]
    rgb, cfg3 = detect_models[3]
    with pytest.raises(ValueError, match="exclude"):
        MaskRCNN("inference", cfg1, "/tmp/mrcnn_logs", device=dev, weights=_weights(cfg3, 3))
    fresh = MaskRCNN("inference", cfg1, "/tmp/mrcnn_logs", device=dev, seed=1)
    for ext in ("h5", "npz"):
        p3 = str(tmp_path / ("rgb." + ext))
        rgb.save_weights(p3)
        with pytest.raises(ValueError, match="exclude"):
            fresh.load_weights(p3, by_name=True)
        stem = fresh.engine.get_weights()["conv1/kernel"].copy()
        fresh.load_weights(p3, by_name=True, exclude="conv1")
        got, src = fresh.engine.get_weights(), rgb.engine.get_weights()
        assert np.array_equal(got["conv1/kernel"], stem) and got["conv1/kernel"].shape == (7, 7, 1, 16)
        assert all(np.array_equal(got[k], src[k]) for k in src if not k.startswith("conv1/"))
        p1 = str(tmp_path / ("gray." + ext))
        gray.save_weights(p1)
        assert weights_io.load(p1)["conv1/kernel"].shape == (7, 7, 1, 16)
        other = MaskRCNN("inference", cfg1, "/tmp/mrcnn_logs", device=dev, seed=2)
        other.load_weights(p1, by_name=True)
        a, b = other.engine.get_weights(), gray.engine.get_weights()
        assert set(a) == set(b) and all(np.array_equal(a[k], b[k]) for k in b)


def test_gray_head_dtype(dev):
    """HEAD_DTYPE = bfloat16 on a one-channel model: the stem stays float32, detect() runs and the device-molded input gives the
    host-molded result."""
    from caesar_mrcnn_amd.model import MaskRCNN
    cfg = _gray_cfg("custom", 128, mode="inference")
    cfg.DETECTION_MIN_CONFIDENCE = 0.0
    cfg.HEAD_DTYPE = "bfloat16"
    model = MaskRCNN("inference", cfg, "/tmp/mrcnn_logs", device=dev, weights=_weights(cfg, 3))
    assert model.engine.op("conv1").w.dtype == torch.float32
    image = _blobs((100, 90, 1), 4, scale=1.0 / 255.0)
    want = _host_molded_detect(model, image)
    got = model.detect([torch.from_numpy(image).to(dev)])[0]
    assert want["rois"].shape[0] > 0
    for k in ("rois", "class_ids", "scores", "masks"):
        assert np.array_equal(got[k], want[k]), k


def test_read_fits_keeps_float_images_on_the_device(dev, tmp_path):
    """read_fits(device=, device_out="any"): the float32 RGB image as a [H, W, 3] device tensor, the gray one as [H, W], equal to
    the host path's arrays; device_out=True keeps returning the host array for them."""
    from caesar_mrcnn_amd import fits
    img = tc.mosaic()[:128, :160]
    path = str(tmp_path / "t.fits")
    fits.write_fits(path, img)
    for kw, shape in ((dict(to_uint8=False), (128, 160, 3)), (dict(convertToRGB=False), (128, 160)), (dict(), (128, 160, 3))):
        want = fits.read_fits(path, **kw)[0]
        kept = fits.read_fits(path, device=dev, device_out="any", **kw)[0]
        assert torch.is_tensor(kept) and kept.is_cuda and tuple(kept.shape) == shape == want.shape
        assert str(kept.dtype).replace("torch.", "") == str(want.dtype)
        assert np.array_equal(kept.cpu().numpy(), want)
        back = fits.read_fits(path, device=dev, device_out=True, **kw)[0]
        assert torch.is_tensor(back) == (want.dtype == np.uint8)


# ---- the tiled source finder -----------------------------------------------------------------------------------------------
class _Threshold(tc.ThresholdModel):
    """tc.ThresholdModel for images of `image_channels` channels in [0, top]: 2-D, [h, w, 1] or [h, w, 3], host or device."""

    def __init__(self, config, image_channels, top):
        import types
        tc.ThresholdModel.__init__(self, config)
        self.top, self.seen = top, []
        # what SFinder reads of a MaskRCNN: the shape of its stem's kernel
        self.engine = types.SimpleNamespace(layout=types.SimpleNamespace(by_name={"conv1": types.SimpleNamespace(shape=(7, 7, image_channels, 16))}))

    def detect(self, images, verbose=0):
        host = []
        for image in images:
            self.seen.append((torch.is_tensor(image) and image.is_cuda, str(image.dtype).replace("torch.", ""), tuple(image.shape)))
            a = image.cpu().numpy() if torch.is_tensor(image) else np.asarray(image)
            a = a[:, :, None] if a.ndim == 2 else a
            host.append(np.where(a[..., :1] * (255.0 / self.top) >= 200, 255, 0).astype(np.uint8))
        return tc.ThresholdModel.detect(self, host, verbose)


@pytest.mark.parametrize("kind", ["no_uint8", "grayimg"])
def test_sfinder_batches_float_and_gray_tiles(dev, tmp_path, caplog, kind):
    """The mosaic of the batched-tile tests with IMG_TO_UINT8 off (float32 RGB tiles) and with IMG_TO_RGB off (gray tiles),
    tile_batch = 1 against the loop, the stub model whose detections are a pure function of the tile's values: equal catalogue,
    JSON and region file; every image of the batched run is a float32 device tensor of the model's channels; no log line about
    tile_batch.  A chain whose channels are not the model's raises."""
    from caesar_mrcnn_amd.sfinder import SFinder
    path = str(tmp_path / "mosaic.fits")
    tc.write_mosaic(path)
    channels, top = (3, 255.0) if kind == "no_uint8" else (1, 1.0)

    def cfg_of():
        cfg = tc.config(path, 1.0)
        if kind == "no_uint8":
            cfg.IMG_TO_UINT8 = False
        else:
            cfg.IMG_TO_RGB = False
        return cfg
    runs = {}
    for batch in (0, 1):
        d = str(tmp_path / ("b%d" % batch))
        os.makedirs(d)
        with caplog.at_level(logging.INFO, logger="mrcnn"):
            caplog.clear()
            cfg = cfg_of()
            sf = SFinder(_Threshold(cfg, channels, top), cfg)
            sf.merge_device = sf.params_device = False
            sf.tile_batch = batch
            sf.outfile_json, sf.outfile_ds9 = os.path.join(d, "cat.json"), os.path.join(d, "cat.reg")
            assert sf.run_parallel() == 0
            said = [r.getMessage() for r in caplog.records if "tile_batch" in r.getMessage() or "one at a time" in r.getMessage()]
        assert said == []
        runs[batch] = (cases.canon(sf.sources["sources"]), open(sf.outfile_json).read(), open(sf.outfile_ds9).read(), sf.model.seen,
                       sf.model.batches)
    assert len(runs[0][0]) > 10 and runs[1][0] == runs[0][0]
    assert runs[1][1] == runs[0][1] and runs[1][2] == runs[0][2]
    assert runs[1][4] == [1] * 9 and len(runs[1][3]) == 9
    for on_dev, dtype, shape in runs[1][3]:
        assert on_dev and dtype == "float32" and len(shape) == 3 and shape[2] == channels
    assert all(not on_dev for on_dev, _, _ in runs[0][3])
    wrong = SFinder(_Threshold(cfg_of(), 4 - channels, top), cfg_of())
    wrong.write_to_json = wrong.write_to_ds9 = False
    wrong.merge_device = wrong.params_device = False
    wrong.tile_batch = 1
    with pytest.raises(ValueError, match="channel"):
        wrong.run_parallel()


# ---- the command line ----------------------------------------------------------------------------------------------------
def _make_dataset(d, n=4, size=128):
    from caesar_mrcnn_amd import fits
    rng = np.random.RandomState(0)
    rows = []
    yy, xx = np.mgrid[0:size, 0:size]
    for i in range(n):
        img = rng.normal(0, 1, (size, size)).astype(np.float32)
        cy, cx = rng.uniform(30, size - 30, 2)
        blob = np.exp(-0.5 * (((yy - cy) / 6.0) ** 2 + ((xx - cx) / 9.0) ** 2))
        img += 80 * blob
        if i == 0:
            img[:3, :] = np.nan
        fits.write_fits(os.path.join(d, "img%d.fits" % i), img, {"BUNIT": "JY/BEAM"})
        fits.write_fits(os.path.join(d, "mask%d.fits" % i), (blob > 0.3).astype(np.float32))
        rows.append("%s,%s,%s" % (os.path.join(d, "img%d.fits" % i), os.path.join(d, "mask%d.fits" % i), ["source", "galaxy"][i % 2]))
    lst = os.path.join(d, "train.dat")
    open(lst, "w").write("\n".join(rows) + "\n")
    return lst


def _run(args, cwd):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "run.py")] + args, cwd=cwd, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=280)
    out = r.stdout.decode()
    assert r.returncode == 0, out[-3000:]
    return out


def test_cli_grayimg(dev, tmp_path):
    """run.py train --grayimg for one tiny epoch: the checkpoint's conv1/kernel has one input channel; run.py detect --grayimg with
    it runs and writes its JSON."""
    from caesar_mrcnn_amd import weights_io
    d = str(tmp_path)
    lst = _make_dataset(d)
    common = ["--imgsize", "128", "--backbone", "custom", "--logs", os.path.join(d, "logs"), "--datalist", lst,
              "--train_rois_per_image", "32", "--rpn_train_anchors_per_image", "64", "--max_gt_instances", "10", "--grayimg"]
    out = _run(["train"] + common + ["--nepochs", "1", "--epoch_length", "2", "--nvalidation_steps", "1", "--nimg_per_gpu", "2"], d)
    assert "Epoch 1/1" in out
    ckpts = glob.glob(os.path.join(d, "logs", "rg-dataset*", "mask_rcnn_rg-dataset_0001.h5"))
    assert len(ckpts) == 1
    assert weights_io.load(ckpts[0])["conv1/kernel"].shape == (7, 7, 1, 16)
    outjson = os.path.join(d, "det.json")
    _run(["detect"] + common + ["--weights", ckpts[0], "--image", os.path.join(d, "img0.fits"), "--scoreThr", "0.0",
                                "--detect_outfile_json", outjson], d)
    res = json.load(open(outjson))
    assert res["image_id"] == "img0" and isinstance(res["objs"], list)
    for s in res["objs"][:3]:
        assert {"name", "x1", "x2", "y1", "y2", "class_id", "class_name", "score", "pixels", "vertexes", "edge"} == set(s)
