"""The mask head's output stage in one launch (mrcnn_deconv2x2_mask_gemm / ops.deconv2x2_mask): the transposed convolution's GEMM
with the mrcnn_mask 1 x 1 convolution, its bias and the sigmoid in the epilogue.

`up` must be what ops.deconv2x2 writes on its GEMM path, bit for bit (every element accumulates over K in the same order in the
128 x 128 and the 128 x 256 tile).  `m` is compared with the float64 sigmoid of the float64 affine map of that stored float32 `up`:

    |m - m64| <= 0.25 (Cd + 2) 2^-24 (sum_co |up_co w_co,k| + |b_k|) + 2^-22

first term: the forward error of a float32 sum of Cd + 1 terms in any order (products rounded once more) times the sigmoid's largest
slope; second: 4 ulp of a value <= 1 for expf and the division.  The two-launch path meets the same bar on the same inputs."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from model_cases import _rand, _scene, _small_cfg, _train_inputs, _weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ops():
    from caesar_mrcnn_amd import ops
    return ops


def test_header_declares_and_library_exports_the_entry():
    from caesar_mrcnn_amd import _hip
    assert "mrcnn_deconv2x2_mask_gemm" in set(_hip.exported_symbols())
    header = open(os.path.join(ROOT, "include", "mrcnn_hip.h")).read()
    assert "int mrcnn_deconv2x2_mask_gemm(" in header


def _inputs(N, H, W, Cin, Cd, C, seed):
    """Seeded operands in the style of _mask_out_inputs (tests/test_kernels_gpu.py), from the deconvolution's input on: about half
    of relu(deconv) is positive, so the ReLU bites."""
    from caesar_mrcnn_amd.params import deconv_keras_to_gemm
    rng = np.random.default_rng(seed)
    x = torch.tensor(_rand(rng, N, H, W, Cin))
    k = _rand(rng, 2, 2, Cd, Cin, scale=0.05)                      # Keras (2, 2, out, in)
    wg = torch.tensor(deconv_keras_to_gemm(k).reshape(Cin, 4 * Cd))
    b = torch.tensor(_rand(rng, Cd, scale=0.1))
    wm = torch.tensor(_rand(rng, Cd, C, scale=0.1))
    bm = torch.tensor(_rand(rng, C, scale=0.1))
    return x, wg, b, wm, bm


def _bar(up32, wm, bm):
    """(m64, bound) from the stored float32 `up` (CPU), in float64."""
    Cd, Cm = wm.shape
    u = up32.double().reshape(-1, Cd)
    b64 = bm.double() if bm is not None else torch.zeros(Cm, dtype=torch.float64)
    m64 = torch.sigmoid(u @ wm.double() + b64)
    mag = u.abs() @ wm.double().abs() + b64.abs()
    bound = 0.25 * (Cd + 2) * 2.0 ** -24 * mag + 2.0 ** -22
    shape = tuple(up32.shape[:3]) + (Cm,)
    return m64.reshape(shape), bound.reshape(shape)


def _over_bar(m, m64, bound):
    return float(((m.cpu().double() - m64).abs() / bound).max())


CASES = ([(1, 2, 2, 256, 4), (127, 14, 14, 256, 4), (3, 14, 14, 48, 4)] +        # one partial tile; 780 tiles > 768 workgroups; 3 K-steps
         [(3, 14, 14, 256, c) for c in (1, 3, 4, 5, 16)])                       # 588 rows: four full tiles and a partial one


@pytest.mark.gpu
@pytest.mark.parametrize("with_bias", [True, False])
@pytest.mark.parametrize("N,H,W,Cin,Cm", CASES)
def test_fused_output_stage(dev, N, H, W, Cin, Cm, with_bias, monkeypatch):
    ops = _ops()
    monkeypatch.setattr(ops, "_DECONV_GEMM_MIN_ROWS", 1)
    Cd = 256
    x, wg, b, wm, bm = (t.to(dev) for t in _inputs(N, H, W, Cin, Cd, Cm, 9100 + 17 * N + Cin + Cm))
    if not with_bias:
        b = bm = None
    up_ref = ops.deconv2x2(x, wg, b, ops.ACT_RELU)                  # the GEMM path (128 x 128 tiles)
    m_pair = ops.conv2d(up_ref, wm.view(1, 1, Cd, Cm), bm, act=ops.ACT_SIGMOID)
    # the entry itself: ops.deconv2x2_mask must not have fallen back
    up = torch.full((N, 2 * H, 2 * W, Cd), 9.0, device=dev)
    m = torch.full((N, 2 * H, 2 * W, Cm), 9.0, device=dev)
    from caesar_mrcnn_amd import _hip
    p = ops.ptr
    rc = _hip.lib().mrcnn_deconv2x2_mask_gemm(p(x), p(wg), p(b), p(up), p(wm), p(bm), p(m), N, H, W, Cin, Cd, Cm, ops.ACT_RELU,
                                              ops.current_stream())
    assert rc == 0
    up2, m2 = ops.deconv2x2_mask(x, wg, b, wm, bm, ops.ACT_RELU)
    torch.cuda.synchronize()
    assert torch.equal(up, up_ref) and torch.equal(up2, up_ref), "up differs from the deconvolution's own GEMM launch"
    frac = float((up_ref > 0).float().mean())
    assert 0.3 < frac < 0.7, frac
    assert torch.equal(m, m2), "two calls on the same inputs differ"
    m64, bound = _bar(up_ref.cpu(), wm.cpu(), None if bm is None else bm.cpu())
    worst, worst_pair = _over_bar(m, m64, bound), _over_bar(m_pair, m64, bound)
    print("[mask_out_fwd %dx%dx%d Cin=%d C=%d bias=%s] max error over the bar: fused %.3f, two launches %.3f" % (
        N, H, W, Cin, Cm, with_bias, worst, worst_pair))
    assert worst <= 1.0 and worst_pair <= 1.0, (worst, worst_pair)
    # inference form: the same m, and nothing written where `up` lived (the freed block is handed out again, poisoned)
    addr, shape = up2.data_ptr(), tuple(up2.shape)
    del up2
    poison = torch.full(shape, -7.0, device=dev)
    none, m3 = ops.deconv2x2_mask(x, wg, b, wm, bm, ops.ACT_RELU, want_up=False)
    torch.cuda.synchronize()
    assert none is None and torch.equal(m3, m)
    assert bool((poison == -7.0).all()), "want_up=False wrote through an `up` buffer (same block: %s)" % (poison.data_ptr() == addr)


@pytest.mark.gpu
def test_unsupported_shapes_run_as_two_launches(dev, monkeypatch):
    ops = _ops()
    from caesar_mrcnn_amd import _hip
    monkeypatch.setattr(ops, "_DECONV_GEMM_MIN_ROWS", 1)
    p = ops.ptr
    for Cd, Cm in ((256, 17), (320, 4)):
        N, H, W, Cin = 3, 14, 14, 64
        x, wg, b, wm, bm = (t.to(dev) for t in _inputs(N, H, W, Cin, Cd, Cm, 77 + Cd + Cm))
        up = torch.full((N, 2 * H, 2 * W, Cd), 9.0, device=dev)
        m = torch.full((N, 2 * H, 2 * W, Cm), 9.0, device=dev)
        rc = _hip.lib().mrcnn_deconv2x2_mask_gemm(p(x), p(wg), p(b), p(up), p(wm), p(bm), p(m), N, H, W, Cin, Cd, Cm, ops.ACT_RELU,
                                                  ops.current_stream())
        assert rc == ops.ERR_UNSUPPORTED
        up2, m2 = ops.deconv2x2_mask(x, wg, b, wm, bm, ops.ACT_RELU, want_up=False)
        up_ref = ops.deconv2x2(x, wg, b, ops.ACT_RELU)
        m_ref = ops.conv2d(up_ref, wm.view(1, 1, Cd, Cm), bm, act=ops.ACT_SIGMOID)
        torch.cuda.synchronize()
        assert bool((up == 9.0).all()) and bool((m == 9.0).all())              # refused: nothing launched
        assert torch.equal(up2, up_ref) and torch.equal(m2, m_ref)
    assert _hip.lib().mrcnn_deconv2x2_mask_gemm(p(x), p(wg), p(b), p(up), p(wm), p(bm), p(m), N, H, W, Cin, 256, 4, ops.ACT_SIGMOID,
                                                ops.current_stream()) == ops.ERR_UNSUPPORTED


def _close(got, ref, rtol, name):           # the bar of tests/test_engine_gpu.py
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    scale = max(float(np.abs(ref).max()), 1e-12)
    err = float(np.abs(got - ref).max()) / scale
    assert err <= rtol, "%s: max error %.3g of max |ref| %.3g (allowed %.3g)" % (name, err, scale, rtol)


@pytest.mark.gpu
def test_engine_switch_training_and_inference(dev, monkeypatch):
    """One training step and one inference pass with fused_mask_out_fwd on and off, same weights and inputs (the small
    configuration's mask head has fewer rows than the product's GEMM threshold, which is lifted here)."""
    ops = _ops()
    from caesar_mrcnn_amd.model import MaskRCNN
    monkeypatch.setattr(ops, "_DECONV_GEMM_MIN_ROWS", 1)
    cfg = _small_cfg("custom", 128)
    w = _weights(cfg, 37)
    inputs, keys = _train_inputs(cfg, 2, 43)
    res, modes = [], []
    for fused in (True, False):
        model = MaskRCNN("training", cfg, "/tmp/mrcnn_logs", device=dev, weights=w)
        eng = model.engine
        assert eng.fused_mask_out_fwd and eng.head_dtype is None
        eng.fused_mask_out_fwd = fused
        modes.append(eng._mode_key())
        calls = []
        real = ops.deconv2x2_mask
        monkeypatch.setattr(ops, "deconv2x2_mask", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
        losses = model.train_on_batch(inputs, rand_keys=keys, apply=False, keep_outputs=True)
        torch.cuda.synchronize()
        monkeypatch.setattr(ops, "deconv2x2_mask", real)
        assert len(calls) == (1 if fused else 0)
        g = eng.get_weights(grads=True)
        res.append((losses.cpu().numpy().copy(), eng.last["mrcnn_mask"].cpu().numpy().copy(),
                    {n: g[n].copy() for n in ("mrcnn_mask/kernel", "mrcnn_mask/bias", "mrcnn_mask_deconv/bias")}))
    assert modes[0] != modes[1]
    (l1, m1, g1), (l0, m0, g0) = res
    assert l1.shape == (5,) and m1.any()
    _close(m1, m0, 1e-3, "mrcnn_mask")
    for i in range(5):
        _close(l1[i], l0[i], 1e-3, "loss %d" % i)
    for n in g1:
        _close(g1[n], g0[n], 1e-3, n)

    cfg_i = _small_cfg("custom", 128, mode="inference")
    model = MaskRCNN("inference", cfg_i, "/tmp/mrcnn_logs", device=dev, weights=_weights(cfg_i, 3))
    images, _, _, _ = _scene(cfg_i, 1, 7)
    molded, metas, windows = model.mold_inputs([images[0].astype(np.float32)])
    import mrcnn_oracle as orc
    win = torch.tensor(orc.norm_boxes(windows.astype(np.float32), molded.shape[1:3]), device=dev)
    outs = []
    for fused in (True, False):
        model.engine.fused_mask_out_fwd = fused
        out = model.engine.infer(torch.tensor(molded.astype(np.float32), device=dev), win)
        torch.cuda.synchronize()
        outs.append((out["detections"].cpu().numpy().copy(), out["mrcnn_mask"].cpu().numpy().copy()))
    np.testing.assert_array_equal(outs[0][0], outs[1][0])
    _close(outs[0][1], outs[1][1], 1e-3, "mrcnn_mask (inference)")
