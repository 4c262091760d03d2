"""The forward chain of two 3 x 3 Winograd layers (mrcnn_winograd_chain, ops.conv2d_winograd_chain, engine._wino_chained_fwd): the
output transform and epilogue of a layer and the input transform of the next as one launch, the activated output kept in LDS.
It computes the separate launches' expressions in their order, so everything it writes -- z, the next layer's V -- and everything
computed from those must equal the separate launches' BIT FOR BIT; one case goes against the oracle as well."""
import numpy as np
import pytest
import torch

import mrcnn_oracle as orc
from model_cases import _rand

pytestmark = pytest.mark.gpu

# (N, H = W, C): one 4 x 4 tile per map with every group present; tile counts far from a 128-row GEMM tile; the mask head's map;
# 390 tiles in the 4 x 2 and 2 x 4 groups (three 128-row GEMM tiles and a ragged fourth)
CASES = [(1, 6, 128), (3, 10, 128), (9, 14, 256), (130, 14, 128)]
RELU = 1


def _ops():
    from caesar_mrcnn_amd import ops
    return ops


def _layers(dev, N, H, C, seed, bn=True):
    """x and two C -> C layers: (U, bias, scale, shift) each, mixed tiling."""
    ops = _ops()
    rng = np.random.default_rng(seed)
    t = lambda a: torch.tensor(a, device=dev)
    x = t(_rand(rng, N, H, H, C))
    layers = []
    for _ in range(2):
        w = t(_rand(rng, 3, 3, C, C, scale=1.0 / np.sqrt(9 * C)))
        b = t(_rand(rng, C, scale=0.1))
        sc = t(rng.uniform(.5, 1.5, C).astype(np.float32)) if bn else None
        sh = t(rng.uniform(-.2, .2, C).astype(np.float32)) if bn else None
        layers.append((ops.winograd_weights(w, tile=ops.TILE_MIXED), b, sc, sh, w))
    return x, layers


def _separate(x, layers, with_z=True):
    """Layer 1 (output materialised), then layer 2 with its input transform kept: z1, V2, y2."""
    ops = _ops()
    N, H, W, C = x.shape
    (U1, b1, sc1, sh1, _), (U2, b2, sc2, sh2, _) = layers
    z = torch.zeros((N, H, W, C), device=x.device) if with_z else None
    out = ops.conv2d_winograd(x, U1, b1, sc1, sh1, RELU, z_out=z)
    V = torch.zeros(ops.winograd_v_floats((N, H, W, C), ops.TILE_MIXED), device=x.device)     # zeros: the padded rows compare too
    y = ops.conv2d_winograd(out, U2, b2, sc2, sh2, RELU, keep_v=V)
    return z, V, y, out


def _chained(x, layers, with_z=True):
    ops = _ops()
    N, H, W, C = x.shape
    (U1, b1, sc1, sh1, _), (U2, b2, sc2, sh2, _) = layers
    z = torch.zeros((N, H, W, C), device=x.device) if with_z else None
    V = torch.zeros(ops.winograd_v_floats((N, H, W, C), ops.TILE_MIXED), device=x.device)
    out = ops.conv2d_winograd_chain(x, U1, V, b1, sc1, sh1, RELU, z_out=z)
    assert out is None, "the one-launch kernel refused a shape it is required to take"
    y = ops.conv2d_winograd((N, H, W, C), U2, b2, sc2, sh2, RELU, keep_v=V, v_ready=True)
    return z, V, y


@pytest.mark.parametrize("bn", [True, False])
@pytest.mark.parametrize("with_z", [True, False])
@pytest.mark.parametrize("case", CASES)
def test_chain_equals_separate_launches(dev, case, with_z, bn):
    N, H, C = case
    x, layers = _layers(dev, N, H, C, 500 + sum(case), bn)
    z1, V1, y1, _ = _separate(x, layers, with_z)
    z2, V2, y2 = _chained(x, layers, with_z)
    torch.cuda.synchronize()
    assert float(V1.abs().max()) > 0 and float(y1.abs().max()) > 0
    if with_z:
        assert torch.equal(z1, z2)
    assert torch.equal(V1, V2)
    assert torch.equal(y1, y2)


def test_chain_on_the_relu_edge(dev):
    """scale * z + shift == 0 exactly in every channel of one pixel: shift = -(scale * z) there, z from a first pass (it does not
    depend on the shift); the float32 product and its negation cancel exactly."""
    N, H, C = 3, 10, 128
    x, layers = _layers(dev, N, H, C, 77)
    z0 = _separate(x, layers)[0]
    U1, b1, sc1, _, w1 = layers[0]
    layers[0] = (U1, b1, sc1, -(sc1 * z0[1, 9, 9, :]), w1)           # a pixel of the 2 x 2 group
    z1, V1, y1, out = _separate(x, layers)
    z2, V2, y2 = _chained(x, layers)
    torch.cuda.synchronize()
    assert torch.equal(out[1, 9, 9, :], torch.zeros(C, device=dev)) and torch.equal(sc1 * z1[1, 9, 9, :] + layers[0][3], torch.zeros(C, device=dev))
    assert torch.equal(z1, z2) and torch.equal(V1, V2) and torch.equal(y1, y2)


def test_two_chained_layers_against_the_oracle(dev):
    """(9, 14, 256) through two layers, the first chained into the second, against the oracle's convolution twice: the second
    layer's output at test_conv_winograd's tile-4 tolerance (rtol 1e-4, atol 5e-5 of the reference's range)."""
    N, H, C = 9, 14, 256
    x, layers = _layers(dev, N, H, C, 91)
    _, _, y = _chained(x, layers)
    torch.cuda.synchronize()
    ref = x.cpu()
    for _, b, sc, sh, w in layers:
        ref = torch.relu(orc.conv2d_nhwc(ref, w.cpu(), b.cpu(), 1, "same") * sc.cpu() + sh.cpu())
    err = float((y.cpu() - ref).abs().max())
    print("two chained layers: max |error| %.3e, reference range %.3e" % (err, float(ref.abs().max())))
    torch.testing.assert_close(y.cpu(), ref, rtol=1e-4, atol=5e-5 * float(ref.abs().max()))


@pytest.mark.parametrize("what, tile, H, C", [("uniform 4 x 4 tiling", 4, 14, 128), ("uniform 2 x 2 tiling", 2, 14, 128),
                                              ("odd extent", 6, 7, 128), ("extent 0 mod 4", 6, 8, 128), ("extent 2: no 4 x 4 tile", 6, 2, 128),
                                              ("channels not in 128s", 6, 14, 64), ("channels not in 128s", 6, 14, 192)])
def test_chain_entry_refuses_before_any_launch(dev, what, tile, H, C):
    from caesar_mrcnn_amd import _hip
    ops = _ops()
    N = 2
    n = 36 * 128 * C * 4                                             # more than any group of these shapes
    Mt = torch.zeros(n, device=dev)
    V = torch.full((n,), 3.0, device=dev)
    z = torch.full((N, H, H, C), 5.0, device=dev)
    rc = _hip.lib().mrcnn_winograd_chain(_hip.ptr(Mt), _hip.ptr(z), None, None, None, _hip.ptr(V), N, H, H, C, RELU, tile, _hip.current_stream())
    torch.cuda.synchronize()
    assert rc == ops.ERR_UNSUPPORTED, what
    assert bool((V == 3.0).all()) and bool((z == 5.0).all()), what


def test_ops_take_the_separate_launches_where_the_kernel_refuses(dev):
    """The uniform 4 x 4 tiling (one group, tiles hanging over the edge of a 10 x 10 map): conv2d_winograd_chain returns the
    activated output and has written the next layer's V, both as the separate calls do."""
    ops = _ops()
    N, H, C = 3, 10, 128
    rng = np.random.default_rng(5)
    t = lambda a: torch.tensor(a, device=dev)
    x = t(_rand(rng, N, H, H, C))
    w, b = t(_rand(rng, 3, 3, C, C, scale=1.0 / np.sqrt(9 * C))), t(_rand(rng, C, scale=0.1))
    sc, sh = t(rng.uniform(.5, 1.5, C).astype(np.float32)), t(rng.uniform(-.2, .2, C).astype(np.float32))
    U = ops.winograd_weights(w, tile=4)
    nv = ops.winograd_v_floats((N, H, H, C), 4)
    z1, z2 = torch.zeros((N, H, H, C), device=dev), torch.zeros((N, H, H, C), device=dev)
    V1, V2 = torch.zeros(nv, device=dev), torch.zeros(nv, device=dev)
    out1 = ops.conv2d_winograd(x, U, b, sc, sh, RELU, z_out=z1)
    ops.conv2d_winograd(out1, U, keep_v=V1)
    out2 = ops.conv2d_winograd_chain(x, U, V2, b, sc, sh, RELU, z_out=z2)
    torch.cuda.synchronize()
    assert out2 is not None and torch.equal(out1, out2) and torch.equal(z1, z2) and torch.equal(V1, V2) and float(V1.abs().max()) > 0


# ---- engine level: 512 ROIs of 14 x 14, the smallest count at which ops.winograd_tile picks the mixed tiling -----------------------
def _engine(dev, seed):
    import test_engine_gpu as T
    from caesar_mrcnn_amd.model import MaskRCNN
    cfg = T._full_cfg("resnet50", 256, nimg=1)
    model = MaskRCNN("training", cfg, "/tmp/mrcnn_logs", device=dev, weights=T._weights(cfg, seed))
    return T, cfg, model


def test_mask_head_forward_chained_equals_unchained(dev):
    from caesar_mrcnn_amd import engine as E, ops
    T, cfg, model = _engine(dev, 31)
    eng = model.engine
    assert eng.winograd_chain and cfg.TRAIN_ROIS_PER_IMAGE == 512
    rng = np.random.default_rng(9)
    images = torch.tensor(rng.uniform(-100, 100, (1, 256, 256, 3)).astype(np.float32), device=dev)
    yx = rng.uniform(0, 0.6, (1, 512, 2))
    rois = torch.tensor(np.concatenate([yx, yx + rng.uniform(0.05, 0.4, (1, 512, 2))], axis=2).astype(np.float32), device=dev)
    assert ops.winograd_tile((512, 14, 14, 256)) == ops.TILE_MIXED
    pyr, _, p16h, _ = eng._trunk_fwd(images, True)
    runs = {}
    for on in (True, False):
        eng.winograd_chain = on
        masks, ctxs = eng._mask_head_fwd(rois, pyr[:4], p16h, float(256 * 256), True)
        torch.cuda.synchronize()
        runs[on] = (masks, ctxs)
    (m1, c1), (m0, c0) = runs[True], runs[False]
    assert torch.equal(m1, m0) and float(m0.std()) > 0
    for i in range(4):
        assert c1[i].path == c0[i].path == E.WINO
        assert torch.equal(c1[i].z, c0[i].z), i
        assert c1[i].V is not None and torch.equal(c1[i].V, c0[i].V), i     # (512 maps: every group's tile count is a multiple of 128, no padded rows)
        assert c0[i].out is not None and c0[i].x is not None
    assert [c.out is None for c in c1[:4]] == [True, True, True, False]
    assert [c.x is None for c in c1[:4]] == [False, True, True, True]
    assert torch.equal(c1[3].out, c0[3].out)


def test_training_step_with_the_chain(dev, monkeypatch):
    """One forward_backward with all 512 ROIs in the mask head (sparse_mask_bwd off: the positive quota alone, 168 ROIs, would stay
    on F(2x2, 3x3) and never link a layer), chain on and off on the same seeded batch and weights.  With the chain on the three
    linked launches are issued (and none with it off), the backward runs through contexts whose out / x are None, the losses are
    finite; losses and gradients agree between the two within the bound of the engine's other switch tests
    (test_fused_dgrad_epilogue_equals_unfused: losses rtol 5e-6, gradients 2e-5 of their largest entry -- the order of the
    float atomics in the channel sums; the mask-head forward itself is bit-identical)."""
    from caesar_mrcnn_amd import ops
    assert ops.winograd_tile((512, 14, 14, 256)) == ops.TILE_MIXED
    calls = []
    real = ops.conv2d_winograd_chain

    def spy(*a, **k):
        out = real(*a, **k)
        calls.append(out is None)
        return out
    monkeypatch.setattr(ops, "conv2d_winograd_chain", spy)
    res = {}
    for on in (True, False):
        T, cfg, model = _engine(dev, 37)
        eng = model.engine
        assert eng.winograd_chain
        eng.winograd_chain = on
        eng.sparse_mask_bwd = False
        inputs, keys = T._train_inputs(cfg, 1, 43)
        del calls[:]
        losses = model.train_on_batch(inputs, rand_keys=keys, apply=False)
        torch.cuda.synchronize()
        assert calls == ([True, True, True] if on else []), calls       # conv1-3 linked, each by the one-launch kernel
        res[on] = (losses.cpu().numpy(), eng.grads.cpu().numpy().copy())
        del model, eng
    got = res[True][0]
    assert got.shape == (5,) and np.all(np.isfinite(got)) and np.all(np.isfinite(res[True][1])), got
    np.testing.assert_allclose(res[True][0], res[False][0], rtol=5e-6)
    scale = np.abs(res[False][1]).max()
    assert scale > 0 and np.abs(res[True][1] - res[False][1]).max() <= 2e-5 * scale
