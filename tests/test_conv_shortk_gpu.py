"""conv_fwd_sk64_kernel: the single-launch kernel for short-K 1 x 1 layers (res4 2c forward, the data gradient of res4 2a) against
the two-launch split-K plan it replaces, the CPU oracle, and inside a training step.  "old" / "new" are the tuning key "sk64" at
0 (the pair: K slices + slab reduction) and 1 (the kernel takes every shape its rules allow) in one process."""
import numpy as np
import pytest
import torch

import mrcnn_oracle as orc
from model_cases import _rand, _small_cfg, _train_inputs, _weights

pytestmark = pytest.mark.gpu

F32 = dict(rtol=2e-4, atol=2e-4)     # test_conv_fwd's float32 tolerance (fp32 contractions with a different summation order)

# N, H, W, Cin, Cout, stride, act, bn, res, z
FWD_CASES = [
    (4, 16, 16, 256, 1024, 1, 1, True, True, True),     # res4 2c of the headline step: BN, shortcut, ReLU, pre-BN output
    (1, 13, 11, 256, 128, 1, 0, False, False, False),   # M = 143: ragged against the 64-row tile and the 32-row wave tile
    (2, 8, 8, 288, 256, 1, 2, False, False, False),     # 9 K-steps: slices of 5 and 4; sigmoid
]
# shapes the kernel must leave alone: a three-slice plan, a Cout that is no multiple of 64, a stride-2 1 x 1
DECLINED_CASES = [
    (4, 16, 16, 384, 1024, 1, 1, True, True, True),
    (4, 16, 16, 256, 96, 1, 1, True, False, True),
    (4, 16, 16, 256, 512, 2, 1, True, False, True),
]


def _ops():
    from caesar_mrcnn_amd import ops
    return ops


class _Key:
    """with _Key(v): the tuning key "sk64" at v, back to the default window afterwards."""

    def __init__(self, value):
        self.value = value

    def __enter__(self):
        _ops().tuning_set("sk64", self.value)

    def __exit__(self, *exc):
        _ops().tuning_set("sk64", -1)


def _fwd_inputs(case):
    N, H, W, Cin, Cout, stride, act, bn, res, z = case
    rng = np.random.default_rng(4000 + sum(int(v) for v in case))
    OH, OW = (H - 1) // stride + 1, (W - 1) // stride + 1
    t = {"x": _rand(rng, N, H, W, Cin), "w": _rand(rng, 1, 1, Cin, Cout, scale=1.0 / np.sqrt(Cin)), "b": _rand(rng, Cout, scale=0.1)}
    if bn:
        t["bn"] = [a.astype(np.float32) for a in (rng.uniform(.5, 1.5, Cout), rng.uniform(-.2, .2, Cout), rng.uniform(-.2, .2, Cout),
                                                  rng.uniform(.5, 1.5, Cout))]
    if res:
        t["r"] = _rand(rng, N, OH, OW, Cout)
    return t


def _fwd_run(dev, case, t, key):
    """(out, z) of the layer with the tuning key at `key`."""
    ops = _ops()
    N, H, W, Cin, Cout, stride, act, bn, res, z = case
    up = lambda a: torch.tensor(a, device=dev)
    scale = shift = None
    if bn:
        g, be, mu, var = (up(a) for a in t["bn"])
        scale = torch.empty(Cout, device=dev); shift = torch.empty(Cout, device=dev)
        ops.bn_fold(g, be, mu, var, scale, shift, None)
    OH, OW = (H - 1) // stride + 1, (W - 1) // stride + 1
    zt = torch.full((N, OH, OW, Cout), float("nan"), device=dev) if z else None
    with _Key(key):
        out = ops.conv2d(up(t["x"]), up(t["w"]), up(t["b"]), scale, shift, up(t["r"]) if res else None, stride, "valid", act,
                         1 if res else 0, z_out=zt)
    torch.cuda.synchronize()
    return out, zt


@pytest.fixture(scope="module")
def fwd_results(dev):
    """Every forward case once: inputs, the old pair's result and the new kernel's."""
    got = {}
    for case in FWD_CASES + DECLINED_CASES:
        t = _fwd_inputs(case)
        got[case] = (t, _fwd_run(dev, case, t, 0), _fwd_run(dev, case, t, 1))
    return got


@pytest.mark.parametrize("case", FWD_CASES)
def test_forward_equals_the_two_launch_plan_bit_for_bit(fwd_results, case):
    _, (o0, z0), (o1, z1) = fwd_results[case]
    assert torch.isfinite(o1).all()
    assert torch.equal(o1, o0)
    if case[-1]:
        assert torch.isfinite(z1).all()
        assert torch.equal(z1, z0)


@pytest.mark.parametrize("case", FWD_CASES)
def test_forward_against_the_oracle(fwd_results, case):
    N, H, W, Cin, Cout, stride, act, bn, res, z = case
    t, _, (o1, z1) = fwd_results[case]
    y = orc.conv2d_nhwc(torch.tensor(t["x"]), torch.tensor(t["w"]), torch.tensor(t["b"]), stride, "valid")
    z_ref = y.clone()
    if bn:
        y = orc.batchnorm_frozen(y, *(torch.tensor(a) for a in t["bn"]))
    if res:
        y = y + torch.tensor(t["r"])
    if act == 1:
        y = torch.relu(y)
    elif act == 2:
        y = torch.sigmoid(y)
    torch.testing.assert_close(o1.cpu(), y, **F32)
    if z:
        torch.testing.assert_close(z1.cpu(), z_ref, **F32)


@pytest.mark.parametrize("case", DECLINED_CASES)
def test_declined_shapes_are_untouched(fwd_results, case):
    _, (o0, z0), (o1, z1) = fwd_results[case]
    assert torch.equal(o1, o0) and torch.equal(z1, z0)


@pytest.mark.parametrize("case", FWD_CASES[:2])
def test_data_gradient_with_backward_epilogue(dev, case):
    """mrcnn_conv2d_dgrad_ep with the residual port and the second output dy: dz and dy equal the old pair's and the composition
    conv2d + epilogue_bwd bit for bit; the channel sums (float atomics: another order) hold to the split-K test's bars."""
    ops = _ops()
    N, H, W, Cin, Cout = case[:5]
    rng = np.random.default_rng(5000 + Cout + H)
    up = lambda a: torch.tensor(a, device=dev)
    dz = up(_rand(rng, N, H, W, Cin))
    wt = up(_rand(rng, 1, 1, Cin, Cout, scale=1.0 / np.sqrt(Cin)))
    below_out = torch.relu(up(_rand(rng, N, H, W, Cout)))
    below_z = up(_rand(rng, N, H, W, Cout))
    r = up(_rand(rng, N, H, W, Cout))
    scale, mean, rstd = (up(rng.uniform(0.5, 1.5, Cout).astype(np.float32)) for _ in range(3))
    runs = {}
    for key in (0, 1):
        sums = [torch.zeros(Cout, device=dev) for _ in range(3)]
        dy = torch.full((N, H, W, Cout), float("nan"), device=dev)
        with _Key(key):
            got = ops.conv2d_dgrad_ep(dz, wt, "valid", below_out, below_z, scale, mean, rstd, sums[0], sums[1], sums[2], 1, res=r,
                                      dy_out=dy)
        assert got is not None, "expected a split-K plan for %s" % (case,)
        runs[key] = (got, dy, sums)
    with _Key(0):
        y = ops.conv2d(dz, wt, res=r, stride=1, padding="valid", res_mode=1)
    ref, dy_ref = torch.empty_like(y), torch.empty_like(y)
    rs = [torch.zeros(Cout, device=dev) for _ in range(3)]
    ops.epilogue_bwd(y, below_out, below_z, scale, mean, rstd, dy_ref, ref, rs[0], rs[1], rs[2], 1)
    torch.cuda.synchronize()
    got, dy, sums = runs[1]
    assert torch.isfinite(got).all() and torch.isfinite(dy).all()
    assert torch.equal(got, runs[0][0]) and torch.equal(dy, runs[0][1])
    assert torch.equal(got, ref) and torch.equal(dy, dy_ref)
    for a, b0, b in zip(sums, runs[0][2], rs):
        torch.testing.assert_close(a, b, rtol=2e-4, atol=2e-4 * float(b.abs().max()))
        torch.testing.assert_close(a, b0, rtol=2e-4, atol=2e-4 * float(b0.abs().max()))


def test_layer_without_a_split_plan_still_reports_unsupported(dev):
    """4 images, K = 128: neither LDS-DMA tiles nor a split-K plan; the kernel does not invent one."""
    ops = _ops()
    rng = np.random.default_rng(78)
    N, H, W, Cin, Cout = 4, 14, 14, 128, 256
    up = lambda a: torch.tensor(a, device=dev)
    dz, wt = up(_rand(rng, N, H, W, Cin)), up(_rand(rng, 1, 1, Cin, Cout, scale=1.0 / np.sqrt(Cin)))
    below_out, below_z = torch.relu(up(_rand(rng, N, H, W, Cout))), up(_rand(rng, N, H, W, Cout))
    scale, mean, rstd = (up(rng.uniform(0.5, 1.5, Cout).astype(np.float32)) for _ in range(3))
    sums = [torch.zeros(Cout, device=dev) for _ in range(3)]
    with _Key(1):
        small = ops.conv2d_dgrad_ep(dz, wt, "valid", below_out, below_z, scale, mean, rstd, sums[0], sums[1], sums[2], 1)
    assert small is None


FORWARD_TENSORS = ("rpn_class_logits", "rpn_bbox", "rpn_rois", "rois", "target_class_ids", "target_bbox", "target_mask",
                   "mrcnn_class_logits", "mrcnn_bbox", "mrcnn_mask")


@pytest.fixture(scope="module", params=["custom", "resnet50"])
def step_pair(dev, request):
    """One forward_backward on a fresh engine per key value (0, then 1): losses, the forward's tensors, the gradients.  "custom" is
    the smallest configuration the engine tests build; ResNet-50 at the same size is the smallest whose trunk has the layers the
    kernel is for (res4 at 8 x 8: 32 workgroups, below the default window, taken with the key at 1)."""
    from caesar_mrcnn_amd.model import MaskRCNN
    cfg = _small_cfg(request.param, 128)
    w = _weights(cfg, 11)
    inputs, keys = _train_inputs(cfg, 2, 5)
    res = []
    for key in (0, 1):
        with _Key(key):
            model = MaskRCNN("training", cfg, "/tmp/mrcnn_logs", device=dev, weights=w)
            losses = model.train_on_batch(inputs, rand_keys=keys, apply=False, keep_outputs=True)
            torch.cuda.synchronize()
            last = model.engine.last
            res.append((losses.cpu().numpy().copy(), {k: last[k].cpu().numpy().copy() for k in FORWARD_TENSORS},
                        model.engine.get_weights(grads=True)))
    return res


def test_training_step_forward_and_gradients(step_pair):
    """Every tensor the forward hands to the losses, the proposals included, is identical bit for bit (none of it goes through an
    atomic); gradients hold to the step bar of test_engine_gpu (5e-3 of the tensor's maximum)."""
    (_, f0, g0), (_, f1, g1) = step_pair
    for k in FORWARD_TENSORS:
        np.testing.assert_array_equal(f1[k], f0[k], err_msg=k)
    bad = []
    for name in g0:
        scale = max(float(np.abs(g0[name]).max()), 1e-8)
        err = float(np.abs(g1[name].astype(np.float64) - g0[name]).max()) / scale
        if err > 5e-3:
            bad.append((name, err, scale))
    assert not bad, bad[:8]


def test_training_step_losses_bit_for_bit(step_pair):
    """The five losses of the two steps, compared exactly.  The forward's tensors are identical (the test above) and the loss
    kernels add their block sums in a fixed order (loss_finalize_kernel), so nothing on the way to the losses depends on the
    order in which workgroups finish."""
    (l0, _, _), (l1, _, _) = step_pair
    assert l0.shape[-1] == 5 and np.all(np.isfinite(l1))
    print("losses key 0:", l0.tolist(), " key 1:", l1.tolist())
    np.testing.assert_array_equal(l1, l0)


def test_losses_are_reproducible_run_after_run(dev):
    """mrcnn_losses_fwd_bwd on the same inputs, six times: the five losses and every gradient are bit-identical (2 images of 64 ROI
    rows: 128 head block sums of three losses, which float atomics added in an order that changed from run to run).  With the
    Dice loss too, whose gradient is scaled by two of the sums."""
    from model_cases import losses_inputs
    from test_counts_gpu import _run_losses
    for dice in (False, True):
        d = losses_inputs(4, False)
        ls0, g0 = _run_losses(dev, d, dice)
        assert np.all(np.isfinite(ls0)) and float(np.abs(ls0).sum()) > 0
        for _ in range(5):
            ls, g = _run_losses(dev, d, dice)
            np.testing.assert_array_equal(ls, ls0)
            for n in g0:
                np.testing.assert_array_equal(g[n], g0[n], err_msg=n)
