"""winograd_output_bwd_kernel + winograd_bwd_sums_kernel (ops.conv2d_dgrad_ep_winograd): the output transform of a data gradient
fused with the epilogue backward of the layer below.

dz is pinned EXACTLY: y = ops.conv2d_winograd(dz_above, Ut) runs the same transform code without an epilogue, and the expected
dz = where(mask, y, 0) * scale is one correctly rounded float32 multiply.  The channel sums are held to the first-order bound of
a float32 sum in any order, |got - ref64| <= n 2^-24 sum|terms|, n additions: the N H W terms of a channel
onto the value the buffer held before the call.

Shapes (tile, N, H, W, C), the smallest at which each path is taken: mixed tiling (all four instantiations, 128 / 64 lanes, a
ragged last workgroup), several workgroups per group, more tiles than the persistent grid holds (4 workgroups per CU: each walks
more than one), the uniform 4 x 4 tiling with tiles past the edge, the 2 x 2 instantiation alone, one ROI."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(6, 5, 14, 14, 256), (6, 9, 6, 10, 128), (6, 130, 14, 14, 256), (6, 260, 14, 14, 256), (4, 3, 7, 9, 128),
          (2, 5, 8, 12, 256), (6, 1, 14, 14, 256)]
CIN = 32            # channels of the gradient above: the transform-domain GEMM's K, irrelevant to the kernel under test
U24 = 2.0 ** -24
PREFILL = 0.75      # what the sum buffers hold before a call


def _ops():
    from caesar_mrcnn_amd import ops
    return ops


@functools.lru_cache(maxsize=None)
def _case(shape, seed=0):
    """Inputs on the device, y (the plain transform) and the masks: computed once per shape, never modified."""
    ops = _ops()
    tile, N, H, W, C = shape
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(900 + sum(shape) + seed)
    t = lambda a: torch.tensor(np.asarray(a, np.float32), device=dev)
    dz_above = t(rng.standard_normal((N, H, W, CIN)))
    Ut = ops.winograd_weights(t(rng.standard_normal((3, 3, CIN, C)) / np.sqrt(9 * CIN)), tile=tile)
    z = t(rng.standard_normal((N, H, W, C)))
    scale, shift = t(rng.uniform(0.5, 1.5, C)), t(rng.uniform(-0.3, 0.3, C))
    mean, rstd = t(rng.uniform(-0.5, 0.5, C)), t(rng.uniform(0.5, 1.5, C))
    z[0, 0, 0, :] = -shift / scale                              # scale * z + shift == 0, or within an ulp of it
    v = scale * z + shift                                       # mul, then add: the forward epilogue's expression
    y = ops.conv2d_winograd(dz_above, Ut)
    torch.cuda.synchronize()
    return dict(dz_above=dz_above, Ut=Ut, z=z, scale=scale, shift=shift, mean=mean, rstd=rstd, y=y, mask=v > 0,
                out=torch.clamp_min(v, 0.0))


def _sum_buffers(C, dev):
    return [torch.full((C,), PREFILL, device=dev) for _ in range(3)]


def _check_sums(shape, got, gg, dz, z, mean, rstd):
    """got = (dgamma, dbeta, dbias) after a call onto PREFILL; gg, dz float32 [N, H, W, C] as the kernel forms them"""
    _, N, H, W, C = shape
    n = N * H * W                                               # additions per channel: n terms onto the prefill
    gg, dz, z, mean, rstd = (a.cpu() for a in (gg, dz, z, mean, rstd))
    terms = {"dgamma": (gg * (z - mean)) * rstd, "dbeta": gg, "dbias": dz}      # float32, operation for operation
    for name, g in zip(("dgamma", "dbeta", "dbias"), got):
        t64 = terms[name].double().reshape(-1, C)
        ref = t64.sum(0) + PREFILL
        bound = n * U24 * (t64.abs().sum(0) + PREFILL)
        err = (g.double().cpu() - ref).abs()
        worst = int(torch.argmax(err / bound))
        print("%s %s: worst channel %d err %.3e bound %.3e" % (shape, name, worst, float(err[worst]), float(bound[worst])))
        assert bool((err <= bound).all()), (name, worst, float(err[worst]), float(bound[worst]))
        assert float((g - PREFILL).abs().max()) > 0


def _run(shape, form, c=None, sums=None):
    """one call of the op in one of its three mask forms; returns (dz, gg expected, dz expected, sums)"""
    ops = _ops()
    c = c or _case(shape)
    C = shape[4]
    dg, db, dbi = sums if sums is not None else _sum_buffers(C, c["y"].device)
    if form == "zmask":
        dz = ops.conv2d_dgrad_ep_winograd(c["dz_above"], c["Ut"], None, c["z"], c["scale"], c["mean"], c["rstd"], dg, db, dbi, ops.ACT_RELU,
                                          fwd_shift=c["shift"])
    elif form == "below_out":
        dz = ops.conv2d_dgrad_ep_winograd(c["dz_above"], c["Ut"], c["out"], c["z"], c["scale"], c["mean"], c["rstd"], dg, db, dbi, ops.ACT_RELU)
    else:
        dz = ops.conv2d_dgrad_ep_winograd(c["dz_above"], c["Ut"], None, c["z"], None, c["mean"], c["rstd"], dg, db, dbi, ops.ACT_NONE)
    torch.cuda.synchronize()
    if form == "none":
        return dz, c["y"], c["y"], (dg, db, dbi)
    gg = torch.where(c["mask"], c["y"], torch.zeros_like(c["y"]))
    return dz, gg, gg * c["scale"], (dg, db, dbi)


@pytest.mark.parametrize("form", ["zmask", "below_out", "none"])
@pytest.mark.parametrize("shape", SHAPES)
def test_dz_exact_and_sums(dev, shape, form):
    c = _case(shape)
    dz, gg, want, sums = _run(shape, form)
    assert torch.equal(dz, want)
    if form != "none":
        zero = float((dz == 0).float().mean())
        assert 0.2 <= zero <= 0.8, zero
        assert bool((c["mask"] == (c["out"] > 0)).all())
    _check_sums(shape, sums, gg, want, c["z"], c["mean"], c["rstd"])


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[4]])
def test_null_sums_write_nothing_else(dev, shape):
    """dgamma = dbeta = None: only dbias is added to; guards around it stay as they were"""
    ops = _ops()
    c = _case(shape)
    C = shape[4]
    buf = torch.full((3 * C,), PREFILL, device=dev)
    dz = ops.conv2d_dgrad_ep_winograd(c["dz_above"], c["Ut"], None, c["z"], c["scale"], None, None, None, None, buf[C:2 * C], ops.ACT_RELU,
                                      fwd_shift=c["shift"])
    torch.cuda.synchronize()
    gg = torch.where(c["mask"], c["y"], torch.zeros_like(c["y"]))
    assert torch.equal(dz, gg * c["scale"])
    assert bool((buf[:C] == PREFILL).all()) and bool((buf[2 * C:] == PREFILL).all())
    t64 = (gg * c["scale"]).double().reshape(-1, C).cpu()
    n = t64.shape[0]
    err = (buf[C:2 * C].double().cpu() - (t64.sum(0) + PREFILL)).abs()
    assert bool((err <= n * U24 * (t64.abs().sum(0) + PREFILL)).all())


@pytest.mark.parametrize("shape", [SHAPES[2], SHAPES[4]])
def test_partials_workspace_reuse(dev, shape):
    """Two calls back to back on one stream share the partials workspace: different inputs must both give their own sums (stale
    partials, a reduction launched before the last group), and the same inputs twice the same bits (fixed-order reduction)."""
    ops = _ops()
    a, b = _case(shape), _case(shape, 1)
    C = shape[4]
    sa, sb, sa2 = _sum_buffers(C, dev), _sum_buffers(C, dev), _sum_buffers(C, dev)
    call = lambda c, s: ops.conv2d_dgrad_ep_winograd(c["dz_above"], c["Ut"], None, c["z"], c["scale"], c["mean"], c["rstd"], s[0], s[1], s[2],
                                                     ops.ACT_RELU, fwd_shift=c["shift"])
    dza, dzb, dza2 = call(a, sa), call(b, sb), call(a, sa2)                     # no synchronisation in between
    torch.cuda.synchronize()
    for c, dz, s in ((a, dza, sa), (b, dzb, sb)):
        gg = torch.where(c["mask"], c["y"], torch.zeros_like(c["y"]))
        assert torch.equal(dz, gg * c["scale"])
        _check_sums(shape, s, gg, gg * c["scale"], c["z"], c["mean"], c["rstd"])
    assert torch.equal(dza, dza2)
    for u, v in zip(sa, sa2):
        assert torch.equal(u, v)
