"""The backward chain between the data gradients of two 3 x 3 Winograd layers (mrcnn_winograd_bwd_chain, the chain form of
ops.conv2d_dgrad_ep_winograd, ops.conv2d_wgrad_winograd(dm_ready=...), engine._mask_head_bwd_rows): the four output transforms with
the epilogue backward of the layer below, and both transforms of the resulting dz -- B^T dz B for the next data gradient, A dz A^T
for the weight gradient -- as one launch, dz kept in LDS.  It computes the separate launches' expressions in their order, so dz, V
and dM must equal mrcnn_winograd_output_bwd_zmask_g + mrcnn_winograd_input_g + mrcnn_winograd_dy_g BIT FOR BIT (all buffers start
as zeros, so the padded rows compare too); the channel sums, whose order of addition differs, are held to the first-order float32
bound against float64 of test_winograd_output_bwd_gpu.py, n 2^-24 (sum|terms| + prefill), and must not change from run to run."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# (N, H, W, C): the smallest map with all four groups; a non-square map; two channel slices; more maps than one round of workgroups
# (130 maps x 2 slices over 256 CUs x 3) and tile counts that are no multiple of a 128-row GEMM tile
# -- all with 64-channel slices (8 tiles in flight); then the maps at which the slice narrows to 32, 16 and 8 channels (16, 32, 64
# tiles in flight, two to sixteen of them per wave, another shape of the sums stage)
CASES = [(1, 6, 6, 128), (3, 10, 6, 128), (9, 14, 14, 256), (130, 14, 14, 128), (2, 18, 18, 128), (1, 22, 22, 128), (1, 30, 30, 128)]
MIXED = 6
U24 = 2.0 ** -24
PREFILL = 0.75      # what the sum buffers hold before a call


def _ops():
    from caesar_mrcnn_amd import ops
    return ops


def _lib():
    from caesar_mrcnn_amd import _hip
    return _hip, _hip.lib()


def _floats(N, H, W, Cc, tile=MIXED):
    """the tile groups of a map and the floats of each group's transform-domain matrices"""
    ops = _ops()
    _, lib = _lib()
    groups = ops.winograd_groups(H, W, tile)
    return groups, [lib.mrcnn_winograd_group_floats(C.byref(g), N, Cc) for g in groups]


def _separate(Mt, c, N, H, W, Cc, tile=MIXED, sums=None):
    """The launches the chain replaces, from the same Mt: dz, V, dM (zeros where nothing is written), sums added to `sums`."""
    hip, lib = _lib()
    ops = _ops()
    dev = Mt.device
    groups, nms = _floats(N, H, W, Cc, tile)
    dz = torch.zeros((N, H, W, Cc), device=dev)
    V, dM = torch.zeros(sum(nms), device=dev), torch.zeros(sum(nms), device=dev)
    rows = [lib.mrcnn_winograd_output_bwd_rows(C.byref(g), N, Cc) for g in groups]
    part = torch.zeros(sum(rows) * 3 * Cc, device=dev)
    p = hip.ptr
    st = hip.current_stream()
    off = done = 0
    for g, nm, r in zip(groups, nms, rows):
        pp = p(part) + done * 3 * Cc * 4 if sums is not None else None
        ops.check(lib.mrcnn_winograd_output_bwd_zmask_g(p(Mt) + off * 4, p(dz), p(c["z"]), p(c["scale"]), p(c["shift"]),
                                                        p(c["mean"]) if sums is not None else None, p(c["rstd"]) if sums is not None else None,
                                                        pp, N, H, W, Cc, C.byref(g), st), "zmask_g")
        off += nm
        done += r
    off = 0
    for g, nm in zip(groups, nms):
        ops.check(lib.mrcnn_winograd_input_g(p(dz), p(V) + off * 4, N, H, W, Cc, C.byref(g), st), "input_g")
        ops.check(lib.mrcnn_winograd_dy_g(p(dz), p(dM) + off * 4, N, H, W, Cc, C.byref(g), st), "dy_g")
        off += nm
    if sums is not None:
        ops.check(lib.mrcnn_winograd_output_bwd_sums(p(part), done, Cc, p(sums[0]), p(sums[1]), p(sums[2]), st), "sums")
    torch.cuda.synchronize()
    return dz, V, dM


def _chain(Mt, c, N, H, W, Cc, with_dz=True, with_dm=True, sums=None, tile=MIXED, fill=0.0):
    """One mrcnn_winograd_bwd_chain launch (+ the sums launch); returns rc, dz, V, dM, partials."""
    hip, lib = _lib()
    ops = _ops()
    dev = Mt.device
    _, nms = _floats(N, H, W, Cc, tile)
    dz = torch.full((N, H, W, Cc), fill, device=dev)
    V, dM = torch.full((sum(nms),), fill, device=dev), torch.full((sum(nms),), fill, device=dev)
    part = torch.full((N * 3 * Cc + 64,), 7.0, device=dev)
    p = hip.ptr
    st = hip.current_stream()
    want = sums is not None
    rc = lib.mrcnn_winograd_bwd_chain(p(Mt), p(c["z"]), p(c["scale"]), p(c["shift"]), p(c["mean"]) if want else None,
                                      p(c["rstd"]) if want else None, p(part) if want else None, p(V), p(dM) if with_dm else None,
                                      p(dz) if with_dz else None, N, H, W, Cc, tile, st)
    if rc == 0 and want:
        ops.check(lib.mrcnn_winograd_output_bwd_sums(p(part), N, Cc, p(sums[0]), p(sums[1]), p(sums[2]), st), "sums")
    torch.cuda.synchronize()
    return rc, dz, V, dM, part


@functools.lru_cache(maxsize=None)
def _case(case, seed=0):
    """Inputs on the device and the separate launches' results: computed once per case, never modified."""
    N, H, W, Cc = case
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(1300 + sum(case) + seed)
    t = lambda a: torch.tensor(np.asarray(a, np.float32), device=dev)
    _, nms = _floats(N, H, W, Cc)
    c = dict(Mt=t(rng.standard_normal(sum(nms))), z=t(rng.standard_normal((N, H, W, Cc))), scale=t(rng.uniform(0.5, 1.5, Cc)),
             shift=t(rng.uniform(-0.3, 0.3, Cc)), mean=t(rng.uniform(-0.5, 0.5, Cc)), rstd=t(rng.uniform(0.5, 1.5, Cc)))
    c["dz"], c["V"], c["dM"] = _separate(c["Mt"], c, N, H, W, Cc)
    # gg as the kernels form it: y = A^T m A by the plain output transform (the same wino_at sequences, no epilogue), masked with
    # the forward epilogue's expression (a multiply, then an add); dz = gg * scale is one correctly rounded multiply
    hip, lib = _lib()
    groups, _ = _floats(N, H, W, Cc)
    y = torch.zeros((N, H, W, Cc), device=dev)
    off = 0
    for g, nm in zip(groups, nms):
        _ops().check(lib.mrcnn_winograd_output_g(hip.ptr(c["Mt"]) + off * 4, hip.ptr(y), None, None, None, None, N, H, W, Cc, 0, C.byref(g),
                                                 hip.current_stream()), "output_g")
        off += nm
    c["gg"] = torch.where(c["scale"] * c["z"] + c["shift"] > 0, y, torch.zeros_like(y))
    torch.cuda.synchronize()
    assert torch.equal(c["dz"], c["gg"] * c["scale"])
    return c


def _check_sums(case, got, gg, dz, z, mean, rstd):
    """got = (dgamma, dbeta, dbias) after a call onto PREFILL; gg, dz float32 [N, H, W, C] as the kernel forms them
    (test_winograd_output_bwd_gpu.py's check, its bound)"""
    N, H, W, Cc = case
    n = N * H * W                                               # additions per channel: n terms onto the prefill
    gg, dz, z, mean, rstd = (a.cpu() for a in (gg, dz, z, mean, rstd))
    terms = {"dgamma": (gg * (z - mean)) * rstd, "dbeta": gg, "dbias": dz}      # float32, operation for operation
    for name, g in zip(("dgamma", "dbeta", "dbias"), got):
        t64 = terms[name].double().reshape(-1, Cc)
        ref = t64.sum(0) + PREFILL
        bound = n * U24 * (t64.abs().sum(0) + PREFILL)
        err = (g.double().cpu() - ref).abs()
        worst = int(torch.argmax(err / bound))
        print("%s %s: worst channel %d err %.3e bound %.3e" % (case, name, worst, float(err[worst]), float(bound[worst])))
        assert bool((err <= bound).all()), (name, worst, float(err[worst]), float(bound[worst]))
        assert float((g - PREFILL).abs().max()) > 0


@pytest.mark.parametrize("with_sums", [True, False])
@pytest.mark.parametrize("with_dm", [True, False])
@pytest.mark.parametrize("with_dz", [True, False])
@pytest.mark.parametrize("case", CASES)
def test_one_launch_equals_the_separate_launches(dev, case, with_dz, with_dm, with_sums):
    N, H, W, Cc = case
    c = _case(case)
    sums = [torch.full((Cc,), PREFILL, device=dev) for _ in range(3)] if with_sums else None
    rc, dz, V, dM, part = _chain(c["Mt"], c, N, H, W, Cc, with_dz, with_dm, sums)
    assert rc == 0, "the one-launch kernel refused a shape it is required to take"
    assert float(c["V"].abs().max()) > 0 and float(c["dM"].abs().max()) > 0
    zero = float((c["dz"] == 0).float().mean())
    assert 0.2 <= zero <= 0.8, zero
    assert torch.equal(V, c["V"])
    assert torch.equal(dz, c["dz"] if with_dz else torch.zeros_like(dz))
    assert torch.equal(dM, c["dM"] if with_dm else torch.zeros_like(dM))
    if with_sums:
        assert bool((part[N * 3 * Cc:] == 7.0).all())              # N rows of partials, no more
        _check_sums(case, sums, c["gg"], c["dz"], c["z"], c["mean"], c["rstd"])
        again = [torch.full((Cc,), PREFILL, device=dev) for _ in range(3)]
        _chain(c["Mt"], c, N, H, W, Cc, with_dz, with_dm, again)
        for u, v in zip(sums, again):
            assert torch.equal(u, v)                                # fixed order of addition: the same bits every run
    else:
        assert bool((part == 7.0).all())


def test_null_sums_write_nothing_but_the_outputs(dev):
    """No partials: the outputs equal the separate launches', the rows past the last tile keep what they held, and the ops form
    with dgamma = dbeta = None adds to dbias alone."""
    ops = _ops()
    case = CASES[1]
    N, H, W, Cc = case
    c = _case(case)
    rc, dz, V, dM, part = _chain(c["Mt"], c, N, H, W, Cc, True, True, None, fill=3.0)
    assert rc == 0 and bool((part == 7.0).all())
    groups, nms = _floats(N, H, W, Cc)
    off = 0
    for g, nm in zip(groups, nms):
        nb, T = (g.oth + 2) * (g.otw + 2), N * g.th_n * g.tw_n
        for got, want in ((V, c["V"]), (dM, c["dM"])):
            got, want = got[off:off + nm].view(nb, -1, Cc), want[off:off + nm].view(nb, -1, Cc)
            assert torch.equal(got[:, :T], want[:, :T]) and bool((got[:, T:] == 3.0).all())
        off += nm
    assert torch.equal(dz, c["dz"])
    # the ops form: a data gradient through random weights, dbias only
    rng = np.random.default_rng(3)
    t = lambda a: torch.tensor(np.asarray(a, np.float32), device=dev)
    dz_above = t(rng.standard_normal((N, H, W, 32)))
    Ut = ops.winograd_weights(t(rng.standard_normal((3, 3, 32, Cc)) / np.sqrt(9 * 32)), tile=ops.TILE_MIXED)
    buf1, buf2 = torch.full((3 * Cc,), PREFILL, device=dev), torch.full((3 * Cc,), PREFILL, device=dev)
    want = ops.conv2d_dgrad_ep_winograd(dz_above, Ut, None, c["z"], c["scale"], None, None, None, None, buf1[Cc:2 * Cc], ops.ACT_RELU,
                                        fwd_shift=c["shift"])
    Vn = torch.zeros(sum(nms), device=dev)
    got = ops.conv2d_dgrad_ep_winograd(dz_above, Ut, None, c["z"], c["scale"], None, None, None, None, buf2[Cc:2 * Cc], ops.ACT_RELU,
                                       fwd_shift=c["shift"], next_v=Vn, dz_out=torch.zeros_like(want))
    torch.cuda.synchronize()
    assert torch.equal(got, want) and float(Vn.abs().max()) > 0
    assert bool((buf2[:Cc] == PREFILL).all()) and bool((buf2[2 * Cc:] == PREFILL).all())
    t64 = want.double().reshape(-1, Cc).cpu()
    err = (buf2[Cc:2 * Cc].double().cpu() - (t64.sum(0) + PREFILL)).abs()
    assert bool((err <= t64.shape[0] * U24 * (t64.abs().sum(0) + PREFILL)).all())


def test_on_the_relu_edge(dev):
    """scale * z + shift exactly 0 in every channel of two pixels (the 2 x 2 and the 2 x 4 group), and a few ulps either side of it
    on two more (the 4 x 4 and the 4 x 2 group): shift = -(scale * z) of one pixel, the float32 product and its negation cancel
    exactly.  The masks, and so every output, are the separate launches' bits."""
    case = (3, 10, 6, 128)
    N, H, W, Cc = case
    base = _case(case)
    c = {k: base[k].clone() for k in ("Mt", "z", "scale", "shift", "mean", "rstd")}
    z0 = c["z"][1, H - 1, W - 1, :].clone()
    c["shift"] = -(c["scale"] * z0)
    c["z"][1, H - 1, 0, :] = z0
    c["z"][1, 0, 0, :] = z0 * (1 + 2.0 ** -21)
    c["z"][1, 0, W - 1, :] = z0 * (1 - 2.0 ** -21)
    v = c["scale"] * c["z"] + c["shift"]
    assert bool((v[1, H - 1, W - 1] == 0).all()) and bool((v[1, H - 1, 0] == 0).all())
    assert bool((v[1, 0, 0] != 0).all()) and bool((v[1, 0, W - 1] != 0).all())
    assert bool((torch.sign(v[1, 0, 0]) == -torch.sign(v[1, 0, W - 1])).all())
    dz1, V1, dM1 = _separate(c["Mt"], c, N, H, W, Cc)
    rc, dz2, V2, dM2, _ = _chain(c["Mt"], c, N, H, W, Cc)
    assert rc == 0
    assert bool((dz1[1, H - 1, W - 1] == 0).all()) and bool((dz1[1, H - 1, 0] == 0).all())
    assert bool(((dz1[1, 0, 0] != 0) != (dz1[1, 0, W - 1] != 0)).all())          # exactly one side of the edge passes the gradient
    assert torch.equal(dz1, dz2) and torch.equal(V1, V2) and torch.equal(dM1, dM2)


@pytest.mark.parametrize("what, tile, H, C_", [("uniform 4 x 4 tiling", 4, 14, 128), ("uniform 2 x 2 tiling", 2, 14, 128),
                                               ("channels not in 128s", MIXED, 14, 64), ("a map over 2048 pixels", MIXED, 46, 128)])
def test_entry_refuses_before_any_launch(dev, what, tile, H, C_):
    hip, lib = _lib()
    ops = _ops()
    N = 2
    n = 100 * 384 * C_                                              # more than all groups of these shapes
    Mt = torch.zeros(n, device=dev)
    V, dM = torch.full((n,), 3.0, device=dev), torch.full((n,), 4.0, device=dev)
    dz, z = torch.full((N, H, H, C_), 5.0, device=dev), torch.zeros((N, H, H, C_), device=dev)
    part = torch.full((N * 3 * C_,), 6.0, device=dev)
    one = torch.ones(C_, device=dev)
    p = hip.ptr
    rc = lib.mrcnn_winograd_bwd_chain(p(Mt), p(z), p(one), p(one), p(one), p(one), p(part), p(V), p(dM), p(dz), N, H, H, C_, tile,
                                      hip.current_stream())
    torch.cuda.synchronize()
    assert rc == ops.ERR_UNSUPPORTED, what
    assert bool((V == 3.0).all()) and bool((dM == 4.0).all()) and bool((dz == 5.0).all()) and bool((part == 6.0).all()), what


@pytest.mark.parametrize("what, tile, N, H, Cc", [("uniform 4 x 4 tiling", 4, 3, 10, 128), ("uniform 2 x 2 tiling", 2, 3, 10, 128),
                                                  ("channels not in 128s", MIXED, 3, 10, 64), ("a map over 2048 pixels", MIXED, 1, 46, 128)])
def test_ops_take_the_separate_launches_where_the_kernel_refuses(dev, what, tile, N, H, Cc):
    """conv2d_dgrad_ep_winograd's chain form on a shape the entry refuses: it returns dz and has written next_v and next_dm, all as
    the separate calls do, and the sums are the separate calls' bits; the weight gradient from dm_ready equals the one from dz.
    With 64 channels the module's transform-domain GEMM does not run at all (whole 128s), in the plain form either: that case
    hands the product in (mt_ready) and is compared with the separate entries on the same Mt."""
    ops = _ops()
    hip, lib = _lib()
    Cin = 32
    rng = np.random.default_rng(11 + tile + H + Cc)
    t = lambda a: torch.tensor(np.asarray(a, np.float32), device=dev)
    Ut = ops.winograd_weights(t(rng.standard_normal((3, 3, Cin, Cc)) / np.sqrt(9 * Cin)), tile=tile)
    z, scale, shift = t(rng.standard_normal((N, H, H, Cc))), t(rng.uniform(0.5, 1.5, Cc)), t(rng.uniform(-0.3, 0.3, Cc))
    mean, rstd = t(rng.uniform(-0.5, 0.5, Cc)), t(rng.uniform(0.5, 1.5, Cc))
    s1, s2 = [torch.full((Cc,), PREFILL, device=dev) for _ in range(3)], [torch.full((Cc,), PREFILL, device=dev) for _ in range(3)]
    groups, nms = _floats(N, H, H, Cc, tile)

    def transforms(x, entry, C_):
        """entry (mrcnn_winograd_input_g / _dy_g) of every group of x, end to end"""
        gs, ns = _floats(N, H, H, C_, tile)
        out = torch.zeros(sum(ns), device=dev)
        off = 0
        for g, n in zip(gs, ns):
            ops.check(entry(hip.ptr(x), hip.ptr(out) + off * 4, N, H, H, C_, C.byref(g), hip.current_stream()), "transform")
            off += n
        return out

    V2, dM2 = torch.zeros(sum(nms), device=dev), torch.zeros(sum(nms), device=dev)
    if Cc % 128 == 0:
        dz_above = t(rng.standard_normal((N, H, H, Cin)))
        call = lambda s, **k: ops.conv2d_dgrad_ep_winograd(dz_above, Ut, None, z, scale, mean, rstd, s[0], s[1], s[2], ops.ACT_RELU,
                                                           fwd_shift=shift, **k)
        want = call(s1)
        V1, dM1 = transforms(want, lib.mrcnn_winograd_input_g, Cc), transforms(want, lib.mrcnn_winograd_dy_g, Cc)
        got = call(s2, next_v=V2, next_dm=dM2)
    else:
        Mt = t(rng.standard_normal(sum(nms)))
        c = dict(z=z, scale=scale, shift=shift, mean=mean, rstd=rstd)
        want, V1, dM1 = _separate(Mt, c, N, H, H, Cc, tile, sums=s1)
        got = ops.conv2d_dgrad_ep_winograd((N, H, H, Cin), Ut, None, z, scale, mean, rstd, s2[0], s2[1], s2[2], ops.ACT_RELU,
                                           fwd_shift=shift, next_v=V2, next_dm=dM2, mt_ready=Mt)
    torch.cuda.synchronize()
    assert got is not None and torch.equal(got, want) and torch.equal(V1, V2) and torch.equal(dM1, dM2), what
    assert float(V1.abs().max()) > 0 and float(dM1.abs().max()) > 0 and float(want.abs().max()) > 0
    for u, v in zip(s1, s2):
        assert torch.equal(u, v) and float((u - PREFILL).abs().max()) > 0, what      # the same launches in the same order: the same sums
    # weight gradient of the layer below (32 input channels): from dz, and from dm_ready with dz given as a shape
    Vx = transforms(t(rng.standard_normal((N, H, H, 32))), lib.mrcnn_winograd_input_g, 32)
    dw1, dw2 = torch.zeros((3, 3, 32, Cc), device=dev), torch.zeros((3, 3, 32, Cc), device=dev)
    ops.conv2d_wgrad_winograd(Vx, (N, H, H, 32), want, dw1, tile=tile)
    ops.conv2d_wgrad_winograd(Vx, (N, H, H, 32), (N, H, H, Cc), dw2, tile=tile, dm_ready=dM2)
    torch.cuda.synchronize()
    assert torch.equal(dw1, dw2) and float(dw1.abs().max()) > 0, what


def test_ops_chain_form_runs_the_one_launch(dev):
    """(9, 14, 14, 256) through ops: the chain form returns None (no dz anywhere), next_v / next_dm equal the transforms of the plain
    form's dz, the next data gradient from v_ready equals the one from dz, bit for bit."""
    ops = _ops()
    hip, lib = _lib()
    N, H, Cc, Cin = 9, 14, 256, 32
    rng = np.random.default_rng(23)
    t = lambda a: torch.tensor(np.asarray(a, np.float32), device=dev)
    dz_above = t(rng.standard_normal((N, H, H, Cin)))
    Ut = ops.winograd_weights(t(rng.standard_normal((3, 3, Cin, Cc)) / np.sqrt(9 * Cin)), tile=ops.TILE_MIXED)
    Ut2 = ops.winograd_weights(t(rng.standard_normal((3, 3, Cc, 128)) / np.sqrt(9 * Cc)), tile=ops.TILE_MIXED)
    z, scale, shift = t(rng.standard_normal((N, H, H, Cc))), t(rng.uniform(0.5, 1.5, Cc)), t(rng.uniform(-0.3, 0.3, Cc))
    mean, rstd = t(rng.uniform(-0.5, 0.5, Cc)), t(rng.uniform(0.5, 1.5, Cc))
    s1, s2 = [torch.full((Cc,), PREFILL, device=dev) for _ in range(3)], [torch.full((Cc,), PREFILL, device=dev) for _ in range(3)]
    call = lambda s, **k: ops.conv2d_dgrad_ep_winograd(dz_above, Ut, None, z, scale, mean, rstd, s[0], s[1], s[2], ops.ACT_RELU,
                                                       fwd_shift=shift, **k)
    want = call(s1)
    d1 = ops.conv2d_winograd(want, Ut2)
    nv = ops.winograd_v_floats((N, H, H, Cc), ops.TILE_MIXED)
    V2, dM2 = torch.zeros(nv, device=dev), torch.zeros(nv, device=dev)
    got = call(s2, next_v=V2, next_dm=dM2)
    assert got is None, "the one-launch kernel refused a shape it is required to take"
    d2 = ops.conv2d_winograd((N, H, H, Cc), Ut2, keep_v=V2, v_ready=True)
    torch.cuda.synchronize()
    assert torch.equal(d1, d2) and float(d1.abs().max()) > 0
    y = ops.conv2d_winograd(dz_above, Ut)                       # the same transform code without an epilogue
    gg = torch.where(scale * z + shift > 0, y, torch.zeros_like(y))
    assert torch.equal(want, gg * scale)
    _check_sums((N, H, H, Cc), s2, gg, want, z, mean, rstd)


# ---- engine level: 512 ROIs of 14 x 14, the smallest count at which ops.winograd_tile picks the mixed tiling -----------------------
def _engine(dev, seed):
    import test_engine_gpu as T
    from caesar_mrcnn_amd.model import MaskRCNN
    cfg = T._full_cfg("resnet50", 256, nimg=1)
    model = MaskRCNN("training", cfg, "/tmp/mrcnn_logs", device=dev, weights=T._weights(cfg, seed))
    return T, cfg, model


def test_mask_head_backward_chained_equals_unchained(dev, monkeypatch):
    """The mask head's backward on 512 ROIs with the switch on, off, and off once more.  What depends only on dz, V and dM is equal
    bit for bit: dW of the four layers, and the head's data gradient d [512, 14, 14, 256] as it is handed to the ROIAlign adjoint.
    The pyramid gradients are that adjoint's scatter of d with float atomics (roialign.hip), whose order changes from run to run:
    they are held to the bar of the sums (2e-5 of their largest entry), and the run-to-run difference of the unchained backward
    with itself is printed beside the chained one's (measured: level 0, largest entry 1.06e-4, chained - unchained 8.0e-11,
    unchained - unchained again 1.0e-10; level 1 3.3e-11 both).  d-gamma / d-beta / d-bias differ by the order of their sums only (2e-5 of
    the largest gradient entry)."""
    from caesar_mrcnn_amd import ops, _hip
    T, cfg, model = _engine(dev, 31)
    eng = model.engine
    assert eng.winograd_bwd_chain and cfg.TRAIN_ROIS_PER_IMAGE == 512
    assert ops.winograd_tile((512, 14, 14, 256)) == ops.TILE_MIXED
    calls, adjoint_in = [], []
    real, real_adjoint = ops.conv2d_dgrad_ep_winograd, ops.roialign_bwd

    def spy(*a, **k):
        out = real(*a, **k)
        calls.append((k.get("next_v") is not None, out is None))
        return out

    def spy_adjoint(rois_, d, *a, **k):
        adjoint_in.append(d.clone())
        return real_adjoint(rois_, d, *a, **k)
    monkeypatch.setattr(ops, "conv2d_dgrad_ep_winograd", spy)
    monkeypatch.setattr(ops, "roialign_bwd", spy_adjoint)
    rng = np.random.default_rng(9)
    images = torch.tensor(rng.uniform(-100, 100, (1, 256, 256, 3)).astype(np.float32), device=dev)
    yx = rng.uniform(0, 0.6, (1, 512, 2))
    rois = torch.tensor(np.concatenate([yx, yx + rng.uniform(0.05, 0.4, (1, 512, 2))], axis=2).astype(np.float32), device=dev)
    eng.refresh_wt()
    pyr, _, p16h, _ = eng._trunk_fwd(images, True)
    area = float(256 * 256)
    d_mmask = None
    runs = []
    for on in (True, False, False):
        eng.winograd_bwd_chain = on
        masks, ctxs = eng._mask_head_fwd(rois, pyr[:4], p16h, area, True)      # (bit-identical from run to run)
        if d_mmask is None:
            d_mmask = torch.tensor(rng.standard_normal(tuple(masks.shape)).astype(np.float32) * 1e-3, device=dev)
        eng.grads.zero_()
        dP = [torch.zeros_like(p) for p in pyr[:4]]
        del calls[:]
        ev = _hip.ev_record(torch.cuda.current_stream(dev))
        eng._mask_head_bwd(d_mmask, ctxs, rois, dP, area, ev)
        eng.join_wgrad()
        torch.cuda.synchronize()
        assert calls == ([(True, True)] * 3 if on else [(False, False)] * 3), calls
        runs.append((eng.grads.clone(), dP))
    (g1, p1), (g0, p0), (g00, p00) = runs
    assert len(adjoint_in) == 3 and float(adjoint_in[1].abs().max()) > 0
    assert torch.equal(adjoint_in[0], adjoint_in[1]) and torch.equal(adjoint_in[1], adjoint_in[2])
    for i in range(1, 5):
        op = eng.op("mrcnn_mask_conv%d" % i)
        lo, n = (op.dw.data_ptr() - eng.grads.data_ptr()) // 4, op.dw.numel()
        assert torch.equal(g1[lo:lo + n], g0[lo:lo + n]) and float(g0[lo:lo + n].abs().max()) > 0, i
    for lvl, (a, b, b2) in enumerate(zip(p1, p0, p00)):
        top = float(b.abs().max())
        print("pyramid gradient %d: largest entry %.3e, chained - unchained %.3e, unchained - unchained again %.3e"
              % (lvl, top, float((a - b).abs().max()), float((b - b2).abs().max())))
        assert float((a - b).abs().max()) <= 2e-5 * top                    # (a level no ROI is assigned to: zero in both)
        # and no more than the adjoint's own run-to-run noise on identical input: 8 x the unchained pair's difference, or, where
        # that pair happens to agree closely, 8 float32 ulps of the level's largest entry
        assert float((a - b).abs().max()) <= max(8 * float((b - b2).abs().max()), 2.0 ** -20 * top)
    assert max(float(b.abs().max()) for b in p0) > 0
    scale = float(g0.abs().max())
    print("gradients: largest entry %.3e, chained - unchained %.3e, unchained - unchained again %.3e"
          % (scale, float((g1 - g0).abs().max()), float((g0 - g00).abs().max())))
    assert scale > 0 and float((g1 - g0).abs().max()) <= 2e-5 * scale


def test_training_step_with_the_backward_chain(dev, monkeypatch):
    """One forward_backward with all 512 ROIs in the mask head (sparse_mask_bwd off, as test_training_step_with_the_chain), the
    backward chain on and off on the same seeded batch and weights, at that test's bars: losses rtol 5e-6, gradients 2e-5 of
    their largest entry.  With the switch on the three linked launches are issued, each by the one-launch kernel."""
    from caesar_mrcnn_amd import ops
    calls = []
    real = ops.conv2d_dgrad_ep_winograd

    def spy(*a, **k):
        out = real(*a, **k)
        calls.append((k.get("next_v") is not None, out is None))
        return out
    monkeypatch.setattr(ops, "conv2d_dgrad_ep_winograd", spy)
    res = {}
    for on in (True, False):
        T, cfg, model = _engine(dev, 37)
        eng = model.engine
        assert eng.winograd_bwd_chain
        eng.winograd_bwd_chain = on
        eng.sparse_mask_bwd = False
        inputs, keys = T._train_inputs(cfg, 1, 43)
        del calls[:]
        losses = model.train_on_batch(inputs, rand_keys=keys, apply=False)
        torch.cuda.synchronize()
        assert calls == ([(True, True)] * 3 if on else [(False, False)] * 3), calls
        res[on] = (losses.cpu().numpy(), eng.grads.cpu().numpy().copy())
        del model, eng
    got = res[True][0]
    assert got.shape == (5,) and np.all(np.isfinite(got)) and np.all(np.isfinite(res[True][1])), got
    np.testing.assert_allclose(res[True][0], res[False][0], rtol=5e-6)
    scale = np.abs(res[False][1]).max()
    assert scale > 0 and np.abs(res[True][1] - res[False][1]).max() <= 2e-5 * scale
