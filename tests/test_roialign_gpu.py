"""csrc/roialign.hip (float32 forward, scatter adjoint, gather adjoint, the two 16-bit forms) against the float64 statement of
tests/roialign_cases.py on the boxes and shapes the parity tests of test_kernels_gpu.py / test_h16_gpu.py never feed it:
non-square maps, C below a wave and with a ragged channel trip, row counts that leave the last workgroup partly filled, P = 1, 2,
32 and 33, boxes beside the half-way level sizes and at the clamps, inverted / empty / outside boxes, gather rounds whose entries
carry fractional weights, and the fall-back of dense=True to the scatter form.

All checks are elementwise, with u = 2^-24 (roialign_cases.fwd_bound / adj_bound carry the derivations):
  forward   |got - ref64| <= 12 u corner_max, outside bins exactly 0, levels exactly those of the oracle
  adjoint   maps pre-filled with 0.25: |got - 0.25 - sum| <= (n + 6) u abs_sum + min(n, adds) u 0.25; n = 0 keeps exactly 0.25
  16 bit    forward e |ref64| + 12 u corner_max + t (e = 2^-11, t = 2^-25 float16; e = 2^-8, t = 0 bfloat16); adjoint with n + 7
tests/test_roialign_cpu.py checks without a GPU that the cases reach what they are for."""
import ctypes as C

import numpy as np
import pytest
import torch

import mrcnn_oracle as orc
import roialign_cases as rc

pytestmark = pytest.mark.gpu

PREFILL = 0.25
GATHER = ("p33", "stage", "wrap", "rect", "p32")     # C = 256: the gather form takes them (p33 with P lowered to 32)


def _ops():
    from caesar_mrcnn_amd import ops
    return ops


def _hip():
    from caesar_mrcnn_amd import _hip
    return _hip


@pytest.fixture(scope="module")
def ref():
    """Per case, computed once and left unchanged: the case, its maps and gradient, the float64 forward and adjoint."""
    cache = {}

    def get(name, forward=True):
        d = cache.setdefault(name, {})
        if not d:
            c = rc.CASES[name]()
            d.update(case=c, fms=rc.case_maps(name), dout=rc.case_dout(name))
            d["adj"] = rc.roialign_adj64(c.rois, d["dout"], c.shapes, c.P, c.area)
        if forward and "fwd" not in d:
            d["fwd"] = rc.roialign_ref64(d["case"].rois, d["fms"], d["case"].P, d["case"].area)
        return d
    return get


def _prefilled(c, dev):
    return [torch.full((c.rois.shape[0], H, W, c.C), PREFILL, device=dev) for H, W in c.shapes]


def _check_adjoint(tag, maps, adj, extra=6, adds=None):
    worst = first = 0.0
    for a, m in zip(maps, adj):
        a = a.cpu().numpy()
        assert (a[m["n"] == 0] == np.float32(PREFILL)).all(), tag + ": a pixel no bin reaches was written"
        err = np.abs(a.astype(np.float64) - PREFILL - m["sum"])
        worst = max(worst, rc.worst_ratio(err, rc.adj_bound(m, extra=extra, prefill=PREFILL, adds=adds)))
        # for the record: the bound as first written, 2 u 0.25 for the pre-fill whatever the number of additions (see rc.adj_bound)
        first = max(first, rc.worst_ratio(err, (m["n"][..., None] + extra) * rc.U * m["abs_sum"] + 2 * rc.U * PREFILL))
    print("[%s] max |err| / ((n + %d) u abs_sum + %s u 0.25) = %.3f (with 2 u 0.25: %.3f)"
          % (tag, extra, "n" if adds is None else "min(n, %d)" % adds, worst, first))
    assert worst <= 1.0, tag


def _gather_direct(c, boxes, dout, maps, P=None):
    """mrcnn_roialign_bwd_gather itself, with the descriptor ops.roialign_bwd builds: its status says which route dense=True takes."""
    ops, hip = _ops(), _hip()
    d = ops._roi_desc(boxes, maps, c.P if P is None else P, c.area)
    rc_ = hip.lib().mrcnn_roialign_bwd_gather(C.byref(d), hip.ptr(boxes), hip.ptr(dout), hip.ptr(maps[0]), hip.ptr(maps[1]),
                                              hip.ptr(maps[2]), hip.ptr(maps[3]), hip.current_stream())
    torch.cuda.synchronize()
    return rc_


# ---- float32 forward -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["odd", "thin", "p1", "p2", "p33", "rect", "p32"])
def test_forward_f32(dev, ref, name):
    d = ref(name); c = d["case"]
    out64, cmax, levels = d["fwd"]
    got, lv = _ops().roialign(torch.tensor(c.rois, device=dev), [torch.tensor(f, device=dev) for f in d["fms"]], c.P, c.area,
                              want_levels=True)
    torch.cuda.synchronize()
    assert torch.equal(lv.cpu().long(), orc.roi_levels(c.rois, c.area))
    got = got.cpu().numpy()
    assert got.shape == out64.shape
    assert (got[cmax == 0] == 0).all()                                     # outside bins are exactly 0.0
    ratio = rc.worst_ratio(np.abs(got.astype(np.float64) - out64), rc.fwd_bound(cmax) * np.ones_like(out64))
    print("[roialign fwd %s] max |err| / (12 u corner_max) = %.3f" % (name, ratio))
    assert ratio <= 1.0


# ---- float32 adjoint: scatter form, dense=True, and the route dense=True takes -------------------------------------------------------
@pytest.mark.parametrize("name", list(rc.CASES))
def test_adjoint_f32(dev, ref, name):
    d = ref(name, forward=False); c = d["case"]
    ops = _ops()
    boxes, dout = torch.tensor(c.rois, device=dev), torch.tensor(d["dout"], device=dev)
    maps = _prefilled(c, dev)
    ops.roialign_bwd(boxes, dout, maps, c.P, c.area)
    torch.cuda.synchronize()
    _check_adjoint("roialign bwd scatter %s" % name, maps, d["adj"])
    # the gather entry point itself: refuses (and writes nothing) where dense=True is meant to fall back, else it is the adjoint
    maps = _prefilled(c, dev)
    status = _gather_direct(c, boxes, dout, maps)
    takes = name in GATHER and name != "p33"
    assert status == (0 if takes else ops.ERR_UNSUPPORTED)
    if takes:
        _check_adjoint("roialign bwd gather %s" % name, maps, d["adj"], adds=4)
    else:
        assert all(bool((m == PREFILL).all()) for m in maps)
    if name == "p33":                                                       # P <= 32 is all that kept it out
        assert _gather_direct(c, boxes, dout, _prefilled(c, dev), P=32) == 0
    maps = _prefilled(c, dev)
    ops.roialign_bwd(boxes, dout, maps, c.P, c.area, dense=True)
    torch.cuda.synchronize()
    _check_adjoint("roialign bwd dense=True %s" % name, maps, d["adj"], adds=4 if takes else None)


def test_adjoint_dense_misaligned_dout_falls_back(dev, ref):
    """dout one float into a larger buffer: not 16-byte aligned, the gather form refuses and dense=True takes the scatter form."""
    d = ref("stage", forward=False); c = d["case"]
    ops = _ops()
    boxes = torch.tensor(c.rois, device=dev)
    buf = torch.zeros(d["dout"].size + 4, device=dev)
    dout = buf[1:1 + d["dout"].size].view(d["dout"].shape)
    dout.copy_(torch.tensor(d["dout"]))
    assert dout.is_contiguous() and dout.data_ptr() % 16 == 4
    maps = _prefilled(c, dev)
    assert _gather_direct(c, boxes, dout, maps) == ops.ERR_UNSUPPORTED
    assert all(bool((m == PREFILL).all()) for m in maps)
    ops.roialign_bwd(boxes, dout, maps, c.P, c.area, dense=True)
    torch.cuda.synchronize()
    _check_adjoint("roialign bwd dense=True stage, dout misaligned", maps, d["adj"])


# ---- 16-bit forms ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("name", ["odd", "thin", "p1", "stage"])
def test_h16_forms(dev, ref, name, dtype):
    """The maps are rounded to the 16-bit type first and the float64 statement sees the rounded values: what is left is the
    float32 interpolation (12 u corner_max) and one rounding of the result (e |ref64|, or half a subnormal step t).  The adjoint
    reads a 16-bit gradient scaled by the loss scale 64 and multiplies by 1/64 (exact), one more rounding per term than the
    float32 form allows for: n + 7."""
    d = ref(name, forward=False); c = d["case"]
    ops = _ops()
    e, t = (2.0 ** -11, 2.0 ** -25) if dtype == torch.float16 else (2.0 ** -8, 0.0)
    fm16 = [torch.tensor(f).to(dtype) for f in d["fms"]]
    out64, cmax, _ = rc.roialign_ref64(c.rois, [f.double().numpy() for f in fm16], c.P, c.area)
    boxes = torch.tensor(c.rois, device=dev)
    got = ops.roialign_h16(boxes, [f.to(dev) for f in fm16], c.P, c.area)
    torch.cuda.synchronize()
    assert got.dtype == dtype and tuple(got.shape) == out64.shape
    got = got.cpu().double().numpy()
    assert (got[cmax == 0] == 0).all()
    ratio = rc.worst_ratio(np.abs(got - out64), e * np.abs(out64) + rc.fwd_bound(cmax) + np.where(cmax > 0, t, 0.0)[..., None])
    print("[roialign fwd %s %s] max |err| / (e |ref| + 12 u corner_max + t) = %.3f" % (name, dtype, ratio))
    assert ratio <= 1.0
    S = 64.0
    dout16 = (torch.tensor(d["dout"]) * S).to(dtype)
    dout16[0, 1] = 0                                                        # an all-zero ROI row: adds nothing, counts for nothing
    adj = rc.roialign_adj64(c.rois, dout16.double().numpy() / S, c.shapes, c.P, c.area)
    maps = _prefilled(c, dev)
    ops.roialign_bwd_h16(boxes, dout16.to(dev), maps, c.P, c.area, multiplier=1.0 / S)
    torch.cuda.synchronize()
    _check_adjoint("roialign bwd %s %s" % (name, dtype), maps, adj, extra=7)


# ---- the partly filled last workgroup writes nothing past the end --------------------------------------------------------------------
def test_ragged_last_workgroup_stays_inside(dev, ref):
    """odd has 259 rows of bins: the last workgroup holds three, its fourth wave must leave.  Boxes, outputs and gradients are views
    into larger buffers whose tails hold a usable box, a sentinel and a large gradient: a wave that ran on would leave a trace."""
    d = ref("odd", forward=False); c = d["case"]
    ops, hip = _ops(), _hip()
    B, R = c.rois.shape[:2]
    nbin, tail = B * R * c.P * c.P * c.C, 4 * c.P * c.C                       # four more rows of bins
    boxbuf = torch.tensor(np.concatenate([c.rois.reshape(-1, 4), np.tile(np.float32([0.1, 0.1, 0.3, 0.3]), (4, 1))]), device=dev)
    boxes = boxbuf[:B * R].view(B, R, 4)
    fms = [torch.tensor(f, device=dev) for f in d["fms"]]
    desc = ops._roi_desc(boxes, fms, c.P, c.area)
    for dtype in (torch.float32, torch.float16, torch.bfloat16):
        # forward
        outbuf = torch.full((nbin + tail,), -7.0, dtype=dtype, device=dev)
        f = [m.to(dtype) for m in fms]
        if dtype == torch.float32:
            status = hip.lib().mrcnn_roialign_fwd(C.byref(desc), hip.ptr(boxes), *[hip.ptr(m) for m in f], hip.ptr(outbuf), None,
                                                  hip.current_stream())
        else:
            status = hip.lib().mrcnn_roialign_fwd_h16(C.byref(desc), ops._H16[dtype], hip.ptr(boxes), *[hip.ptr(m) for m in f],
                                                      hip.ptr(outbuf), hip.current_stream())
        torch.cuda.synchronize()
        assert status == 0
        assert bool((outbuf[nbin:] == -7.0).all()), dtype
        assert bool((outbuf[nbin - c.P * c.C:nbin] != -7.0).all())                 # the last real row was written
        # adjoint
        S = 1.0 if dtype == torch.float32 else 64.0
        gbuf = torch.full((nbin + tail,), 1000.0, dtype=dtype, device=dev)
        dout16 = (torch.tensor(d["dout"]) * S).to(dtype)
        gbuf[:nbin] = dout16.reshape(-1).to(dev)
        dout = gbuf[:nbin].view(d["dout"].shape)
        maps = _prefilled(c, dev)
        if dtype == torch.float32:
            ops.roialign_bwd(boxes, dout, maps, c.P, c.area)
            adj, extra = d["adj"], 6
        else:
            ops.roialign_bwd_h16(boxes, dout, maps, c.P, c.area, multiplier=1.0 / S)
            adj, extra = rc.roialign_adj64(c.rois, dout16.double().numpy() / S, c.shapes, c.P, c.area), 7
        torch.cuda.synchronize()
        _check_adjoint("roialign bwd odd %s, guarded buffers" % dtype, maps, adj, extra=extra)


# ---- arguments -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["C=6", "P=0", "W=0"])
def test_arguments_rejected(dev, what):
    """C % 4 != 0, P = 0 and a level without columns: every entry point raises HipPathError and launches nothing (the maps of
    the adjoints keep their pre-fill, the forward outputs their sentinel)."""
    ops, hip = _ops(), _hip()
    B, R = 1, 3
    C_ = 6 if what == "C=6" else 8
    P = 0 if what == "P=0" else 2
    shapes = [(8, 8), (4, 4), (2, 0) if what == "W=0" else (2, 2), (1, 1)]
    boxes = torch.tensor(rc._random_rois(np.random.default_rng(3), B, R), device=dev)
    fms = [torch.ones(B, H, W, C_, device=dev) for H, W in shapes]
    maps = [torch.full((B, H, W, C_), PREFILL, device=dev) for H, W in shapes]
    dout = torch.ones(B, R, P, P, C_, device=dev)
    calls = [lambda: ops.roialign(boxes, fms, P, rc.AREA),
             lambda: ops.roialign_bwd(boxes, dout, maps, P, rc.AREA),
             lambda: ops.roialign_bwd(boxes, dout, maps, P, rc.AREA, dense=True)]
    for dtype in (torch.float16, torch.bfloat16):
        calls += [lambda dtype=dtype: ops.roialign_h16(boxes, [f.to(dtype) for f in fms], P, rc.AREA),
                  lambda dtype=dtype: ops.roialign_bwd_h16(boxes, dout.to(dtype), maps, P, rc.AREA)]
    for call in calls:
        with pytest.raises(hip.HipPathError):
            call()
    # the C entry points with an output that can be looked at
    d = ops._roi_desc(boxes, fms, P, rc.AREA)
    out = torch.full((B * R * 4 * 8,), -7.0, device=dev)
    out16 = out.to(torch.float16)
    f16 = [f.to(torch.float16) for f in fms]
    st = [hip.lib().mrcnn_roialign_fwd(C.byref(d), hip.ptr(boxes), *[hip.ptr(f) for f in fms], hip.ptr(out), None, hip.current_stream()),
          hip.lib().mrcnn_roialign_fwd_h16(C.byref(d), 0, hip.ptr(boxes), *[hip.ptr(f) for f in f16], hip.ptr(out16), hip.current_stream()),
          hip.lib().mrcnn_roialign_bwd_gather(C.byref(d), hip.ptr(boxes), hip.ptr(dout), *[hip.ptr(m) for m in maps], hip.current_stream())]
    torch.cuda.synchronize()
    assert st == [-1, -1, -1]                                               # MRCNN_ERR_ARG, not a refusal that falls back
    assert bool((out == -7.0).all()) and bool((out16 == -7.0).all())
    assert all(bool((m == PREFILL).all()) for m in maps)
