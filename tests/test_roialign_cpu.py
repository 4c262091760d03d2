"""Host-side checks of tests/roialign_cases.py: the float64 statement of RoIAlign against the CPU oracle, and the properties of
the seeded cases that tests/test_roialign_gpu.py relies on (levels reached, share of outside bins, gather rounds with fractional
weights).  Without them a GPU test could pass vacuously."""
import numpy as np
import pytest
import torch

import mrcnn_oracle as orc
import roialign_cases as rc

NAMES = list(rc.CASES)


@pytest.fixture(scope="module")
def ref():
    """Per case, computed once and left unchanged: the case, its maps and gradient, the float64 forward and adjoint."""
    cache = {}

    def get(name):
        if name not in cache:
            c = rc.CASES[name]()
            fms, dout = rc.case_maps(name), rc.case_dout(name)
            cache[name] = dict(case=c, fms=fms, dout=dout, fwd=rc.roialign_ref64(c.rois, fms, c.P, c.area),
                               adj=rc.roialign_adj64(c.rois, dout, c.shapes, c.P, c.area))
        return cache[name]
    return get


def _oracle_autograd(c, fms, dout, dtype):
    """orc.crop_and_resize per level on maps of `dtype` (coordinates and fractions stay float32), gradient of <out, dout>."""
    t = [torch.tensor(f, dtype=dtype, requires_grad=True) for f in fms]
    lv = orc.roi_levels(c.rois, c.area)
    loss = 0
    for i, f in enumerate(t):
        ix = torch.nonzero(lv == i + 2)
        if ix.shape[0]:
            pooled = orc.crop_and_resize(f, torch.tensor(c.rois)[ix[:, 0], ix[:, 1]], ix[:, 0], c.P, c.P)
            loss = loss + (pooled * torch.tensor(dout, dtype=dtype)[ix[:, 0], ix[:, 1]]).sum()
    loss.backward()
    return [(f.grad if f.grad is not None else torch.zeros_like(f)).numpy().astype(np.float64) for f in t]


@pytest.mark.parametrize("name", NAMES)
def test_oracle_forward_within_bound(ref, name):
    d = ref(name); c = d["case"]
    out, cmax, levels = d["fwd"]
    got = orc.pyramid_roi_align(c.rois, [torch.tensor(f) for f in d["fms"]], c.P, c.area).numpy().astype(np.float64)
    assert (got[cmax == 0] == 0).all() and (out[cmax == 0] == 0).all()
    ratio = rc.worst_ratio(np.abs(got - out), rc.fwd_bound(cmax) * np.ones_like(out))
    print("[roialign oracle fwd %s] max |err| / (12 u corner_max) = %.3f" % (name, ratio))
    assert ratio <= 1.0


@pytest.mark.parametrize("dtype,unit", [(torch.float32, 2.0 ** -24), (torch.float64, 2.0 ** -53)], ids=["f32", "f64"])
@pytest.mark.parametrize("name", NAMES)
def test_oracle_autograd_within_adjoint_bound(ref, name, dtype, unit):
    """The oracle's gradient against roialign_adj64 within (n + 6) unit abs_sum: on float32 maps, and on float64 maps (same float32
    coordinates), where the two differ by float64 rounding only -- that pins the statement to 2^-53.
    The bound needs every term accurate relative to |g * w|, i.e. the weights multiplied, as the kernels and TF's
    CropAndResizeBackpropImage do.  torch's chain rule through the forward's t + (b - t) * yl forms a term as
    (g - g * yl) - (g - g * yl) * xl instead, accurate relative to |g| only: with it this check missed by up to 22 times on `odd`
    (P3 pixel (5, 19): one bin through a corner of weight 3e-3, error 0.5 u |g|), 13.7 on p1, 10.5 on p2.  orc.crop_and_resize now
    carries TF's backward."""
    d = ref(name)
    got = _oracle_autograd(d["case"], d["fms"], d["dout"], dtype)
    ratio = 0.0
    for g, m in zip(got, d["adj"]):
        assert (g[m["n"] == 0] == 0).all()
        ratio = max(ratio, rc.worst_ratio(np.abs(g - m["sum"]), rc.adj_bound(m) * (unit / rc.U)))
    print("[roialign oracle adjoint %s %s] max |err| / ((n + 6) u abs_sum) = %.3f" % (name, dtype, ratio))
    assert ratio <= 1.0


@pytest.mark.parametrize("crop", [1, 3])
def test_oracle_crop_and_resize_backward_is_its_adjoint(crop):
    """orc.crop_and_resize has a hand-written backward (TF's): finite differences of its forward must agree with it, on boxes that
    are inside, partly outside, wholly outside, reversed and empty, two of them on the same image."""
    image = torch.tensor(np.random.default_rng(5).standard_normal((2, 5, 7, 3)), requires_grad=True)
    boxes = np.float32([[0.1, 0.2, 0.8, 0.9], [-0.3, 0.1, 0.6, 1.2], [1.2, 1.2, 1.6, 1.6], [0.7, 0.6, 0.3, 0.1], [0.5, 0.5, 0.5, 0.5],
                        [0.15, 0.25, 0.7, 0.8]])
    idx = [0, 1, 1, 0, 1, 0]
    assert torch.autograd.gradcheck(lambda im: orc.crop_and_resize(im, boxes, idx, crop, crop), (image,), eps=1e-6, atol=1e-9)


@pytest.mark.parametrize("name,prefill", [("odd", 0.25), ("odd", 0.0), ("p1", 0.25), ("p2", 0.25)])
def test_scatter_order_emulation(ref, name, prefill):
    """The scatter kernel's arithmetic replayed in float32 on the host (ROI, py, px order; weights (1 - yl) * (1 - xl) ... formed
    first, zero weights skipped, one float32 addition into the map per term) stays inside adj_bound.  With 2 u prefill in place of
    n u prefill it does not: odd, prefill 0.25, reaches 1.22."""
    d = ref(name); c = d["case"]
    levels, ((vy, top, bot, yl), (vx, lef, rig, xl)) = rc._samples(c.rois, c.shapes, c.P, c.area)
    maps = [np.full((c.rois.shape[0], H, W, c.C), prefill, np.float32) for H, W in c.shapes]
    one = np.float32(1)
    for b, r, py, px in np.ndindex(c.rois.shape[0], c.rois.shape[1], c.P, c.P):
        if not (vy[b, r, py] and vx[b, r, px]):
            continue
        m, g = maps[levels[b, r] - 2], d["dout"][b, r, py, px]
        y, x = yl[b, r, py], xl[b, r, px]
        for yy, wy in ((top[b, r, py], one - y), (bot[b, r, py], y)):
            for xx, wx in ((lef[b, r, px], one - x), (rig[b, r, px], x)):
                w = wy * wx
                assert w.dtype == np.float32
                if w != 0:
                    m[b, yy, xx] += g * w
    worst = 0.0
    for a, m in zip(maps, d["adj"]):
        assert (a[m["n"] == 0] == np.float32(prefill)).all()
        worst = max(worst, rc.worst_ratio(np.abs(a.astype(np.float64) - prefill - m["sum"]), rc.adj_bound(m, prefill=prefill)))
    print("[roialign scatter emulation %s prefill %g] max |err| / bound = %.3f" % (name, prefill, worst))
    assert worst <= 1.0


def test_levels_and_special_rows(ref):
    for name in ("odd", "thin"):
        levels = ref(name)["fwd"][2]
        assert np.bincount(levels.ravel(), minlength=6)[2:].min() >= 3, name
    d = ref("odd")
    out, cmax, levels = d["fwd"]
    assert levels[0, :12].tolist() == rc.ODD_LEVELS_0_11
    assert levels[0, [rc.ODD_ZERO_AREA, rc.ODD_INVERTED]].tolist() == [2, 2]
    assert (cmax[0, rc.ODD_OUTSIDE] == 0).all()
    assert cmax[0, rc.ODD_WHOLE_MAP, -1, -1] > 0 and (cmax[0, rc.ODD_WHOLE_MAP] > 0).all()
    assert (cmax[0, rc.ODD_INVERTED] > 0).all() and (cmax[0, rc.ODD_REVERSED] > 0).all()       # reversed boxes sample, downwards
    assert (cmax[0, rc.ODD_STARTS_OUTSIDE, 0] == 0).all() and cmax[0, rc.ODD_STARTS_OUTSIDE, -1, -1] > 0
    assert np.isfinite(d["case"].rois).all()
    # nothing is added in the adjoint by the wholly-outside row: without it every pixel keeps its count
    c = d["case"]
    dout = d["dout"].copy(); dout[0, rc.ODD_OUTSIDE] = 0
    for m, m0 in zip(d["adj"], rc.roialign_adj64(c.rois, dout, c.shapes, c.P, c.area)):
        assert np.array_equal(m["n"], m0["n"]) and np.array_equal(m["sum"], m0["sum"])
    # the P5 map of `thin` has H - 1 = 0: every sample row is row 0 with fraction 0
    t = ref("thin")
    lv, ((vy, top, bot, yl), _) = rc._samples(t["case"].rois, t["case"].shapes, t["case"].P, t["case"].area)
    assert vy[lv == 5].all() and (top[lv == 5] == 0).all() and (bot[lv == 5] == 0).all() and (yl[lv == 5] == 0).all()


@pytest.mark.parametrize("name", NAMES)
def test_outside_bins_are_few(ref, name):
    """A cap, so that zeros cannot carry a test (odd: 4.3 % with its hand-set boxes)."""
    cmax = ref(name)["fwd"][1]
    assert np.isfinite(ref(name)["case"].rois).all()
    assert (cmax == 0).mean() <= 0.10


def test_shapes_reach_the_paths():
    c = {n: f() for n, f in rc.CASES.items()}
    rows = {n: v.rois.shape[0] * v.rois.shape[1] * v.P for n, v in c.items()}
    assert rows["odd"] == 259 and rows["thin"] == 210 and rows["odd"] % 4 and rows["thin"] % 4         # ragged last workgroup
    assert c["odd"].C < 64 and c["thin"].C // 4 == 65                                                  # c += 64 loops
    assert all(h != w for n in ("odd", "thin", "rect") for h, w in c[n].shapes)
    assert c["thin"].shapes[3][0] == 1
    assert c["p1"].P == 1 and c["p2"].P == 2 and c["p33"].P == 33 and c["wrap"].rois.shape[1] > 256
    assert all(c[n].C == 256 for n in ("p33", "stage", "wrap", "rect")) and all(c[n].C != 256 for n in ("odd", "thin", "p1", "p2"))


def test_gather_staging_rounds():
    s = rc.stage()
    e, f = rc.gather_staging(s.rois, s.shapes, s.P, s.area)[0]
    assert ((e > 512) & (f > 256)).any()
    w = rc.wrap()
    e, f = rc.gather_staging(w.rois, w.shapes, w.P, w.area)[0]
    assert e.shape[1] == 5 and ((e[:, 4] > 512) & (f[:, 4] > 256)).any()        # block 4 = ROIs 256-299: second trip of part 0
    # what the new cases are for: on the inputs of test_kernels_gpu.py::test_roialign_fwd_bwd[14] no entry with a fractional
    # weight takes part in a pixel that needs a second round (only the zero-padded ROIs at pixel (0, 0) of P2 do)
    rois, shapes, P, area = rc.kernel_test_14_rois()
    over = 0
    for e, f in rc.gather_staging(rois, shapes, P, area):
        assert (f[e > 256] == 0).all()
        over += int((e > 256).sum())
    assert over > 0


def test_perturbed_statement_disagrees_with_oracle(ref):
    """The CPU side of "would a wrong kernel be caught": the float64 statement with the fault built in leaves the forward bound
    against the oracle."""
    # P == 1 sampled at (y1, x1) instead of the midpoint
    d = ref("p1"); c = d["case"]
    got = orc.pyramid_roi_align(c.rois, [torch.tensor(f) for f in d["fms"]], c.P, c.area).numpy().astype(np.float64)
    corner = c.rois.copy(); corner[..., 2:] = corner[..., :2]                 # 0.5 * (y1 + y1) == y1 exactly
    out, cmax, _ = rc.roialign_ref64(corner, d["fms"], c.P, c.area, levels=d["fwd"][2])
    assert (np.abs(got - out) > rc.fwd_bound(np.maximum(cmax, d["fwd"][1]))).any(-1).mean() > 0.9
    # level rounding: truncation, floor, ceil and an offset of one all move some of rows 4-9 of `odd` (2 % either side of the
    # half-way sizes) to another level, and with it to another map
    d = ref("odd"); c = d["case"]
    got = orc.pyramid_roi_align(c.rois, [torch.tensor(f) for f in d["fms"]], c.P, c.area).numpy().astype(np.float64)
    h = c.rois[..., 2] - c.rois[..., 0]; w = c.rois[..., 3] - c.rois[..., 1]
    with np.errstate(all="ignore"):
        v = np.log(np.sqrt(h * w) / (np.float32(224.0) / np.sqrt(np.float32(c.area)))) / np.log(np.float32(2.0))
    v = np.where(np.isfinite(v), v, -1e9)
    assert np.array_equal(np.clip(4 + np.rint(v), 2, 5).astype(np.int64), d["fwd"][2])
    for wrong in (np.trunc, np.floor, np.ceil, lambda t: np.rint(t) + 1, lambda t: np.rint(t) - 1):
        levels = np.clip(4 + wrong(v), 2, 5).astype(np.int64)
        assert (levels[0, 4:10] != d["fwd"][2][0, 4:10]).any()
        out, cmax, _ = rc.roialign_ref64(c.rois, d["fms"], c.P, c.area, levels=levels)
        assert (np.abs(got - out) > rc.fwd_bound(np.maximum(cmax, d["fwd"][1]))).any()
    # (round-half-away differs from round-half-even only where the float32 log2 is exactly k + 0.5; no box can be placed there
    # without depending on the last bit of logf, so that mutation is outside what these cases can see)
