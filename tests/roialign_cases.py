"""RoIAlign (csrc/roialign.hip) stated in float64, and the seeded boxes / shapes its tests feed it: pure NumPy + the CPU oracle,
so tests/test_roialign_cpu.py can check without a GPU that the cases reach what tests/test_roialign_gpu.py relies on.

The sample coordinates are float32 with the operands and the order of orc.crop_and_resize and of the kernels
(lo*(D-1) + k*((hi-lo)*(D-1)/(P-1)); 0.5*(lo+hi)*(D-1) for P = 1): the library is built with -ffp-contract=off, so the
inside / outside decisions and the fractions yl, xl are the same numbers on both sides.  Everything after them is float64."""
import collections

import numpy as np

import mrcnn_oracle as orc
from model_cases import _rand, _random_rois

AREA = 1024.0 ** 2      # the kernels use it only to pick the level; with it box sides of 0.01 - 0.9 reach all four levels on small maps
U = 2.0 ** -24          # unit roundoff of float32

Case = collections.namedtuple("Case", "rois shapes P C area")


# ---- float64 statement ----------------------------------------------------------------------------------------------------------
def _samples(rois, shapes, P, image_area, levels=None):
    """levels [B,R]; per axis (inside [B,R,P] bool, floor, ceil [B,R,P] int (0 where outside), fraction [B,R,P] float32)."""
    rois = np.asarray(rois, np.float32)
    if levels is None:
        levels = orc.roi_levels(rois, image_area).numpy()
    dims = np.asarray(shapes, np.int64)[levels - 2]                       # [B,R,2]
    k = np.arange(P, dtype=np.float32)
    axes = []
    for a in (0, 1):
        lo, hi = rois[..., a], rois[..., a + 2]
        d1 = (dims[..., a] - 1).astype(np.float32)
        if P > 1:
            step = (hi - lo) * d1 / np.float32(P - 1)
            s = (lo * d1)[..., None] + k * step[..., None]
        else:
            s = (np.float32(0.5) * (lo + hi) * d1)[..., None]
        assert s.dtype == np.float32
        inside = ~((s < 0) | (s > d1[..., None]))
        s0 = np.where(inside, s, np.float32(0))
        fl = np.floor(s0)
        axes.append((inside, fl.astype(np.int64), np.ceil(s0).astype(np.int64), s0 - fl))
    return levels, axes


def roialign_ref64(rois, fms, P, image_area, levels=None):
    """out [B,R,P,P,C] float64, corner_max [B,R,P,P] (largest |value| among the four corners of a bin over its channels; 0 for a
    bin that is outside), levels [B,R].  fms: NHWC arrays of P2..P5 (any float type; read as float64).  levels: taken from
    orc.roi_levels unless given (tests/test_roialign_cpu.py perturbs the statement with it)."""
    fms = [np.asarray(f, np.float64) for f in fms]
    levels, ((vy, top, bot, yl), (vx, lef, rig, xl)) = _samples(rois, [f.shape[1:3] for f in fms], P, image_area, levels)
    B, R = levels.shape
    out = np.zeros((B, R, P, P, fms[0].shape[3]))
    cmax = np.zeros((B, R, P, P))
    for li, f in enumerate(fms):
        b, r = np.nonzero(levels == li + 2)
        if b.size == 0:
            continue
        bi = b[:, None, None]
        t_, b_ = top[b, r][:, :, None], bot[b, r][:, :, None]
        l_, r_ = lef[b, r][:, None, :], rig[b, r][:, None, :]
        tl, tr, bl, br = f[bi, t_, l_], f[bi, t_, r_], f[bi, b_, l_], f[bi, b_, r_]
        y = yl[b, r].astype(np.float64)[:, :, None, None]
        x = xl[b, r].astype(np.float64)[:, None, :, None]
        val = (1 - y) * ((1 - x) * tl + x * tr) + y * ((1 - x) * bl + x * br)
        valid = vy[b, r][:, :, None] & vx[b, r][:, None, :]
        out[b, r] = np.where(valid[..., None], val, 0.0)
        m = np.maximum(np.maximum(np.abs(tl).max(-1), np.abs(tr).max(-1)), np.maximum(np.abs(bl).max(-1), np.abs(br).max(-1)))
        cmax[b, r] = np.where(valid, m, 0.0)
    return out, cmax, levels


def _adjoint_matrices(rois, shapes, P, image_area, b):
    """Image b: per level (A, N) of shape [H*W, R*P*P]: A = the summed float64 bilinear weight with which a bin reaches a pixel,
    N = how many of a bin's four corners reach it with a non-zero weight (a corner of weight 0 adds nothing in the kernels)."""
    levels, ((vy, top, bot, yl), (vx, lef, rig, xl)) = _samples(rois, shapes, P, image_area)
    R = levels.shape[1]
    mats = []
    for li, (H, W) in enumerate(shapes):
        A = np.zeros((H * W, R * P * P)); N = np.zeros((H * W, R * P * P))
        r = np.nonzero(levels[b] == li + 2)[0]
        valid = vy[b, r][:, :, None] & vx[b, r][:, None, :]
        col = (r[:, None, None] * P + np.arange(P)[None, :, None]) * P + np.arange(P)[None, None, :]
        y = yl[b, r].astype(np.float64)[:, :, None]; x = xl[b, r].astype(np.float64)[:, None, :]
        for rows, wy in ((top, 1 - y), (bot, y)):
            for cols, wx in ((lef, 1 - x), (rig, x)):
                pix = rows[b, r][:, :, None] * W + cols[b, r][:, None, :]
                w = np.where(valid, wy * wx, 0.0)
                np.add.at(A, (pix.ravel(), col.ravel()), w.ravel())
                np.add.at(N, (pix.ravel(), col.ravel()), (w != 0).ravel().astype(np.float64))
        mats.append((A, N))
    return mats


def roialign_adj64(rois, dout, shapes, P, image_area):
    """The adjoint of roialign_ref64 applied to dout [B,R,P,P,C]: per level a dict of float64 maps
    sum [B,H,W,C], abs_sum [B,H,W,C] (sum of |g * w|) and n [B,H,W] (non-zero contributions per pixel: weight non-zero and
    the bin's gradient not all zero)."""
    dout = np.asarray(dout, np.float64)
    B, C = dout.shape[0], dout.shape[-1]
    res = [dict(sum=np.zeros((B, H, W, C)), abs_sum=np.zeros((B, H, W, C)), n=np.zeros((B, H, W))) for H, W in shapes]
    for b in range(B):
        g = dout[b].reshape(-1, C)
        live = (g != 0).any(1).astype(np.float64)
        for (H, W), m, (A, N) in zip(shapes, res, _adjoint_matrices(rois, shapes, P, image_area, b)):
            m["sum"][b] = (A @ g).reshape(H, W, C)
            m["abs_sum"][b] = (A @ np.abs(g)).reshape(H, W, C)
            m["n"][b] = (N @ live).reshape(H, W)
    return res


def gather_staging(rois, shapes, P, image_area):
    """What mrcnn_roialign_bwd_gather stages: per level two int arrays [B, ceil(R/64), H, W], the number of (row, weight) entries
    of a block of 64 consecutive ROIs at a pixel, and how many of them have both fractions non-zero.  An entry is a (py, px)
    pair whose floor or ceil row is the pixel's row and likewise for the column; a coordinate counts once when floor == ceil."""
    levels, axes = _samples(rois, shapes, P, image_area)
    B, R = levels.shape
    nblk = (R + 63) // 64
    res = []
    for li, (H, W) in enumerate(shapes):
        cnt = []
        for (inside, fl, ce, frac), D in zip(axes, (H, W)):
            at = np.arange(D)[None, None, None, :]
            hit = inside[..., None] & ((fl[..., None] == at) | (ce[..., None] == at)) & (levels == li + 2)[..., None, None]
            both = np.stack([hit.sum(2), (hit & (frac != 0)[..., None]).sum(2)])         # [2,B,R,D]
            cnt.append(np.concatenate([both, np.zeros((2, B, nblk * 64 - R, D), both.dtype)], 2).reshape(2, B, nblk, 64, D))
        res.append(tuple(np.einsum("bkrh,bkrw->bkhw", cnt[0][i], cnt[1][i]) for i in (0, 1)))
    return res


# ---- bounds (elementwise) ---------------------------------------------------------------------------------------------------------
def fwd_bound(corner_max):
    """With M = corner_max: t = a + (b - a) * xl is three roundings on magnitudes <= 2M, M and M (<= 5uM), u likewise; the second
    lerp t + (u - t) * yl inherits (1 - yl) * 5uM + yl * 5uM and adds three roundings of its own (<= 5uM): 10uM, stated as 12."""
    return 12 * U * corner_max[..., None]


def adj_bound(m, extra=6, prefill=0.0, adds=None):
    """|got - prefill - sum| for a pixel's element that received n non-zero terms g * w, S = abs_sum:
      - a weight (1 - yl) * (1 - xl) is three roundings and g * w a fourth: 4uS;
      - the terms are added one by one in float32 (atomics into the map, or a register sum): n roundings on partial sums
        of magnitude <= prefill + S: n * u * S, and u * prefill for each of the additions made INTO the pre-filled element.
    adds is the number of those: None = n (the scatter forms add every term to the map), 4 for the gather form (one atomic per
    wave that shares the pixel, ROI_GATHER_SPLIT of them).  So (n + 4) u S + min(n, adds) u prefill, stated with n + `extra`.
    (First written with 2 u prefill for the pre-fill: a float32 emulation of the scatter order on `odd` reaches 1.22 times that
    bound at a pixel with n = 4 small terms, see tests/test_roialign_cpu.py::test_scatter_order_emulation; min(n, adds) is the
    term it missed, and no wider for n <= 2.)"""
    n = m["n"][..., None]
    return (n + extra) * U * m["abs_sum"] + (n if adds is None else np.minimum(n, adds)) * U * prefill


def worst_ratio(err, bound):
    """max err / bound; an element with bound 0 must have err 0."""
    assert (err[bound == 0] == 0).all(), "non-zero error where the bound is zero: %g" % err[bound == 0].max()
    return float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0


# ---- cases ----------------------------------------------------------------------------------------------------------------------
ODD_SHAPES = [(24, 40), (12, 20), (6, 10), (3, 5)]
THIN_SHAPES = [(8, 24), (4, 12), (2, 6), (1, 3)]
SQ_SHAPES = [(16, 16), (8, 8), (4, 4), (2, 2)]

ODD_LEVELS_0_11 = [2, 3, 4, 5, 2, 3, 3, 4, 4, 5, 2, 5]
ODD_ZERO_AREA, ODD_INVERTED, ODD_REVERSED, ODD_OUTSIDE, ODD_STARTS_OUTSIDE, ODD_WHOLE_MAP, ODD_ZEROS = range(12, 19)


def _square(y, x, side):
    return [y, x, y + side, x + side]


def odd():
    """Non-square maps, C below one wave, 37 * 7 = 259 rows of bins (ragged last workgroup) and the hand-set boxes."""
    rng = np.random.default_rng(11)
    rois = _random_rois(rng, 1, 37)
    k = 224.0 / 1024.0
    rows = [_square(0.05, 0.1, k * 2.0 ** (l - 4)) for l in (2, 3, 4, 5)]                                 # level centres
    # 2 % either side of each half-way size (0.029 in log2): far from any ulp difference between the device logf and the
    # host's, near enough to catch a wrong rounding mode or offset
    rows += [_square(0.01, 0.02, k * 2.0 ** (j - 1.5) * s) for j in (0, 1, 2) for s in (0.98, 1.02)]
    rows += [_square(0.3, 0.6, 0.004),                  # raw level below 2
             [0.02, 0.03, 0.97, 0.98]]                  # raw level 6
    rows += [[0.5, 0.5, 0.5, 0.5],                      # zero area away from the origin: level 2 by the -inf rule
             [0.7, 0.2, 0.3, 0.6],                      # y2 < y1: negative area, NaN, level 2, samples walk upwards
             [0.7, 0.6, 0.3, 0.1],                      # both axes reversed, positive area
             [1.2, 1.2, 1.6, 1.6],                      # wholly outside
             [-0.3, -0.2, 0.4, 0.5],                    # starts outside
             [0.0, 0.0, 1.0, 1.0],                      # the last sample is exactly H - 1, W - 1
             [0.0, 0.0, 0.0, 0.0]]
    rois[0, :len(rows)] = np.asarray(rows, np.float32)
    return Case(rois, ODD_SHAPES, 7, 8, AREA)


def thin():
    """H - 1 = 0 on P5, three images, 210 rows of bins, a ragged second channel trip (65 float4 per bin)."""
    return Case(_random_rois(np.random.default_rng(42), 3, 5), THIN_SHAPES, 14, 260, AREA)


def p1():
    return Case(_random_rois(np.random.default_rng(13), 2, 9), ODD_SHAPES, 1, 16, AREA)


def p2():
    return Case(_random_rois(np.random.default_rng(14), 2, 9), ODD_SHAPES, 2, 16, AREA)


def p33():
    """P > 32: the gather form refuses, dense=True must fall back to the scatter form."""
    return Case(_random_rois(np.random.default_rng(15), 1, 5), SQ_SHAPES, 33, 256, AREA)


def _cluster(rng, n):
    """Tiny boxes whose P x P samples fall inside one or two cells of the 16 x 16 P2 map: a few pixels collect every one of
    their bins, all with fractional weights."""
    c = np.array([0.41, 0.47]) + rng.uniform(-0.01, 0.01, (n, 2))
    h = rng.uniform(0.004, 0.03, (n, 2))
    return np.concatenate([c - h, c + h], 1).astype(np.float32)


def stage():
    """Gather rounds of ROI_GATHER_CAP = 256 entries with fractional weights: ROIs 0-11 of image 0 are a cluster."""
    rng = np.random.default_rng(7)
    rois = _random_rois(rng, 2, 70)
    rois[0, :12] = _cluster(rng, 12)
    return Case(rois, SQ_SHAPES, 14, 256, AREA)


def wrap():
    """R > 256: the second trip of part 0 (ROIs 256-299) carries the staged rounds."""
    rng = np.random.default_rng(8)
    rois = _random_rois(rng, 1, 300)
    rois[0, 256:] = _cluster(rng, 44)
    return Case(rois, SQ_SHAPES, 7, 256, AREA)


def rect():
    """The gather form (C = 256) on non-square maps: the other cases that reach it are square."""
    return Case(_random_rois(np.random.default_rng(16), 2, 20), [(12, 20), (6, 10), (3, 5), (2, 3)], 7, 256, AREA)


def p32():
    """The largest P the gather form takes: bit 31 of its sample masks is in use."""
    return Case(_random_rois(np.random.default_rng(17), 1, 5), SQ_SHAPES, 32, 256, AREA)


CASES = collections.OrderedDict((f.__name__, f) for f in (odd, thin, p1, p2, p33, stage, wrap, rect, p32))
_SEED = {n: 100 + i for i, n in enumerate(CASES)}


def case_maps(name):
    """The pyramid [P2..P5] of a case, NHWC float32."""
    c = CASES[name]()
    rng = np.random.default_rng(_SEED[name])
    return [_rand(rng, c.rois.shape[0], H, W, c.C) for H, W in c.shapes]


def case_dout(name):
    c = CASES[name]()
    rng = np.random.default_rng(_SEED[name] + 50)
    return _rand(rng, c.rois.shape[0], c.rois.shape[1], c.P, c.P, c.C)


def kernel_test_14_rois():
    """The boxes of tests/test_kernels_gpu.py::test_roialign_fwd_bwd[14] (same generator, same draws before them)."""
    rng = np.random.default_rng(14)
    B, R, C = 2, 60, 256
    for s in (64, 32, 16, 8):
        _rand(rng, B, s, s, C)
    rois = _random_rois(rng, B, R, zero_tail=3)
    rois[0, 0] = [0.2, 0.2, 1.2, 0.7]
    return rois, [(s, s) for s in (64, 32, 16, 8)], 14, AREA
