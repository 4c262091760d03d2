"""Hand-built sources for the source-parameter step of the tiled source finder (SFinder.compute_source_params): the image, the
headers and the sources of tests/golden/sfinder_params.npz, the codec of that fixture, a recording stand-in for the WCS, and a
float64 brute force of what ops.source_params returns.  Not a test module: imported by test_sfinder_params_cpu.py,
test_sfinder_params_gpu.py and the fixture generator tests/golden/make_sfinder_params_fixtures.py."""
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden", "sfinder_params.npz")
NX, NY = 96, 80
BEAM_CARDS = {"CDELT1": -0.0005, "CDELT2": 0.0005, "BMAJ": 0.004, "BMIN": 0.003, "BPA": 12.5}
FLOAT_KEYS = ("X0", "Y0", "X0w", "Y0w", "X0_wcs", "Y0_wcs", "X0w_wcs", "Y0w_wcs", "Xmin_wcs", "Xmax_wcs", "Ymin_wcs", "Ymax_wcs",
              "Smin", "Smax", "Smean", "Smedian", "Sstddev", "flux")
INT_KEYS = ("nPix", "Xmin", "Xmax", "Ymin", "Ymax")
SENTINEL = (-1.0, -2.0, -3.0)           # what the generator's sigma_clipped_stats stand-in returns


class RecorderWCS(object):
    """Stand-in for astropy.wcs.WCS in the generator and in the fixture test: records what it is asked and answers with a fixed
    affine map, so the fixture pins which pixel coordinates reach all_pix2world and where its answers go -- not a projection."""
    valid, why = True, ""

    def __init__(self, header=None):
        self.naxis = int((header or {}).get("NAXIS", 2))
        self.calls = []

    def all_pix2world(self, points, origin):
        self.calls.append(([list(p) for p in points], origin))
        return [[1000.0 + 2.0 * p[0], 2000.0 - 3.0 * p[1]] + [0.0] * (len(p) - 2) for p in points]


def ellipse(cy, cx, a, b):
    yy, xx = np.mgrid[0:NY, 0:NX]
    return np.argwhere(((xx - cx) / a) ** 2 + ((yy - cy) / b) ** 2 <= 1.0)


def rect(y0, y1, x0, x1):
    yy, xx = np.mgrid[y0:y1 + 1, x0:x1 + 1]
    return np.stack([yy.ravel(), xx.ravel()], axis=1)


def source(name, pixels, merged):
    """A catalogue entry as Analyzer.make_json_results (x2 / y2 exclusive) or SFinder._merged_source (inclusive) boxes it."""
    p = np.asarray(pixels, np.int64)
    (y1, x1), (y2, x2) = p.min(axis=0), p.max(axis=0)
    e = 0 if merged else 1
    return {"name": name, "x1": int(x1), "x2": int(x2) + e, "y1": int(y1), "y2": int(y2) + e, "merged": bool(merged), "edge": bool(merged),
            "pixels": p.tolist()}


def make_image():
    """96 x 80 float32: seeded noise plus blobs under the sources; NaN at (35, 30) -- in the halo of `nan_halo`, whose mask is
    columns 34 .. 40 -- and at (52, 70) and (53, 71) inside the mask of `nan_mask`."""
    rng = np.random.RandomState(20240611)
    yy, xx = np.mgrid[0:NY, 0:NX]
    img = rng.normal(0.0, 0.02, (NY, NX))
    for cy, cx, amp in ((20, 20, 1.0), (35, 37, 0.5), (52, 70, 0.8), (60, 30, 2.0), (5, 50, 0.7), (40, 2, 0.6), (40, 93, 0.9), (76, 50, 0.4)):
        img += amp * np.exp(-0.5 * (((yy - cy) / 3.0) ** 2 + ((xx - cx) / 4.0) ** 2))
    img = img.astype(np.float32)
    img[35, 30] = np.nan
    img[52, 70] = np.nan
    img[53, 71] = np.nan
    return img


def make_sources():
    return [
        source("interior", ellipse(20, 20, 6, 4), False),
        source("left", rect(36, 44, 0, 4), False),                       # x1 == 0: offset clamps to 0
        source("top", rect(0, 3, 44, 56), False),                        # y1 == 0
        source("right_excl", rect(38, 42, 90, 94), False),               # exclusive x2 == nx - 1: offset 0
        source("bottom_incl", rect(74, 79, 45, 55), True),               # inclusive y2 == ny - 1: offset 0
        source("wrap", rect(37, 43, 91, 95), False),                     # exclusive x2 == nx: offset -1, the first column wraps
        source("merged", ellipse(60, 30, 7, 5), True),
        source("one_pixel", [[12, 70]], False),
        source("nan_halo", rect(33, 38, 34, 40), False),
        source("nan_mask", ellipse(52, 70, 5, 3), False),
        source("near_border", rect(6, 9, 3, 7), False),                  # offsets 3 (x) and 6 (y)
    ]


def headers():
    return {"beam": dict(BEAM_CARDS, BUNIT="JY/BEAM"), "nobeam": {"BUNIT": "JY/BEAM"}}


# ---- fixture codec --------------------------------------------------------------------------------------------------
def encode(img, srcs, results, beams):
    """results: {header name: [params dict or None per source]}; beams: {header name: beamArea}."""
    out = {"image": img, "headers": np.array(json.dumps(headers())), "names": np.array([s["name"] for s in srcs], dtype="U16"),
           "boxes": np.array([(s["x1"], s["x2"], s["y1"], s["y2"], s["merged"]) for s in srcs], np.int32),
           "pix_offsets": np.concatenate([[0], np.cumsum([len(s["pixels"]) for s in srcs])]).astype(np.int64),
           "pixels": np.array([p for s in srcs for p in s["pixels"]], np.int16).reshape(-1, 2)}
    for hname, res in results.items():
        out[hname + "__beamArea"] = np.array(beams[hname], np.float64)
        out[hname + "__ints"] = np.array([[int(r[k]) for k in INT_KEYS] for r in res], np.int64)
        out[hname + "__S"] = np.array([r["S"] for r in res], np.float32)
        out[hname + "__floats"] = np.array([[float(r[k]) for k in FLOAT_KEYS] for r in res], np.float64)
    return out


def decode(z):
    po, pix = z["pix_offsets"], z["pixels"].astype(np.int64)
    srcs = []
    for s, (x1, x2, y1, y2, merged) in enumerate(z["boxes"].tolist()):
        srcs.append({"name": str(z["names"][s]), "x1": x1, "x2": x2, "y1": y1, "y2": y2, "merged": bool(merged), "edge": bool(merged),
                     "pixels": pix[po[s]:po[s + 1]].tolist()})
    want = {}
    for hname in json.loads(str(z["headers"])):
        rows = []
        for s in range(len(srcs)):
            r = {k: int(v) for k, v in zip(INT_KEYS, z[hname + "__ints"][s])}
            r.update({k: float(v) for k, v in zip(FLOAT_KEYS, z[hname + "__floats"][s])})
            r["S"] = z[hname + "__S"][s]
            rows.append(r)
        want[hname] = (float(z[hname + "__beamArea"]), rows)
    return z["image"], json.loads(str(z["headers"])), srcs, want


def write_image(path, img, cards):
    from caesar_mrcnn_amd import fits
    fits.write_fits(path, img, cards)


# ---- float64 brute force of mrcnn_source_params -----------------------------------------------------------------------
def brute_record(img, pixels, cutout, sigma=3.0, maxiters=5):
    """One record of include/mrcnn_hip.h (mrcnn_source_record) as a dict, from the definition: img [H, W] float32, pixels [y, x]
    rows (duplicates count once, pixels outside the clipped cut-out are ignored), cutout (cx0, cy0, cx1, cy1).  Sums by
    math.fsum; `abs_*` are the sums of the absolute terms (for the comparison bounds).  `min_margin` is the smallest relative
    distance of a kept-or-dropped value to a clipping bound over all iterations (inf when no bound was applied)."""
    img = np.asarray(img, np.float32)
    H, W = img.shape
    cx0, cy0, cx1, cy1 = (int(v) for v in cutout)
    rx0, ry0, rx1, ry1 = max(cx0, 0), max(cy0, 0), min(cx1, W), min(cy1, H)
    nan32 = np.float32(np.nan)
    cut = img[ry0:ry1, rx0:rx1] if rx1 > rx0 and ry1 > ry0 else np.zeros((0, 0), np.float32)
    good = cut[~np.isnan(cut)]
    fill = good.min() if good.size else nan32
    p = np.unique(np.asarray(pixels, np.int64).reshape(-1, 2), axis=0) if len(pixels) else np.zeros((0, 2), np.int64)
    p = p[(p[:, 1] >= rx0) & (p[:, 1] < rx1) & (p[:, 0] >= ry0) & (p[:, 0] < ry1)]
    v = img[p[:, 0], p[:, 1]].copy()
    v[np.isnan(v)] = fill
    ok = ~np.isnan(v)
    lx, ly = (p[:, 1] - cx0).astype(np.float64), (p[:, 0] - cy0).astype(np.float64)
    v64 = v.astype(np.float64)

    def fsum(terms):
        terms = np.asarray(terms, np.float64)
        if not np.all(np.isfinite(terms)):
            with np.errstate(all="ignore"):
                return float(np.sum(terms))                              # IEEE: inf, or NaN for NaN terms / inf - inf
        return math.fsum(terms.tolist())

    with np.errstate(all="ignore"):
        tx, ty = lx * v64, ly * v64
    rec = {"fill": fill, "n_mask": int(p.shape[0]), "npix": int(ok.sum()),
           "smin": v[ok].min() if ok.any() else nan32, "smax": v[ok].max() if ok.any() else nan32,
           "s64": fsum(v64[ok]), "abs_s64": fsum(np.abs(v64[ok])),
           "m00": int(p.shape[0]), "m10": int((p[:, 1] - cx0).sum()), "m01": int((p[:, 0] - cy0).sum()),
           "w00": fsum(v64), "w10": fsum(tx), "w01": fsum(ty),
           "abs_w00": fsum(np.abs(v64)), "abs_w10": fsum(np.abs(tx)), "abs_w01": fsum(np.abs(ty))}
    # the clipping loop, every sum by fsum
    x = np.sort(v64[np.isfinite(v64)])
    iters, min_margin = 0, float("inf")

    def stats(x):
        k = x.size
        med = float(x[k // 2]) if k & 1 else (float(x[k // 2 - 1]) + float(x[k // 2])) / 2.0
        mean = math.fsum(x.tolist()) / k
        sd = math.sqrt(math.fsum(((x - mean) ** 2).tolist()) / k)
        return mean, med, sd

    while iters < maxiters and x.size:
        mean, med, sd = stats(x)
        lo, hi = med - sigma * sd, med + sigma * sd
        for b in (lo, hi):
            # (all kept values equal: their sum is exact in float64, the mean is the value, every deviation and the std are
            # exactly 0 in any summation order -- both bounds ARE the value, bit for bit, and nothing is left to rounding)
            if x.size and math.isfinite(b) and x[0] != x[-1]:
                dist = np.abs(x - b) / max(abs(b), np.finfo(np.float64).tiny)
                min_margin = min(min_margin, float(dist.min()))
        keep = (x >= lo) & (x <= hi)
        iters += 1
        removed = x.size - int(keep.sum())
        x = x[keep]
        if not removed:
            break
    if x.size:
        mean, med, sd = stats(x)
    else:
        mean = med = sd = float("nan")
    rec.update({"clip_mean": mean, "clip_median": med, "clip_std": sd, "clip_kept": int(x.size), "clip_iters": iters,
                "min_margin": min_margin, "clip_abs": math.fsum(np.abs(x).tolist()) if x.size else 0.0})
    return rec


def numpy_source_params(img, pixel_lists, cutouts, sigma=3.0, maxiters=5):
    """The records of ops.source_params as a NumPy structured array, from brute_record: the CPU stand-in of the launch."""
    from caesar_mrcnn_amd import ops
    dt = ops.source_record_dtype()
    out = np.zeros(len(pixel_lists), dt)
    for i, (p, c) in enumerate(zip(pixel_lists, cutouts)):
        r = brute_record(img, p, c, sigma, maxiters)
        for k in dt.names:
            out[k][i] = r["n_mask"] if k == "n_gathered" else r[k]
    return out


# ---- comparing two parameter dicts of one source ---------------------------------------------------------------------
U64, U32 = 2.0 ** -53, 2.0 ** -24
EXACT_KEYS = ("nPix", "Xmin", "Xmax", "Ymin", "Ymax", "Xmin_wcs", "Xmax_wcs", "Ymin_wcs", "Ymax_wcs", "Smin", "Smax", "Smedian",
              "X0", "Y0", "X0_wcs", "Y0_wcs")


def _same(a, b):
    return a == b or (a != a and b != b)


def assert_params_close(got, want, rec, beam_area=0.0, wcs_slope=(0.0, 0.0)):
    """`got` and `want` are two parameter dicts of ONE source, computed by different summation orders (the device path and the
    host statement); `rec` = brute_record of that source (the exact sums and the sums of absolute terms).  The bounds:

      exact keys   integers, min / max, the median (a value or the mean of two float32 values: exact in float64), and X0 / Y0
                   (ratios of equal integers) with their sky positions are equal;
      S            float32 recursive summation of n terms errs by at most (n - 1) 2^-24 sum|x| in any order, rounding a float64
                   sum to float32 by 2^-24 |S| <= 2^-24 sum|x|: together n 2^-24 sum|x|;  flux = S / beamArea the same, scaled;
      X0w, Y0w     r = a / b + offset with |da| <= 2 n 2^-53 sum|x I| and |db| <= 2 n 2^-53 sum|I| between two summation orders
                   (n 2^-53 sum|term| each against the exact sum): |dr| <= (|da| + |r - offset| |db|) / |b| to first order -- taken
                   with a factor 1.01 for the second order plus 4 ulp of the result for the division and the addition;
      *w_wcs       that bound times the slope of the (affine) stand-in WCS, plus 4 ulp;
      Smean        sum / k: 2 k 2^-53 sum|x| / k = 2 * 2^-53 sum|x| over the kept values, plus 2 ulp;
      Sstddev      two-pass formula, k kept values: each term (x - m)^2 carries <= 3 * 2^-53 relative (one subtraction, one product;
                   the error of the computed mean enters only in second order, because d/dm sum (x - m)^2 = 0 at the mean -- as
                   long as |mean| / std * k * 2^-53 << 1, asserted), the sum of k non-negative terms (k - 1) 2^-53, the division
                   2^-53; the square root halves the total and adds 2^-53: (k + 5) / 2 * 2^-53 <= 4 k 2^-53 relative per computed value,
                   8 k 2^-53 between two of them (c = 8)."""
    assert set(got) == set(want)
    for k in EXACT_KEYS:
        assert _same(got[k], want[k]), (k, got[k], want[k])
    n = max(rec["n_mask"], 1)
    bS = n * U32 * rec["abs_s64"]
    assert abs(got["S"] - want["S"]) <= bS, ("S", got["S"], want["S"], bS)
    scale = 1.0 / beam_area if beam_area > 0 else 1.0
    assert abs(got["flux"] - want["flux"]) <= bS * scale * (1 + 4 * U64) + 4 * U64 * abs(want["flux"]), ("flux", got["flux"], want["flux"])
    b0 = 2 * n * U64 * rec["abs_w00"]
    for key, num, a, off, slope in (("X0w", "w10", "abs_w10", got["X0"] - rec["m10"] / max(rec["m00"], 1), wcs_slope[0]),
                                    ("Y0w", "w01", "abs_w01", got["Y0"] - rec["m01"] / max(rec["m00"], 1), wcs_slope[1])):
        if rec["w00"] == 0 or not math.isfinite(rec["w00"]) or not math.isfinite(rec[num]):
            assert _same(got[key], want[key]), (key, got[key], want[key])
            assert _same(got[key + "_wcs"], want[key + "_wcs"])
            continue
        r = rec[num] / rec["w00"]
        bound = 1.01 * (2 * n * U64 * rec[a] + abs(r) * b0) / abs(rec["w00"]) + 4 * U64 * max(abs(r), abs(r + off), abs(off))
        assert abs(got[key] - want[key]) <= bound, (key, got[key], want[key], bound)
        bw = abs(slope) * bound + 4 * U64 * max(abs(got[key + "_wcs"]), 1.0)
        assert abs(got[key + "_wcs"] - want[key + "_wcs"]) <= bw, (key + "_wcs", got[key + "_wcs"], want[key + "_wcs"], bw)
    k = rec["clip_kept"]
    if k == 0:
        assert _same(got["Smean"], want["Smean"]) and _same(got["Sstddev"], want["Sstddev"])
        return
    bm = 2 * U64 * rec["clip_abs"] + 2 * U64 * abs(rec["clip_mean"])
    assert abs(got["Smean"] - want["Smean"]) <= bm, ("Smean", got["Smean"], want["Smean"], bm)
    if rec["clip_std"] > 0:
        assert abs(rec["clip_mean"]) / rec["clip_std"] * k * U64 < 1e-6
    bs = 8 * k * U64 * rec["clip_std"]
    assert abs(got["Sstddev"] - want["Sstddev"]) <= bs, ("Sstddev", got["Sstddev"], want["Sstddev"], bs)
