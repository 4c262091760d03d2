"""The device half of the source-parameter step: csrc/srcparams.hip (ops.source_params) against a float64 brute force,
SFinder.compute_sources_params' device path against its host statement, and the command line."""
import glob
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import sfinder_cases as mcases
import sfinder_params_cases as cases

pytestmark = pytest.mark.gpu
ROOT = cases.ROOT
N = 132                                  # image side
U = cases.U64
LADDER8 = [float(v) for v in range(-10, 11)] + [1000.0 ** j for j in range(1, 9)]       # eight rungs: more than maxiters = 5
LADDER2 = [float(v) for v in range(-10, 11)] + [1.0e3, 1.0e6]                           # two rungs: three iterations


def _first(n, y0, x0, w):
    """The first n pixels, in raster order, of the rows of width w that start at (y0, x0)."""
    k = np.arange(n)
    return np.stack([y0 + k // w, x0 + k % w], axis=1)


def _pad(p, off=10):
    """The cut-out rule of sfinder.py:1013-1016 for an inclusive pixel box: +- off, clamped at the image."""
    p = np.asarray(p)
    (y0, x0), (y1, x1) = p.min(axis=0), p.max(axis=0)
    ox, oy = min(off, N - 1 - x1, x0), min(off, N - 1 - y1, y0)
    return (x0 - ox, y0 - oy, x1 + ox + 1, y1 + oy + 1)


def _problem():
    """(image [132, 132] float32, [(name, pixels, cutout)]).  Seeded noise (mean 5, sigma 1) with planted features; every
    feature sits where no other source's mask is."""
    rng = np.random.RandomState(812)
    img = rng.normal(5.0, 1.0, (N, N)).astype(np.float32)
    src = []

    def add(name, p, cut=None):
        p = np.asarray(p, np.int64).reshape(-1, 2)
        src.append((name, p, cut if cut is not None else _pad(p)))

    # widths 1, 31, 32, 33, 64, 65 (around the 32-bit word and the 64-lane wave), heights 1 and 3
    for i, w in enumerate((1, 31, 32, 33, 64, 65)):
        for h in (1, 3):
            add("w%d_h%d" % (w, h), cases.rect(2 + 5 * i, 2 + 5 * i + h - 1, 30 + i, 30 + i + w - 1))
    # pixel counts around the wave and the workgroup: the first n pixels of rows of width 65 / 67 (257 = 3 rows of 67 + 56)
    for i, n in enumerate((1, 2, 3, 63, 64, 65)):
        add("n%d" % n, _first(n, 36 + 4 * i, 3, 65))
    for i, n in enumerate((255, 256, 257)):
        add("n%d" % n, _first(n, 60 + 5 * i, 3, 67))
    # larger than the workgroup by far: an ellipse of more than 5000 pixels (no LDS-resident path exists; every pass strides)
    yy, xx = np.mgrid[0:N, 0:N]
    big = np.argwhere(((xx - 62) / 50.0) ** 2 + ((yy - 98) / 33.0) ** 2 <= 1.0)
    assert big.shape[0] >= 5000
    add("big", big)
    # boxes at the four borders (the offset clamps to 0 there), and a corner
    add("left", cases.rect(70, 75, 0, 6))
    add("right", cases.rect(20, 24, 125, 131))
    add("top", cases.rect(0, 2, 100, 120))
    add("bottom", cases.rect(129, 131, 5, 20))
    add("corner", cases.rect(128, 131, 128, 131))
    # a cut-out the image clips on two sides (the launch takes any rectangle), and one that misses part of its mask
    add("clipped", cases.rect(1, 4, 1, 5), (-9, -9, 16, 15))
    add("mask_outside", cases.rect(60, 64, 1, 12), (4, 58, 20, 70))
    # all-equal values, halo included
    img[44:60, 100:128] = 1.5
    add("equal", cases.rect(48, 55, 104, 123))
    # NaN only in the halo: the fill changes, the statistics do not; NaN inside the mask: filled
    img[30, 112] = np.nan
    add("nan_halo", cases.rect(28, 33, 116, 121))
    img[38, 118] = img[39, 120] = np.nan
    img[37, 110] = -3.25                                                    # the cut-out's minimum, outside the mask
    add("nan_mask", cases.rect(36, 41, 116, 122))
    # +inf, and +inf with -inf, inside the mask
    img[62, 104] = np.inf
    add("pinf", cases.rect(61, 64, 102, 108))
    img[68, 121] = np.inf
    img[69, 123] = -np.inf
    add("pminf", cases.rect(67, 70, 119, 126))
    # clipping: two rungs -> three iterations; eight rungs -> the cap of five
    lad2 = _first(len(LADDER2), 100, 116, 12)                              # (right of the ellipse: not in its mask)
    img[lad2[:, 0], lad2[:, 1]] = LADDER2
    add("ladder2", lad2)
    lad8 = _first(len(LADDER8), 110, 114, 15)
    img[lad8[:, 0], lad8[:, 1]] = LADDER8
    add("ladder8", lad8)
    # the same source twice, and a source without pixels (pack_sources: an empty 1 x 1 box at the origin)
    add("twice", src[3][1], src[3][2])
    add("empty", np.zeros((0, 2), np.int64), (0, 0, 11, 11))
    return img, src


@pytest.fixture(scope="module")
def problem():
    img, src = _problem()
    brute = [cases.brute_record(img, p, c) for _, p, c in src]
    return img, src, brute


def test_problem_is_comparable(problem):
    """On the brute force alone: in every clipping iteration of every source no value lies within relative 1e-9 of a bound (a
    last-bit difference in a computed std cannot move a value across), the sizes the kernel can go wrong at are there, and the
    clipping cases do what they were built for."""
    img, src, brute = problem
    by = {s[0]: b for s, b in zip(src, brute)}
    assert all(b["min_margin"] > 1e-9 for b in brute), [(s[0], b["min_margin"]) for s, b in zip(src, brute) if not b["min_margin"] > 1e-9]
    assert {by["n%d" % n]["n_mask"] for n in (1, 2, 3, 63, 64, 65, 255, 256, 257)} == {1, 2, 3, 63, 64, 65, 255, 256, 257}
    assert by["big"]["n_mask"] >= 5000 and by["empty"]["n_mask"] == 0 and by["mask_outside"]["n_mask"] == 5 * 9
    assert by["ladder2"]["clip_iters"] == 3 and by["ladder2"]["clip_kept"] == 21
    assert by["ladder8"]["clip_iters"] == 5 and by["ladder8"]["clip_kept"] == len(LADDER8) - 5
    assert by["nan_mask"]["fill"] == np.float32(-3.25) and by["nan_mask"]["smin"] == np.float32(-3.25) and by["nan_mask"]["npix"] == 42
    assert np.isnan(img[30, 112]) and by["nan_halo"]["npix"] == by["nan_halo"]["n_mask"] == 36
    assert by["pinf"]["s64"] == math.inf and math.isnan(by["pminf"]["s64"]) and by["pinf"]["clip_kept"] <= 27
    assert by["equal"]["clip_std"] == 0.0 and by["equal"]["smin"] == by["equal"]["smax"] == np.float32(1.5)
    assert any(b["clip_kept"] & 1 for b in brute) and any(b["clip_kept"] and not b["clip_kept"] & 1 for b in brute)


def _launch(dev, img, src, big_endian, sigma=3.0, maxiters=5):
    import torch
    from caesar_mrcnn_amd import ops
    from caesar_mrcnn_amd.sfinder import pack_sources
    pool, desc = pack_sources([p for _, p, _ in src])
    pool_t, desc_t = ops.tile_upload(pool, desc, dev)
    if big_endian:
        img_t = torch.from_numpy(img.astype(">f4").view(np.uint8).reshape(img.shape[0], img.shape[1], 4).copy()).to(dev)
    else:
        img_t = torch.from_numpy(img).to(dev)
    cut = np.array([c for _, _, c in src], np.int32)
    out = ops.source_params(img_t, pool_t, desc_t, cut, sigma, maxiters, big_endian=big_endian, desc_host=desc)
    return out.cpu().numpy().view(ops.source_record_dtype()).reshape(-1)


def _same(a, b):
    return a == b or (a != a and b != b)


def _check_record(name, r, b):
    """One device record against the brute force.  Exact: fill, counts, min / max, the integer moments, kept count,
    iterations, median.  Sums: |sum_dev - fsum| <= n 2^-53 sum|term| (recursive summation in any order).  Clipped mean: that
    bound over the kept values, divided by their count, plus one rounding of the quotient.  Clipped std: relative
    c k 2^-53 with c = 4: the two-pass formula's (k + 5) / 2 * 2^-53 (sfinder_params_cases.assert_params_close) against a
    brute force that is itself correct to a few 2^-53."""
    for k in ("fill", "n_mask", "npix", "smin", "smax", "m00", "m10", "m01", "clip_kept", "clip_iters", "clip_median"):
        assert _same(r[k], b[k]), (name, k, r[k], b[k])
    assert r["n_gathered"] == r["n_mask"]
    n = max(b["n_mask"], 1)
    for k in ("s64", "w00", "w10", "w01"):
        if not math.isfinite(b[k]):
            assert _same(float(r[k]), b[k]), (name, k, r[k], b[k])
        else:
            assert abs(float(r[k]) - b[k]) <= n * U * b["abs_" + k], (name, k, r[k], b[k], n * U * b["abs_" + k])
    kk = b["clip_kept"]
    if kk == 0:
        assert math.isnan(r["clip_mean"]) and math.isnan(r["clip_std"]), name
        return
    assert abs(float(r["clip_mean"]) - b["clip_mean"]) <= U * b["clip_abs"] + U * abs(b["clip_mean"]), (name, r["clip_mean"], b["clip_mean"])
    if b["clip_std"] > 0:
        assert abs(b["clip_mean"]) / b["clip_std"] * kk * U < 1e-6
    assert abs(float(r["clip_std"]) - b["clip_std"]) <= 4 * kk * U * b["clip_std"], (name, r["clip_std"], b["clip_std"])


@pytest.mark.parametrize("big_endian", [False, True], ids=["native", "big_endian"])
def test_source_params_equals_brute_force(dev, problem, big_endian):
    img, src, brute = problem
    rec = _launch(dev, img, src, big_endian)
    assert len(rec) == len(src)
    for (name, _, _), r, b in zip(src, rec, brute):
        _check_record(name, r, b)
    names = [s[0] for s in src]
    a, b = rec[3], rec[names.index("twice")]
    assert a.tobytes() == b.tobytes()                                     # the same source twice: the same record, bit for bit


def test_source_params_other_sigma_and_cap(dev, problem):
    """sigma and maxiters reach the kernel: no iteration at all, and a cap that lets the eight-rung ladder finish."""
    img, src, _ = problem
    by = {s[0]: s for s in src}
    pick = [by[k] for k in ("ladder8", "ladder2", "big", "n257")]
    for sigma, maxiters in ((3.0, 0), (3.0, 20), (2.0, 5)):
        brute = [cases.brute_record(img, p, c, sigma, maxiters) for _, p, c in pick]
        assert all(b["min_margin"] > 1e-9 for b in brute)
        assert brute[0]["clip_iters"] == {0: 0, 20: 9, 5: 5}[maxiters]
        rec = _launch(dev, img, pick, False, sigma, maxiters)
        for (name, _, _), r, b in zip(pick, rec, brute):
            _check_record("%s sigma %g maxiters %d" % (name, sigma, maxiters), r, b)


def test_source_params_is_reproducible(dev, problem):
    img, src, _ = problem
    a, b = _launch(dev, img, src, False), _launch(dev, img, src, False)
    assert a.tobytes() == b.tobytes()


def test_source_params_rejects_bad_input(dev, problem):
    import torch
    from caesar_mrcnn_amd import ops
    from caesar_mrcnn_amd._hip import HipPathError
    from caesar_mrcnn_amd.sfinder import pack_sources
    img, src, _ = problem
    pool, desc = pack_sources([src[0][1]])
    pool_t, desc_t = ops.tile_upload(pool, desc, dev)
    cut = np.array([src[0][2]], np.int32)
    with pytest.raises(HipPathError):
        ops.source_params(torch.from_numpy(img), pool_t, desc_t, cut)                      # image on the host
    with pytest.raises(HipPathError):
        ops.source_params(torch.from_numpy(img).to(dev), pool_t.cpu(), desc_t, cut)        # pool on the host
    with pytest.raises(AssertionError):
        ops.source_params(torch.from_numpy(img).to(dev), pool_t, desc_t, np.zeros((2, 4), np.int32))


# ---- SFinder -----------------------------------------------------------------------------------------------------
def _cut_of(sf, s):
    g = sf._cutout_geometry(s)
    return (g[0] - g[6], g[2] - g[7], g[1] + g[6] + 1, g[3] + g[7] + 1)


@pytest.mark.parametrize("hname", ["beam", "nobeam"])
def test_device_path_equals_host_on_fixture(dev, tmp_path, hname):
    """The fixture's cases through compute_sources_params, device against host: every key present, exact keys equal, the
    rest within the bounds of sfinder_params_cases.assert_params_close; the wrap-quirk source took the host path and is equal."""
    from caesar_mrcnn_amd.sfinder import SFinder
    img, hdrs, srcs, _ = cases.decode(np.load(cases.GOLDEN))
    path = str(tmp_path / "img.fits")
    cases.write_image(path, img, hdrs[hname])
    got = {}
    for device in (True, False):
        cfg = mcases.label_map_config(path)
        cfg.SPLIT_IMG_IN_TILES = False
        sf = SFinder(None, cfg)
        assert sf.compute_params is False
        sf.params_device = device
        sf.params_device_min_sources = 0
        assert sf.set_img_size_params() == 0
        sf.wcs = cases.RecorderWCS(sf.header)
        sf.sources = {"sources": [dict(s) for s in srcs]}
        assert sf.compute_sources_params() == 0
        assert sf.params_timing["failed_sources"] == 0
        assert sf.params_timing["device_sources"] == (len(srcs) - 1 if device else 0)      # all but the wrap-quirk source
        got[device] = sf.sources["sources"]
    for src, d, h in zip(srcs, got[True], got[False]):
        assert set(sf.PARAM_KEYS) <= set(d) and set(d) == set(h)
        dp, hp = {k: d[k] for k in sf.PARAM_KEYS}, {k: h[k] for k in sf.PARAM_KEYS}
        if src["name"] == "wrap":
            assert dp == hp
            continue
        cases.assert_params_close(dp, hp, cases.brute_record(img, src["pixels"], _cut_of(sf, src)), float(sf.beamArea), (2.0, 3.0))


def test_device_path_on_planted_mosaic(dev, tmp_path):
    """A tiled run with the label-map model: run_parallel computes the parameters on the device path and on the host; the two
    catalogues agree source by source."""
    from caesar_mrcnn_amd import fits
    from caesar_mrcnn_amd.sfinder import SFinder
    labels, n = mcases.planted_mosaic(3, nx=256, ny=256, n_try=60, rmax=14)
    path = str(tmp_path / "mosaic.fits")
    fits.write_fits(path, labels.astype(np.float32), dict(cases.BEAM_CARDS))
    got = {}
    for device in (True, False):
        cfg = mcases.label_map_config(path)
        cfg.TILE_XSIZE = cfg.TILE_YSIZE = 128
        cfg.TILE_XSTEP = cfg.TILE_YSTEP = 1.0
        sf = SFinder(mcases.LabelMapModel(cfg), cfg)
        sf.compute_params = True
        sf.params_device = device
        sf.params_device_min_sources = 0
        sf.outfile_json = str(tmp_path / ("cat%d.json" % device))
        sf.outfile_ds9 = str(tmp_path / ("cat%d.reg" % device))
        assert sf.run_parallel() == 0
        assert sf.params_timing["failed_sources"] == 0 and (sf.params_timing["device_sources"] > 0) == device
        got[device] = json.load(open(sf.outfile_json))["objs"]
    assert len(got[True]) == n == len(got[False])
    img = labels.astype(np.float32)
    wrapped = 0
    for d, h in zip(got[True], got[False]):
        assert set(sf.PARAM_KEYS) <= set(d) and set(d) == set(h)
        assert {k: d[k] for k in d if k not in sf.PARAM_KEYS} == {k: h[k] for k in h if k not in sf.PARAM_KEYS}
        dp, hp = {k: d[k] for k in sf.PARAM_KEYS}, {k: h[k] for k in sf.PARAM_KEYS}
        if d["x2"] == sf.nx or d["y2"] == sf.ny:                          # the wrap quirk: the host statement on both sides
            assert dp == hp
            wrapped += 1
            continue
        cases.assert_params_close(dp, hp, cases.brute_record(img, d["pixels"], _cut_of(sf, d)), float(sf.beamArea))
        assert d["flux"] == d["S"] / float(sf.beamArea)
    assert wrapped < n


# ---- command line ------------------------------------------------------------------------------------------------
def test_cli_compute_source_params(dev, tmp_path):
    from caesar_mrcnn_amd import fits
    d = str(tmp_path)
    rng = np.random.RandomState(0)
    yy, xx = np.mgrid[0:256, 0:256]
    img = rng.normal(0, 1, (256, 256)).astype(np.float32)
    for cy, cx in ((128, 128), (60, 127), (200, 40), (128, 200)):            # blobs on the tile borders of a 2 x 2 grid
        img += 80 * np.exp(-0.5 * (((yy - cy) / 6.0) ** 2 + ((xx - cx) / 9.0) ** 2))
    fits.write_fits(os.path.join(d, "mosaic.fits"), img, dict(cases.BEAM_CARDS, BUNIT="JY/BEAM"))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "run.py"), "detect", "--imgsize", "128", "--backbone", "custom",
                        "--logs", os.path.join(d, "logs"), "--image", os.path.join(d, "mosaic.fits"), "--scoreThr", "0.0",
                        "--split_img_in_tiles", "--tile_xsize", "128", "--tile_ysize", "128", "--merge_tile_sources",
                        "--compute_source_params"],
                       cwd=d, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=280)
    out = r.stdout.decode()
    assert r.returncode == 0, out[-3000:]
    assert glob.glob(os.path.join(d, "*.json")) == [os.path.join(d, "out_mosaic.json")]
    res = json.load(open(os.path.join(d, "out_mosaic.json")))
    c = cases.BEAM_CARDS
    beam = (np.pi * c["BMAJ"] * c["BMIN"] / (4 * np.log(2))) / np.abs(c["CDELT1"] * c["CDELT2"])
    keys = {"name", "x1", "x2", "y1", "y2", "class_id", "class_name", "score", "pixels", "vertexes", "edge", "merged"}
    params = {"nPix", "X0", "Y0", "X0w", "Y0w", "X0_wcs", "Y0_wcs", "X0w_wcs", "Y0w_wcs", "Xmin", "Xmax", "Ymin", "Ymax", "Xmin_wcs",
              "Xmax_wcs", "Ymin_wcs", "Ymax_wcs", "S", "Smin", "Smax", "Smean", "Smedian", "Sstddev", "flux"}
    assert "Computing source parameters" in out
    print("objects in the catalogue:", len(res["objs"]))
    assert len(res["objs"]) > 0                # (the weights are seeded: with --scoreThr 0.0 the untrained model reports objects)
    for s in res["objs"]:
        assert set(s) == keys | params
        assert s["flux"] == s["S"] / float(beam) and (s["Xmin"], s["Xmax"], s["Ymin"], s["Ymax"]) == (s["x1"], s["x2"], s["y1"], s["y2"])
        assert s["X0_wcs"] == -999 and s["Smin"] <= s["Smedian"] <= s["Smax"]
