"""The source-parameter step of the tiled source finder on the host: SFinder.compute_source_params against the reference
fixture (tests/golden/sfinder_params.npz), fits.sigma_clipped_stats and fits.SimpleWCS on inputs whose answer is known by hand,
the catalogue's JSON, the unchanged default output of run_parallel, and the dict building of the device path behind a NumPy
stand-in for the launch."""
import json
import math
import os

import numpy as np
import pytest

import sfinder_cases as mcases
import sfinder_params_cases as cases


def _finder(tmp_path, hname, img, cards, model=None, sub=None):
    from caesar_mrcnn_amd.sfinder import SFinder
    path = str(tmp_path / (hname + ".fits"))
    cases.write_image(path, img, cards)
    cfg = mcases.label_map_config(path)
    cfg.SPLIT_IMG_IN_TILES = False
    if sub:
        cfg.IMG_XMIN, cfg.IMG_XMAX, cfg.IMG_YMIN, cfg.IMG_YMAX = sub
    sf = SFinder(model, cfg)
    sf.params_device = False
    assert sf.set_img_size_params() == 0
    return sf


# ---- the host statement against the reference ----------------------------------------------------------------------
@pytest.mark.parametrize("hname", ["beam", "nobeam"])
def test_host_statement_equals_reference(tmp_path, monkeypatch, hname):
    """Every case of the fixture, under a header with and without the five beam keywords.  The fixture's clipped statistics are
    the generator's sentinel and its sky positions a recorder's affine answers: the same stand-ins are put in here.  Integers,
    Smin / Smax / S (float32 on both sides) and the beam area are compared exactly, and so is everything else: the moments are
    the same NumPy expressions on the same arrays."""
    from caesar_mrcnn_amd import fits
    img, hdrs, srcs, want = cases.decode(np.load(cases.GOLDEN))
    sf = _finder(tmp_path, hname, img, hdrs[hname])
    beam, rows = want[hname]
    assert (sf.nx, sf.ny) == (cases.NX, cases.NY)
    assert float(sf.beamArea) == beam and (beam > 0) == (hname == "beam")
    assert isinstance(sf.wcs, fits.SimpleWCS) and not sf.wcs.valid          # no CRVAL in these headers
    sf.wcs = cases.RecorderWCS(sf.header)
    monkeypatch.setattr(fits, "sigma_clipped_stats", lambda data, sigma=3.0, maxiters=5: cases.SENTINEL + (0, 0))
    assert [s["name"] for s in srcs] == [s["name"] for s in cases.make_sources()]
    for s, w in zip(srcs, rows):
        got = sf.compute_source_params(dict(s))
        assert set(got) == set(sf.PARAM_KEYS) == set(cases.INT_KEYS) | set(cases.FLOAT_KEYS) | {"S"}
        assert type(got["nPix"]) is int and all(type(got[k]) in (int, float) for k in got)
        for k in cases.INT_KEYS:
            assert got[k] == w[k], (s["name"], k)
        assert np.float32(got["S"]) == w["S"] and got["S"] == float(w["S"]), s["name"]
        for k in cases.FLOAT_KEYS:
            assert got[k] == w[k], (s["name"], k, got[k], w[k])
        assert [got[k] for k in ("Xmin_wcs", "Xmax_wcs", "Ymin_wcs", "Ymax_wcs")] == [-999] * 4
        assert got["flux"] == (got["S"] / beam if beam > 0 else got["S"])
    # what reached the WCS: [[x, y]] of a 2-axis header, origin 0, centroid first, weighted centroid second
    assert len(sf.wcs.calls) == 2 * len(srcs) and all(o == 0 and len(p) == 1 and len(p[0]) == 2 for p, o in sf.wcs.calls)


def test_wrap_quirk_and_clamps(tmp_path):
    """The geometry the fixture cases were built for: offsets clamp to 0 at the four borders, the exclusive x2 == nx gives -1."""
    img, hdrs, srcs, _ = cases.decode(np.load(cases.GOLDEN))
    sf = _finder(tmp_path, "nobeam", img, hdrs["nobeam"])
    off = {s["name"]: sf._cutout_geometry(s)[6:] for s in srcs}
    assert off["interior"] == (10, 10) and off["left"] == (0, 10) and off["top"] == (10, 0)
    assert off["right_excl"] == (0, 10) and off["bottom_incl"] == (10, 0) and off["wrap"] == (-1, 10)
    assert off["near_border"] == (3, 6) and off["merged"] == (10, 10)


def test_subimage_run_raises_and_is_caught(tmp_path, caplog):
    """IMG_XMIN .. given: nx = ny = 1 (sfinder.py:353-354), the offsets are hugely negative and the statement raises; the
    caller logs it and leaves the source without parameters."""
    img, hdrs, srcs, _ = cases.decode(np.load(cases.GOLDEN))
    sf = _finder(tmp_path, "nobeam", img, hdrs["nobeam"], sub=(0, 95, 0, 79))
    assert (sf.nx, sf.ny) == (1, 1)
    with pytest.raises(Exception):
        sf.compute_source_params(dict(srcs[0]))
    sf.sources = {"sources": [dict(srcs[0])]}
    with caplog.at_level("ERROR", logger="mrcnn"):
        assert sf.compute_sources_params() == 0
    assert "nPix" not in sf.sources["sources"][0] and sf.params_timing["failed_sources"] == 1
    assert any("parameters not computed" in r.getMessage() for r in caplog.records)


# ---- sigma_clipped_stats on constructed inputs -----------------------------------------------------------------------
def test_sigma_clipped_stats_by_hand():
    from caesar_mrcnn_amd.fits import sigma_clipped_stats as scs
    assert scs(np.full(17, 2.5, np.float32)) == (2.5, 2.5, 0.0, 17, 1)                   # constant: nothing removed, one iteration
    assert scs([4.0]) == (4.0, 4.0, 0.0, 1, 1)
    assert scs([1.0, 3.0]) == (2.0, 2.0, 1.0, 2, 1)                                      # even count: mean of the two middle values
    mean, med, std, k, it = scs([1.0, 2.0, 6.0])
    assert (mean, med, k, it) == (3.0, 2.0, 3, 1) and std == pytest.approx(math.sqrt(14.0 / 3.0), rel=1e-15)
    # twenty zeros and one 100: median 0, std = sqrt(20/21 * 100^2 / 21) = 21.3 < 100 / 3 -> the outlier goes in iteration 1,
    # iteration 2 removes nothing
    assert scs([0.0] * 20 + [100.0]) == (0.0, 0.0, 0.0, 20, 2)
    # odd kept count after one removal: 1 .. 7 and 1000.  Iteration 1: median 4.5, mean 128.5, std = 329.3, 4.5 + 3 std = 992.5 < 1000;
    # iteration 2 on 1 .. 7: median 4, std 2, [-2, 10] keeps all
    assert scs([1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 1000.0]) == (4.0, 4.0, 2.0, 7, 2)
    # a second round of removals: -1, 0 x 20, 1 and 1000.  1000 goes first; then std = sqrt(2 / 22) = 0.30 and 3 std < 1, so -1
    # and 1 go; the third iteration removes nothing
    assert scs([-1.0] + [0.0] * 20 + [1.0, 1000.0]) == (0.0, 0.0, 0.0, 20, 3)
    # NaN and +-inf are dropped first
    assert scs(np.array([np.nan, 1.0, np.inf, 3.0, -np.inf], np.float32)) == (2.0, 2.0, 1.0, 2, 1)
    assert scs([np.nan, np.inf])[3:] == (0, 0) and all(math.isnan(v) for v in scs([np.nan, np.inf])[:3])
    assert scs([])[3:] == (0, 0)


def _ladder(levels=8, base=10, ratio=1000.0):
    """`base` zeros-ish core values 0, then per level j = 1 .. levels one value ratio^j: each iteration's std is dominated by the
    top rung, 3 sigma reaches past it only while few values are below it -- exactly one rung goes per iteration."""
    core = [float(v) for v in range(-base, base + 1)]
    return core + [ratio ** j for j in range(1, levels + 1)]


def test_sigma_clipped_stats_cap():
    """A geometric ladder: with n values of which the largest is R times the rest, std ~ R / sqrt(n), so 3 std < R once n > 9:
    every iteration removes exactly the top rung.  Eight rungs need eight iterations; maxiters = 5 stops after five with three
    rungs left, maxiters = 20 runs all eight plus the one that removes nothing."""
    from caesar_mrcnn_amd.fits import sigma_clipped_stats as scs
    x = _ladder()
    mean, med, std, k, it = scs(x, 3.0, 5)
    assert (k, it) == (len(x) - 5, 5) and med == 1.5                     # -10 .. 10 and 3 rungs = 24 values: the middle pair is 1, 2
    mean, med, std, k, it = scs(x, 3.0, 20)
    assert (k, it) == (21, 9) and (mean, med) == (0.0, 0.0) and std == pytest.approx(math.sqrt(770.0 / 21.0), rel=1e-15)
    assert scs(x, 3.0, 0)[3:] == (len(x), 0)


def test_brute_force_agrees_with_host_clipping():
    """The float64 brute force behind the GPU tests follows the same clipping rule as the host statement."""
    from caesar_mrcnn_amd.fits import sigma_clipped_stats as scs
    rng = np.random.RandomState(5)
    for n in (1, 2, 3, 64, 257):
        v = rng.standard_cauchy(n).astype(np.float32)
        img = v.reshape(1, n)
        r = cases.brute_record(img, [[0, x] for x in range(n)], (0, 0, n, 1))
        mean, med, std, k, it = scs(v)
        assert (r["clip_kept"], r["clip_iters"], r["clip_median"]) == (k, it, med)
        assert r["clip_mean"] == pytest.approx(mean, rel=1e-12, abs=1e-300) and r["clip_std"] == pytest.approx(std, rel=1e-12, abs=1e-300)


# ---- SimpleWCS closed forms ----------------------------------------------------------------------------------------
def _hdr(**kw):
    h = {"NAXIS": 2, "NAXIS1": 100, "NAXIS2": 100, "CRPIX1": 51.0, "CRPIX2": 41.0, "CRVAL1": 83.5, "CRVAL2": -30.25,
         "CDELT1": -0.001, "CDELT2": 0.001}
    h.update(kw)
    return h


@pytest.mark.parametrize("proj", ["", "TAN", "SIN"])
def test_wcs_reference_pixel_maps_to_crval(proj):
    from caesar_mrcnn_amd.fits import SimpleWCS
    ct = {"CTYPE1": "RA---" + proj, "CTYPE2": "DEC--" + proj} if proj else {}
    w = SimpleWCS(_hdr(**ct))
    assert w.valid and w.naxis == 2
    (ra, dec), = w.all_pix2world([[50.0, 40.0]], 0)                      # 0-based pixel of CRPIX = (51, 41)
    assert ra == pytest.approx(83.5, abs=1e-11) and dec == pytest.approx(-30.25, abs=1e-11)
    (ra1, dec1), = w.all_pix2world([[51.0, 41.0]], 1)                    # the same pixel, 1-based
    assert (ra1, dec1) == (ra, dec)


def test_wcs_declination_step():
    """One pixel along the declination axis at the reference point: exactly CDELT2 in the linear case; for TAN the native
    latitude is atan(180 / (pi r)), so the step is atan(r) = r - r^3 / 3 (r in radians): CDELT2 to first order, and to
    1e-11 degrees after the cubic term."""
    from caesar_mrcnn_amd.fits import SimpleWCS
    lin = SimpleWCS(_hdr())
    (ra, dec), = lin.all_pix2world([[50.0, 41.0]], 0)
    assert ra == 83.5 and dec == -30.25 + 0.001
    (ra, dec), = lin.all_pix2world([[53.0, 40.0]], 0)
    assert ra == pytest.approx(83.5 - 0.003, abs=1e-12) and dec == -30.25
    tan = SimpleWCS(_hdr(CTYPE1="RA---TAN", CTYPE2="DEC--TAN"))
    (ra, dec), = tan.all_pix2world([[50.0, 41.0]], 0)
    r = math.radians(0.001)
    assert ra == pytest.approx(83.5, abs=1e-9)
    assert dec + 30.25 == pytest.approx(0.001, rel=1e-6)
    assert dec + 30.25 == pytest.approx(math.degrees(math.atan(r)), abs=1e-11)


def test_wcs_crota_swaps_axes_and_matrices_agree():
    from caesar_mrcnn_amd.fits import SimpleWCS
    rot = SimpleWCS(_hdr(CROTA2=90.0))
    # x' = -CDELT2 p2, y' = CDELT1 p1: a step in pixel x moves the second world axis by CDELT1, a step in y the first by -CDELT2
    (a, b), = rot.all_pix2world([[51.0, 40.0]], 0)
    assert a == pytest.approx(83.5, abs=1e-12) and b == pytest.approx(-30.25 - 0.001, abs=1e-12)
    (a, b), = rot.all_pix2world([[50.0, 41.0]], 0)
    assert a == pytest.approx(83.5 - 0.001, abs=1e-12) and b == pytest.approx(-30.25, abs=1e-12)
    # the same rotation as a PC matrix and as a CD matrix
    pc = SimpleWCS(_hdr(PC1_1=0.0, PC1_2=1.0, PC2_1=-1.0, PC2_2=0.0))
    cd = SimpleWCS(_hdr(CD1_1=0.0, CD1_2=-0.001, CD2_1=-0.001, CD2_2=0.0))
    for p in ([12.0, 70.0], [50.0, 40.0], [99.0, 0.0]):
        r, = rot.all_pix2world([p], 0)
        assert pc.all_pix2world([p], 0)[0] == pytest.approx(r, abs=1e-12) and cd.all_pix2world([p], 0)[0] == pytest.approx(r, abs=1e-12)


def test_wcs_ra_wraps_and_axes():
    from caesar_mrcnn_amd.fits import SimpleWCS
    w = SimpleWCS(_hdr(CTYPE1="RA---TAN", CTYPE2="DEC--TAN", CRVAL1=0.01, CRVAL2=0.0))
    (ra, dec), = w.all_pix2world([[80.0, 40.0]], 0)                       # 30 pixels towards smaller RA: 0.01 - 0.03 -> 359.98
    assert 359.97 < ra < 359.99 and dec == pytest.approx(0.0, abs=1e-12)
    (ra, dec), = w.all_pix2world([[20.0, 40.0]], 0)
    assert 0.03 < ra < 0.05
    # a 4-axis cube as the reference feeds it (sfinder.py:1085-1087): the celestial pair transformed, the rest linear
    w4 = SimpleWCS(_hdr(NAXIS=4, CTYPE1="RA---SIN", CTYPE2="DEC--SIN", CTYPE3="FREQ", CRVAL3=1.4e9, CDELT3=1e6, CRPIX3=1.0,
                        CTYPE4="STOKES", CRVAL4=1.0, CDELT4=1.0, CRPIX4=1.0))
    assert w4.naxis == 4
    row, = w4.all_pix2world([[50.0, 40.0, 0, 0]], 0)
    assert row[0] == pytest.approx(83.5, abs=1e-11) and row[1] == pytest.approx(-30.25, abs=1e-11) and row[2:] == [1.4e9, 1.0]


def test_wcs_unsupported_headers(tmp_path, caplog):
    from caesar_mrcnn_amd import fits
    assert not fits.SimpleWCS(_hdr(CTYPE1="RA---ZEA", CTYPE2="DEC--ZEA")).valid
    assert not fits.SimpleWCS(_hdr(CTYPE1="RA---SIN", CTYPE2="DEC--SIN", PV2_1=0.1)).valid
    assert not fits.SimpleWCS({"NAXIS": 2}).valid
    # keywords that cannot be used at all do not raise from the guarded constructor set_img_size_params uses
    assert not fits.SimpleWCS.from_header(_hdr(CRVAL1="abc")).valid
    assert not fits.SimpleWCS.from_header(_hdr(CDELT1=0.0, CROTA2=30.0)).valid
    assert fits.SimpleWCS.from_header(_hdr()).valid
    for name in ("galaxy0002.fits", "sidelobe0001.fits"):                 # the golden cut-outs carry no CRVAL / CDELT
        assert not fits.SimpleWCS(fits.get_fits_header(os.path.join(mcases.ROOT, "tests", "golden", name))).valid
    # -999 for the four sky keys and ONE warning for the whole catalogue
    img, hdrs, srcs, _ = cases.decode(np.load(cases.GOLDEN))
    sf = _finder(tmp_path, "nobeam", img, hdrs["nobeam"])
    sf.sources = {"sources": [dict(s) for s in srcs[:3]]}
    with caplog.at_level("WARNING", logger="mrcnn"):
        sf.compute_sources_params()
    assert all([s[k] for k in ("X0_wcs", "Y0_wcs", "X0w_wcs", "Y0w_wcs")] == [-999] * 4 for s in sf.sources["sources"])
    assert sum("No sky positions" in r.getMessage() for r in caplog.records) == 1


# ---- catalogue ------------------------------------------------------------------------------------------------------
def test_json_round_trip(tmp_path):
    """Analyzer.write_json_results is a plain json.dump: a catalogue with parameters goes through it and comes back equal."""
    img, hdrs, srcs, _ = cases.decode(np.load(cases.GOLDEN))
    sf = _finder(tmp_path, "beam", img, dict(hdrs["beam"], CRVAL1=10.0, CRVAL2=-45.0, CRPIX1=48.0, CRPIX2=40.0, CTYPE1="RA---SIN",
                                            CTYPE2="DEC--SIN"))
    assert sf.wcs.valid
    sf.sources = {"sources": [dict(s, score=0.9, class_id=1, class_name="source", vertexes=[]) for s in srcs]}
    assert sf.compute_sources_params() == 0
    assert all(set(sf.PARAM_KEYS) <= set(s) for s in sf.sources["sources"])          # the wrap-quirk source included
    sf.write_to_ds9 = False
    sf.outfile_json = str(tmp_path / "cat.json")
    sf.save()
    back = json.load(open(sf.outfile_json))
    assert back["objs"] == sf.sources["sources"]
    s = back["objs"][0]
    assert s["flux"] == s["S"] / float(sf.beamArea) and 9.0 < s["X0_wcs"] < 11.0 and -46.0 < s["Y0_wcs"] < -44.0


@pytest.fixture(scope="module")
def mosaic(tmp_path_factory):
    from caesar_mrcnn_amd import fits
    labels, n = mcases.planted_mosaic(3, nx=256, ny=256, n_try=60, rmax=14)
    path = str(tmp_path_factory.mktemp("params") / "mosaic.fits")
    fits.write_fits(path, labels.astype(np.float32), dict(cases.BEAM_CARDS))
    return path, n


def _run(path, tmp_path, tag, **attrs):
    from caesar_mrcnn_amd.sfinder import SFinder
    cfg = mcases.label_map_config(path)
    cfg.TILE_XSIZE = cfg.TILE_YSIZE = 128
    cfg.TILE_XSTEP = cfg.TILE_YSTEP = 1.0
    sf = SFinder(mcases.LabelMapModel(cfg), cfg)
    sf.merge_device = False
    sf.params_device = False
    for k, v in attrs.items():
        setattr(sf, k, v)
    sf.outfile_json = str(tmp_path / (tag + ".json"))
    sf.outfile_ds9 = str(tmp_path / (tag + ".reg"))
    assert sf.run_parallel() == 0
    return sf, json.load(open(sf.outfile_json))


def test_run_parallel_default_writes_the_same_keys(mosaic, tmp_path):
    from caesar_mrcnn_amd.sfinder import SFinder
    path, n = mosaic
    sf, res = _run(path, tmp_path, "plain")
    assert sf.compute_params is False and SFinder(None, sf.config).compute_params is False
    keys = {"name", "x1", "x2", "y1", "y2", "class_id", "class_name", "score", "pixels", "vertexes", "edge", "merged"}
    assert len(res["objs"]) == n and all(set(s) == keys for s in res["objs"])
    sf2, res2 = _run(path, tmp_path, "params", compute_params=True)
    assert all(set(s) == keys | set(sf.PARAM_KEYS) for s in res2["objs"])
    assert [{k: s[k] for k in keys} for s in res2["objs"]] == res["objs"]
    labels = np.rint(np.asarray([s["Smedian"] for s in res2["objs"]]))                   # the image IS the label map
    assert sorted(labels.tolist()) == list(range(1, n + 1))
    for s in res2["objs"]:
        if s["x2"] == sf2.nx or s["y2"] == sf2.ny:                        # the wrap quirk: a column / row folds onto another
            continue
        assert s["nPix"] == len(s["pixels"]) and s["Smin"] == s["Smax"] == s["Smean"] and s["Sstddev"] == 0.0
        assert s["flux"] == s["S"] / float(sf2.beamArea)


# ---- the device path's host half behind a NumPy stand-in ------------------------------------------------------------
def _standin(calls):
    import torch
    from caesar_mrcnn_amd import ops
    from caesar_mrcnn_amd.sfinder import unpack_bitmap

    def source_params(img, pool, desc, cutouts, sigma=3.0, maxiters=5, big_endian=False, desc_host=None):
        a = img.numpy()
        a = a.reshape(a.shape[0], a.shape[1] * 4).view(">f4").astype(np.float32) if big_endian else a
        words = pool.numpy().view(np.uint32)
        pix = []
        for x0, y0, w, h, off, wpr in desc.numpy().tolist():
            pix.append(np.argwhere(unpack_bitmap(words[off:off + h * wpr], h, w, wpr)) + (y0, x0))
        calls.append(len(pix))
        rec = cases.numpy_source_params(a, pix, np.asarray(cutouts), sigma, maxiters)
        return torch.from_numpy(rec.view(np.uint8).reshape(len(pix), -1).copy())
    return source_params


def test_compute_sources_params_dicts_with_standin(tmp_path, monkeypatch):
    """compute_sources_params with ops.source_params replaced by the brute force (and the "device" the CPU): every source the
    device path covers gets the dict the per-source host statement gives, within the bounds of
    sfinder_params_cases.assert_params_close; the wrap-quirk source goes to the host statement and is equal."""
    import torch
    from caesar_mrcnn_amd import ops
    img, hdrs, srcs, _ = cases.decode(np.load(cases.GOLDEN))
    sf = _finder(tmp_path, "beam", img, hdrs["beam"])
    sf.wcs = cases.RecorderWCS(sf.header)
    want = [sf.compute_source_params(dict(s)) for s in srcs]
    calls = []
    monkeypatch.setattr(ops, "source_params", _standin(calls))
    monkeypatch.setattr(sf, "_device", lambda: torch.device("cpu"))
    sf.params_device, sf.params_device_min_sources = True, 0
    empty = {"name": "empty", "x1": 5, "x2": 6, "y1": 5, "y2": 6, "pixels": []}
    sf.sources = {"sources": [dict(s) for s in srcs] + [empty]}
    assert sf.compute_sources_params() == 0
    assert calls == [len(srcs) - 1]                                       # one launch; the wrap-quirk and the empty source not in it
    assert sf.params_timing["device_sources"] == len(srcs) - 1 and sf.params_timing["host_sources"] == 2
    assert sf.params_timing["failed_sources"] == 1 and "nPix" not in sf.sources["sources"][-1]
    for s, src, w in zip(sf.sources["sources"], srcs, want):
        got = {k: s[k] for k in sf.PARAM_KEYS}
        if src["name"] == "wrap":
            assert got == w
            continue
        g = sf._cutout_geometry(src)
        cut = (g[0] - g[6], g[2] - g[7], g[1] + g[6] + 1, g[3] + g[7] + 1)
        rec = cases.brute_record(img, src["pixels"], cut)
        cases.assert_params_close(got, w, rec, float(sf.beamArea), (2.0, 3.0))


def test_hip_path_error_falls_back_to_host(tmp_path, monkeypatch, caplog):
    import torch
    from caesar_mrcnn_amd import ops
    from caesar_mrcnn_amd._hip import HipPathError
    img, hdrs, srcs, _ = cases.decode(np.load(cases.GOLDEN))
    sf = _finder(tmp_path, "beam", img, hdrs["beam"])
    want = [sf.compute_source_params(dict(s)) for s in srcs]

    def refuse(*a, **k):
        raise HipPathError("no device")
    monkeypatch.setattr(ops, "source_params", refuse)
    monkeypatch.setattr(sf, "_device", lambda: torch.device("cpu"))
    sf.params_device, sf.params_device_min_sources = True, 0
    sf.sources = {"sources": [dict(s) for s in srcs]}
    with caplog.at_level("WARNING", logger="mrcnn"):
        assert sf.compute_sources_params() == 0
    assert sum("Source parameters on the host" in r.getMessage() for r in caplog.records) == 1
    assert [{k: s[k] for k in sf.PARAM_KEYS} for s in sf.sources["sources"]] == want


def test_ops_source_params_needs_device_tensors():
    import torch
    from caesar_mrcnn_amd import ops
    from caesar_mrcnn_amd._hip import HipPathError
    from caesar_mrcnn_amd.sfinder import pack_sources
    pool, desc = pack_sources([[[1, 1]]])
    pool_t, desc_t = ops.tile_upload(pool, desc, torch.device("cpu"))
    with pytest.raises(HipPathError):
        ops.source_params(torch.zeros((4, 4)), pool_t, desc_t, np.array([[0, 0, 4, 4]], np.int32))
