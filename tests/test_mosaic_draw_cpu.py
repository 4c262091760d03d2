"""The overview picture of a mosaic, host statements: fits.mosaic_overview_host, sfinder.source_planes_host,
SFinder.mosaic_scene / render_mosaic / draw_mosaic_results and the run.py flags.  No GPU."""
import importlib.util
import logging
import os

import numpy as np
import pytest

import draw_cases
import mosaic_draw_cases as cases
import sfinder_tiles_cases as tiles
from caesar_mrcnn_amd import draw, fits, sfinder

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the overview frame ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("contrast", [0.25, 0.1])
def test_overview_at_shrink_1_is_read_fits(tmp_path, contrast):
    path = str(tmp_path / "p.fits")
    plane = cases.plane_97x61()
    assert np.isnan(plane).sum() > 100 and np.isneginf(plane).sum() == 1
    fits.write_fits(path, plane)
    want = fits.read_fits(path, zscale_contrasts=[contrast] * 3)[0]
    stored = fits.read_primary_hdu(path, native=False)[0]                     # what SFinder._image_plane() returns
    assert stored.dtype == np.dtype(">f4")
    for p in (stored, plane):
        got = fits.mosaic_overview_host(p, 1, contrast)
        assert got.dtype == np.uint8 and got.shape == (97, 61, 3)
        assert np.array_equal(got, want)
    assert len(np.unique(want)) > 50                                          # a picture, not a constant


def _block_max_by_loop(G, k):
    ny, nx = G.shape
    h, w = -(-ny // k), -(-nx // k)
    O = np.zeros((h, w), np.uint8)
    for Y in range(h):
        for X in range(w):
            O[Y, X] = max(int(G[y, x]) for y in range(k * Y, min(k * (Y + 1), ny)) for x in range(k * X, min(k * (X + 1), nx)))
    return O


def test_block_maximum_by_hand():
    plane = np.arange(35, dtype=np.float32).reshape(7, 5) * 3.0 - 20.0
    plane[0:3, 0:3] = np.nan                      # block (0, 0) at k = 2 and at k = 3: all NaN -> filled with the minimum -> byte 0
    plane[6, 4] = 500.0                           # the maximum: byte 255, alone in the last (partial) block at k = 2 and k = 3
    G = fits.mosaic_overview_host(plane, 1)[..., 0]
    assert G.shape == (7, 5) and G[6, 4] == 255 and not G[0:3, 0:3].any()
    for k, shape in ((2, (4, 3)), (3, (3, 2))):
        got = fits.mosaic_overview_host(plane, k)
        assert got.shape == shape + (3,) and got.dtype == np.uint8
        assert np.array_equal(got[..., 0], got[..., 1]) and np.array_equal(got[..., 0], got[..., 2])
        assert np.array_equal(got[..., 0], _block_max_by_loop(G, k))
        assert got[0, 0, 0] == 0 and got[-1, -1, 0] == 255
    # k = 2: the last row of blocks holds row 6 only, the last column of blocks column 4 only
    O = fits.mosaic_overview_host(plane, 2)[..., 0]
    assert O[3, 0] == max(G[6, 0], G[6, 1]) and O[1, 2] == max(G[2, 4], G[3, 4])
    # a shrink larger than either side: one pixel, the maximum
    assert fits.mosaic_overview_host(plane, 9)[..., 0].tolist() == [[255]]
    for bad in (0, -1, 1.5):
        with pytest.raises(ValueError):
            fits.mosaic_overview_host(plane, bad)


def test_plane_without_a_finite_pixel_gives_zeros():
    for fill in (np.nan, np.inf, -np.inf):
        got = fits.mosaic_overview_host(np.full((5, 7), fill, np.float32), 2)
        assert got.shape == (3, 4, 3) and got.dtype == np.uint8 and not got.any()
    one = fits.mosaic_overview_host(cases.plane_one_finite(), 1)
    assert one.shape == (9, 13, 3)                # a constant plane after the fill: 0 / 0 on the host as in read_fits


# ---- sources as planes -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,h,w", [(1, 12, 33), (2, 9, 33), (3, 7, 64), (5, 4, 11), (40, 2, 2)])
def test_source_planes_host_against_the_pixel_loop(k, h, w):
    lists = cases.source_cases(k, h, w)
    pool, desc = sfinder.pack_sources(lists)
    got = sfinder.source_planes_host(pool, desc, k, h, w)
    want = cases.planes_by_loop(lists, k, h, w)
    assert got.dtype == np.bool_ and got.shape == (len(lists), h, w)
    assert np.array_equal(got, want)
    span, wide, single, empty, last, outside = range(6)
    assert got[single].sum() == 1 and not got[empty].any() and got[last, h - 1, w - 1] and got[last].sum() == 1
    assert got[span].sum() >= 4 and got[wide, min(k * h - 1, 1) // k].all()
    assert got[outside].sum() == 2 and got[outside, 0, 0] and got[outside, (k * h // 2) // k, w - 1]     # the rest is dropped
    boxes = sfinder.plane_boxes_host(got)
    assert boxes[empty].tolist() == [0, 0, 0, 0] and boxes[last].tolist() == [h - 1, w - 1, h, w]


# ---- the scene -----------------------------------------------------------------------------------------------------------------------
def _catalogue_finder(tmp_path, **settings):
    rng = np.random.RandomState(3)
    plane = rng.normal(0, 1, cases.CATALOGUE_PLANE_SHAPE).astype(np.float32)
    sf = cases.sfinder_for(str(tmp_path / "cat.fits"), plane, cases.catalogue())
    for k, v in settings.items():
        setattr(sf, k, v)
    return sf, plane


def test_new_attributes_and_their_defaults(tmp_path):
    sf, _ = _catalogue_finder(tmp_path)
    assert sf.draw_mosaic is False and sf.mosaic_outfile == "" and sf.mosaic_shrink is None and sf.mosaic_scale is None
    assert sf.mosaic_captions == "name" and sf.mosaic_shaded is False and sf.mosaic_device == sf.merge_device


def test_scene_of_a_three_source_catalogue(tmp_path):
    sf, plane = _catalogue_finder(tmp_path, mosaic_shrink=3, mosaic_scale=2)
    sc = sf.mosaic_scene()
    assert sc["scale"] == 2 and sc["shaded"] is False and sc["gt_boxes"] == [] and sc["gt_colours"] == []
    assert np.array_equal(sc["image"], fits.mosaic_overview_host(plane, 3, 0.25)) and sc["image"].shape == (17, 24, 3)
    # boxes of the PLANES at shrink 3 (y1, x1, y2, x2; upper corner exclusive): rows 4 .. 8 -> 1 .. 2, columns 10 .. 20 -> 3 .. 6;
    # rows 20 .. 30 -> 6 .. 10, columns 33 .. 39 -> 11 .. 13; pixel (47, 66) -> (15, 22)
    assert sc["boxes"] == [[1, 3, 3, 7], [6, 11, 11, 14], [15, 22, 16, 23]]
    assert sc["colours"] == [draw.CLASS_COLOR_MAP["compact"], draw.CLASS_COLOR_MAP["extended"], draw.UNKNOWN_COLOUR]
    assert sc["colours"][:2] == [(0, 0, 1), (1, 1, 0)]
    assert [m.shape for m in sc["masks"]] == [(17, 24)] * 3 and [int(m.sum()) for m in sc["masks"]] == [8, 11, 1]      # 2 x 4; 5 x 2 and the block of (25, 39); 1
    assert np.array_equal(np.stack(sc["masks"]).astype(bool), cases.planes_by_loop([s["pixels"] for s in cases.catalogue()], 3, 17, 24))
    assert sc["texts"] == [("S1", 3, 0, draw.CAPTION_COLOUR), ("S2", 11, 5, draw.CAPTION_COLOUR), ("S3", 22, 14, draw.CAPTION_COLOUR)]
    sf.mosaic_captions = "score"
    assert [t[0] for t in sf.mosaic_scene()["texts"]] == ["0.91", "0.50", "1.00"]
    assert [t[1:] for t in sf.mosaic_scene()["texts"]] == [t[1:] for t in sc["texts"]]
    sf.mosaic_captions = "none"
    assert sf.mosaic_scene()["texts"] == []
    sf.mosaic_shaded = True
    assert sf.mosaic_scene()["shaded"] is True
    # at shrink 1 the merged source's box is the exclusive one as well, whatever its catalogue entry says
    sf.mosaic_shrink = 1
    assert sf.mosaic_scene()["boxes"] == [[4, 10, 9, 21], [20, 33, 31, 40], [47, 66, 48, 67]]
    # an empty catalogue: the bare overview
    sf.sources = {"sources": []}
    sc = sf.mosaic_scene()
    assert sc["masks"] == [] and sc["boxes"] == [] and sc["texts"] == [] and sc["image"].shape == (50, 70, 3)
    assert np.array_equal(sf.render_mosaic(False)[4:104, 4:144], np.repeat(np.repeat(sc["image"], 2, axis=0), 2, axis=1))


def test_settings_that_cannot_be_drawn(tmp_path, caplog):
    for name, bad in (("mosaic_shrink", 0), ("mosaic_shrink", 2.5), ("mosaic_scale", 0), ("mosaic_captions", "class")):
        sf, _ = _catalogue_finder(tmp_path, **{name: bad})
        caplog.clear()
        assert sf.mosaic_scene() is None and sf.render_mosaic(False) is None and sf.draw_mosaic_results(False) == -1
        assert any("nothing is drawn" in r.getMessage() for r in caplog.records)


@pytest.mark.parametrize("shape,k,hw,scale", [((384, 320), 1, (384, 320), 2), ((4352, 4352), 5, (871, 871), 1),
                                              ((1024, 1000), 1, (1024, 1000), 1), ((1025, 100), 2, (513, 50), 1)])
def test_default_shrink_and_scale(tmp_path, shape, k, hw, scale):
    sf, _ = _catalogue_finder(tmp_path)
    sf._plane = (np.broadcast_to(np.float32(0), shape), sf.config.IMG_PATH, {})
    assert sf._mosaic_geometry() == shape + (k,) + hw + (scale,)
    assert scale == draw.default_scale(*hw)


# ---- a whole run ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def drawn_run(tmp_path_factory):
    """One tiled run of the stub model over the mosaic of sfinder_tiles_cases with draw_mosaic on (host statement), and one
    without, in a directory of their own."""
    d = tmp_path_factory.mktemp("mosaic_run")
    path = str(d / "mosaic.fits")
    tiles.write_mosaic(path)
    cwd = os.getcwd()
    os.chdir(str(d))
    try:
        def on(sf):
            sf.draw_mosaic, sf.mosaic_device = True, False
        plain = tiles.run(path, 0, outdir=str(d), tag="plain")
        assert [f for f in os.listdir(str(d)) if f.endswith(".png")] == []          # no flag, no picture
        drawn = tiles.run(path, 0, outdir=str(d), tag="drawn", setup=on)
    finally:
        os.chdir(cwd)
    return str(d), plain, drawn


def test_run_with_draw_mosaic_writes_the_png_and_changes_nothing_else(drawn_run):
    d, plain, drawn = drawn_run
    assert sorted(f for f in os.listdir(d) if f.endswith(".png")) == ["mosaic_mosaic.png"]
    assert len(drawn.sources["sources"]) >= 10 and drawn.sources == plain.sources
    for ext in ("json", "reg"):
        assert open(os.path.join(d, "cat_plain." + ext)).read() == open(os.path.join(d, "cat_drawn." + ext)).read()
    assert drawn._plane is None and drawn._plane_dev is None                      # the whole image is not kept beyond the run
    pixels, _ = draw_cases.png_pixels(open(os.path.join(d, "mosaic_mosaic.png"), "rb").read())
    assert np.array_equal(pixels, drawn.render_mosaic(False))                     # the PNG round trip, through zlib


def test_render_mosaic_host_on_the_stub_catalogue(drawn_run):
    d, plain, drawn = drawn_run
    canvas = drawn.render_mosaic(False)
    h, w, s = tiles.NY, tiles.NX, 2                                               # shrink 1, scale 1024 // (384 + 4)
    assert canvas.dtype == np.uint8 and canvas.shape == (s * (h + 4), s * (w + 4), 3) == draw.canvas_shape(h, w, s)
    sc = drawn.mosaic_scene()
    assert len(sc["boxes"]) == len(drawn.sources["sources"]) and sc["scale"] == s
    blue = draw.colour8(draw.CLASS_COLOR_MAP["source"])
    for (y1, x1, y2, x2), src in zip(sc["boxes"], drawn.sources["sources"]):
        p = np.asarray(src["pixels"])
        assert (y1, x1, y2, x2) == (p[:, 0].min(), p[:, 1].min(), p[:, 0].max() + 1, p[:, 1].max() + 1)
        inside = canvas[s * (y1 + 2):s * (y2 + 2), s * (x1 + 2):s * (x2 + 2)]
        assert (inside == np.array(blue, np.uint8)).all(axis=2).any()               # the contour, in the class colour
    # the frame under the overlay is the overview: a corner no source touches
    frame = fits.mosaic_overview_host(tiles.mosaic(), 1)
    assert np.array_equal(canvas[s * 2, s * 2], frame[0, 0]) or any(b[0] == 0 and b[1] == 0 for b in sc["boxes"])
    assert (canvas[0, 0] == 255).all()                                            # the white margin
    assert drawn.mosaic_timing["sources"] == len(sc["boxes"])


def test_mosaic_outfile_is_used(drawn_run, tmp_path):
    d, plain, drawn = drawn_run
    drawn.mosaic_outfile = str(tmp_path / "named.png")
    assert drawn.draw_mosaic_results(False) == 0
    pixels, names = draw_cases.png_pixels(open(drawn.mosaic_outfile, "rb").read())
    assert names == [b"IHDR", b"IDAT", b"IEND"] and np.array_equal(pixels, drawn.render_mosaic(False))


# ---- run.py --------------------------------------------------------------------------------------------------------------------------
def _run_py():
    spec = importlib.util.spec_from_file_location("_run_py_mosaic", os.path.join(ROOT, "scripts", "run.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_run_py_flags(caplog, monkeypatch):
    run = _run_py()
    base = ["detect", "--image", "a.fits"]
    tiled = base + ["--split_img_in_tiles", "--merge_tile_sources"]
    args = run.parse_args(tiled)
    assert args.draw_mosaic is False and args.mosaic_outfile == "" and args.mosaic_shrink == 0
    assert run.mosaic_settings(args) == (False, "", None)
    assert run.mosaic_settings(run.parse_args(tiled + ["--draw_mosaic"])) == (True, "", None)
    assert run.mosaic_settings(run.parse_args(tiled + ["--mosaic_outfile", "m.png"])) == (True, "m.png", None)      # implies the flag
    assert run.mosaic_settings(run.parse_args(tiled + ["--draw_mosaic", "--mosaic_shrink", "4"])) == (True, "", 4)
    assert not [r for r in caplog.records if r.levelno >= logging.WARNING]
    # without the tile flags: one warning, nothing drawn
    for argv in (base + ["--draw_mosaic"], base + ["--split_img_in_tiles", "--mosaic_outfile", "m.png"],
                 ["test", "--datalist", "l.dat", "--draw_mosaic"]):
        caplog.clear()
        assert run.mosaic_settings(run.parse_args(argv))[0] is False
        assert len([r for r in caplog.records if r.levelno == logging.WARNING and "--draw_mosaic" in r.getMessage()]) == 1
    # the old flags keep their meaning on a tiled run
    caplog.clear()
    assert run.draw_settings(run.parse_args(tiled + ["--draw", "--draw_mosaic"]), ntiles=4) == (False, "")
    assert any("draws nothing" in r.getMessage() for r in caplog.records)
    # detect_merged hands the settings to the SFinder
    seen = []

    def fake_run(self):
        seen.append((self.draw_mosaic, self.mosaic_outfile, self.mosaic_shrink))
        return 0
    monkeypatch.setattr(sfinder.SFinder, "run_parallel", fake_run)
    cfg = tiles.config("a.fits")
    for extra in ([], ["--draw_mosaic"], ["--mosaic_outfile", "m.png", "--mosaic_shrink", "2"]):
        assert run.detect_merged(run.parse_args(tiled + extra), tiles.ThresholdModel(cfg), cfg) == 0
    assert seen == [(False, "", None), (True, "", None), (True, "m.png", 2)]
