"""The overview picture of a mosaic on the GPU: ops.mosaic_overview and ops.sources_to_planes byte for byte
against their host statements, the refusals of the C entries, SFinder.render_mosaic on the device against the host statement,
and a whole run with draw_mosaic."""
import ctypes as C
import os

import numpy as np
import pytest

import draw_cases
import mosaic_draw_cases as cases
import sfinder_tiles_cases as tiles

pytestmark = pytest.mark.gpu


def _overview(dev, plane, k, contrast=0.25, big=False):
    import torch
    from caesar_mrcnn_amd import ops
    if big:
        t = torch.from_numpy(plane.astype(">f4").view(np.uint8).reshape(plane.shape + (4,)).copy()).to(dev)
    else:
        t = torch.from_numpy(np.ascontiguousarray(plane, dtype=np.float32)).to(dev)
    return ops.mosaic_overview(t, k, contrast, big_endian=big).cpu().numpy()


# ---- the overview frame ----------------------------------------------------------------------------------------------------------
PLANES = {"nans_and_minus_inf": cases.plane_97x61, "nan_chunks": cases.plane_nan_chunks,
          "nan_chunks_infinite_fill": cases.plane_nan_chunks_infinite_fill}


@pytest.mark.parametrize("name", sorted(PLANES))
def test_overview_equals_the_host_statement(dev, name):
    from caesar_mrcnn_amd import fits
    plane = PLANES[name]()
    for k in (1, 2, 3, 7, 61, 100):                                  # 100: larger than both sides -- one output pixel
        want = fits.mosaic_overview_host(plane, k)
        got = _overview(dev, plane, k)
        assert got.shape == want.shape and got.dtype == np.uint8
        assert np.array_equal(got, want), (name, k, int((got != want).sum()))
        assert np.array_equal(_overview(dev, plane, k, big=True), want), (name, k, "big-endian")
    assert np.array_equal(_overview(dev, plane, 2, contrast=0.1), fits.mosaic_overview_host(plane, 2, 0.1))
    assert len(np.unique(fits.mosaic_overview_host(plane, 1))) > 50


def test_overview_is_reproducible_and_reads_unaligned_planes(dev):
    import torch
    from caesar_mrcnn_amd import fits, ops
    plane = cases.plane_nan_chunks()
    want = fits.mosaic_overview_host(plane, 3)
    buf = torch.zeros(plane.size + 1, dtype=torch.float32, device=dev)
    buf[1:] = torch.from_numpy(plane.reshape(-1)).to(dev)
    view = buf[1:].view(plane.shape)                                 # 4 bytes past a 16-byte boundary: the dword loads
    assert view.data_ptr() % 16 == 4
    a = ops.mosaic_overview(view, 3).cpu().numpy()
    b = ops.mosaic_overview(view, 3).cpu().numpy()
    assert np.array_equal(a, want) and np.array_equal(a, b)


def test_overview_of_degenerate_planes(dev):
    from caesar_mrcnn_amd import fits
    for k in (1, 4):
        one = cases.plane_one_finite()
        assert np.array_equal(_overview(dev, one, k), fits.mosaic_overview_host(one, k))
        for fill in (np.nan, np.inf, -np.inf):
            blank = np.full((9, 13), fill, np.float32)
            got = _overview(dev, blank, k)
            assert got.shape == (-(-9 // k), -(-13 // k), 3) and not got.any()
            assert np.array_equal(got, fits.mosaic_overview_host(blank, k))


def test_overview_past_the_one_workgroup_chunk_table(dev):
    """2049 x 2048: 4098 chunks, five super-chunks -- the shape mrcnn_fits_tiles_to_rgb refuses and the new scan exists for."""
    from caesar_mrcnn_amd import fits, ops
    plane = cases.plane_2049x2048()
    assert plane.size > fits.DEVICE_TILE_MAX_PIXELS
    want = fits.mosaic_overview_host(plane, 2)
    got = _overview(dev, plane, 2)
    assert got.shape == (1025, 1024, 3) and np.array_equal(got, want), int((got != want).sum())
    assert np.array_equal(_overview(dev, plane, 2, big=True), want)
    with pytest.raises(ops.FitsTileUnsupported):                     # the tile chain keeps its limit
        import torch
        ops.fits_tiles_to_rgb(torch.from_numpy(plane).to(dev), [(0, 0, 2048, 2049)])


def test_overview_refusals_launch_nothing(dev):
    import torch
    from caesar_mrcnn_amd import _hip, ops
    L = _hip.lib()
    assert L.mrcnn_mosaic_overview_check(97, 61, 2, 0.25) == 0
    for ny, nx, k, c in ((0, 61, 1, 0.25), (97, -1, 1, 0.25), (97, 61, 0, 0.25), (97, 61, -3, 0.25), (97, 61, 1, float("nan")),
                         (97, 61, 1, float("inf"))):
        assert L.mrcnn_mosaic_overview_check(ny, nx, k, c) == -1, (ny, nx, k, c)
    assert L.mrcnn_mosaic_overview_check(46341, 46341, 1, 0.25) == -4             # 2^31 + 88 pixels
    assert L.mrcnn_mosaic_overview_check(65536, 32768, 16, 0.25) == -4            # 2^31 pixels
    assert L.mrcnn_mosaic_overview_check(65536, 32767, 16, 0.25) == 0             # 2^31 - 65536: inside the cap
    assert L.mrcnn_mosaic_overview_workspace(65536, 32768) == 0 and L.mrcnn_mosaic_overview_workspace(0, 5) == 0
    assert L.mrcnn_mosaic_overview_workspace(97, 61) >= 6 * 24 + 16
    plane = torch.from_numpy(cases.plane_97x61()).to(dev)
    out = torch.full((49, 31, 3), 0xA5, dtype=torch.uint8, device=dev)
    ws = torch.full((4096,), 0x5A, dtype=torch.uint8, device=dev)
    stream = _hip.current_stream()

    def call(ny=97, nx=61, k=2, c=0.25, p=plane.data_ptr(), o=out.data_ptr(), ob=out.numel(), w=ws.data_ptr(), wb=ws.numel()):
        return L.mrcnn_mosaic_overview(p, 0, ny, nx, k, c, o, ob, w, wb, stream)
    assert call(ny=65536, nx=32768) == -4                                          # a claimed plane past the cap
    assert call(k=0) == -1 and call(ny=0) == -1 and call(c=float("nan")) == -1
    assert call(p=None) == -1 and call(o=None) == -1 and call(ob=out.numel() - 1) == -1 and call(p=plane.data_ptr() + 2) == -1
    assert call(w=None) == -3 and call(wb=16) == -3 and call(w=ws.data_ptr() + 4) == -3
    torch.cuda.synchronize()
    assert bool((out == 0xA5).all()) and bool((ws == 0x5A).all())                 # the sentinels keep their bytes
    assert call() == 0
    torch.cuda.synchronize()
    assert not bool((out == 0xA5).all())
    # the wrapper: ValueError for a malformed call
    for bad in (lambda: ops.mosaic_overview(plane, 0), lambda: ops.mosaic_overview(plane, 1.5), lambda: ops.mosaic_overview(plane.reshape(-1), 1),
                lambda: ops.mosaic_overview(plane, 1, float("nan")), lambda: ops.mosaic_overview(plane, 1, big_endian=True),
                lambda: ops.mosaic_overview(plane.double(), 1)):
        with pytest.raises(ValueError):
            bad()
    assert issubclass(ops.MosaicUnsupported, _hip.HipPathError)


# ---- sources as planes -------------------------------------------------------------------------------------------------------------
def _check_planes(dev, lists, k, h, w):
    from caesar_mrcnn_amd import ops, sfinder
    pool, desc = sfinder.pack_sources(lists)
    want = sfinder.source_planes_host(pool, desc, k, h, w)
    assert np.array_equal(want, cases.planes_by_loop(lists, k, h, w))
    pool_t, desc_t = ops.tile_upload(pool, desc, dev)
    planes = ops.sources_to_planes(pool_t, desc_t, k, h, w)
    assert (planes.n, planes.H, planes.W, planes.wpr) == (len(lists), h, w, (w + 31) // 32)
    bits, padding = cases.unpack_words(planes.words.cpu().numpy(), w)
    assert np.array_equal(bits, want), (k, h, w, int((bits != want).sum()))
    assert not padding.any()
    assert planes.count.cpu().numpy().tolist() == want.sum(axis=(1, 2)).tolist()
    assert np.array_equal(planes.box.cpu().numpy(), sfinder.plane_boxes_host(want))
    return planes


@pytest.mark.parametrize("k,h,w", [(1, 12, 33), (2, 9, 33), (3, 7, 64), (5, 4, 11), (40, 2, 2), (1, 5, 65), (33, 3, 40)])
def test_source_planes_of_the_cpu_cases(dev, k, h, w):
    _check_planes(dev, cases.source_cases(k, h, w), k, h, w)


@pytest.mark.parametrize("k", [1, 2, 5])
def test_source_planes_of_seeded_blobs(dev, k):
    from caesar_mrcnn_amd import ops
    lists = cases.blobs_384x320()
    h, w = -(-384 // k), -(-320 // k)
    planes = _check_planes(dev, lists, k, h, w)
    if k == 1:                                                       # the planes are those mask_planes_pack makes of the masks
        import torch
        masks = np.ascontiguousarray(cases.planes_by_loop(lists, 1, h, w).transpose(1, 2, 0)).astype(np.uint8)
        packed = ops.mask_planes_pack(torch.from_numpy(masks).to(dev))
        assert bool((packed.words == planes.words).all()) and bool((packed.box == planes.box).all()) and bool((packed.count == planes.count).all())
    # a smaller frame than the mosaic: everything past it is dropped
    _check_planes(dev, lists, k, h // 2, 33)


def test_source_planes_refusals_launch_nothing(dev):
    import torch
    from caesar_mrcnn_amd import _hip, ops, sfinder
    L = _hip.lib()
    assert L.mrcnn_sources_to_planes_check(3, 2, 10, 33) == 0
    for a in ((0, 2, 10, 33), (3, 0, 10, 33), (3, 2, 0, 33), (3, 2, 10, -1)):
        assert L.mrcnn_sources_to_planes_check(*a) == -1, a
    assert L.mrcnn_sources_to_planes_check(70000, 1, 1024, 1024) == -4            # 2.29e9 words
    assert L.mrcnn_sources_to_planes_check(1, 1 << 20, 4096, 8) == -4             # shrink * h = 2^32
    pool, desc = sfinder.pack_sources(cases.source_cases(2, 10, 33))
    pool_t, desc_t = ops.tile_upload(pool, desc, dev)
    n = len(desc)
    words = torch.full((n, 10, 2), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    count = torch.full((n,), -7, dtype=torch.int32, device=dev)
    box = torch.full((n, 4), -7, dtype=torch.int32, device=dev)
    stream = _hip.current_stream()

    def call(nn=n, k=2, h=10, w=33, p=pool_t.data_ptr(), pw=pool_t.numel(), d=desc_t.data_ptr(), o=words.data_ptr()):
        return L.mrcnn_sources_to_planes(p, pw, d, nn, k, h, w, o, count.data_ptr(), box.data_ptr(), stream)
    assert call(nn=0) == -1 and call(k=0) == -1 and call(h=-2) == -1 and call(p=None) == -1 and call(d=None) == -1 and call(o=None) == -1
    assert call(pw=-1) == -1 and call(nn=70000, h=1024, w=1024) == -4
    torch.cuda.synchronize()
    assert bool((words == 0x5A5A5A5A).all()) and bool((count == -7).all()) and bool((box == -7).all())
    for bad in (lambda: ops.sources_to_planes(pool_t, desc_t, 0, 10, 33), lambda: ops.sources_to_planes(pool_t, desc_t, 2, 10.5, 33),
                lambda: ops.sources_to_planes(pool_t, desc_t, 2, 10, 0)):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(ops.MosaicUnsupported):
        ops.sources_to_planes(pool_t, desc_t, 1 << 20, 4096, 8)


# ---- the picture ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """The mosaic of sfinder_tiles_cases through the stub model: a batched run (resident plane) with draw_mosaic on the device,
    and a tile-at-a-time run without it."""
    d = tmp_path_factory.mktemp("mosaic_gpu")
    path = str(d / "mosaic.fits")
    tiles.write_mosaic(path)
    cwd = os.getcwd()
    os.chdir(str(d))
    try:
        plain = tiles.run(path, 0, outdir=str(d), tag="plain")
        assert [f for f in os.listdir(str(d)) if f.endswith(".png")] == []

        def on(sf):
            sf.draw_mosaic = True
            assert sf.mosaic_device is True
        drawn = tiles.run(path, 2, outdir=str(d), tag="drawn", setup=on)
    finally:
        os.chdir(cwd)
    return str(d), plain, drawn


def test_whole_run_with_draw_mosaic(runs):
    from caesar_mrcnn_amd import analyze
    d, plain, drawn = runs
    assert sorted(f for f in os.listdir(d) if f.endswith(".png")) == ["mosaic_mosaic.png"]
    assert len(drawn.sources["sources"]) >= 10 and drawn.sources == plain.sources
    for ext in ("json", "reg"):
        assert open(os.path.join(d, "cat_plain." + ext)).read() == open(os.path.join(d, "cat_drawn." + ext)).read()
    assert "render_mosaic_device" not in analyze.device_forms_failed
    assert "overview_ms" in drawn.mosaic_timing and "encode_ms" in drawn.mosaic_timing          # the device form drew it
    assert drawn._plane is None and drawn._plane_dev is None
    pixels, _ = draw_cases.png_pixels(open(os.path.join(d, "mosaic_mosaic.png"), "rb").read())
    assert np.array_equal(pixels, drawn.render_mosaic(False))


@pytest.mark.parametrize("shaded", [False, True])
@pytest.mark.parametrize("captions", ["name", "score", "none"])
def test_render_mosaic_device_equals_host(runs, shaded, captions):
    d, plain, sf = runs
    sf.mosaic_shaded, sf.mosaic_captions = shaded, captions
    try:
        want = sf.render_mosaic(False)
        sf._drop_plane()
        got = sf.render_mosaic(True)                                  # not resident: one upload
        assert sf._plane_dev is not None
        resident = sf._plane_dev[0]
        again = sf.render_mosaic(True)                                # resident: the same tensor is read
        assert sf._plane_dev[0] is resident
        assert got.shape == want.shape == (2 * (tiles.NY + 4), 2 * (tiles.NX + 4), 3)
        assert np.array_equal(got, want), int((got != want).sum())
        assert np.array_equal(again, want)
        assert np.array_equal(sf.render_mosaic(None), want)
    finally:
        sf.mosaic_shaded, sf.mosaic_captions = False, "name"
        sf._drop_plane()


def test_render_mosaic_device_other_shrinks_and_catalogues(runs, tmp_path):
    d, plain, sf = runs
    try:
        for k, scale in ((3, None), (5, 4)):
            sf.mosaic_shrink, sf.mosaic_scale = k, scale
            assert np.array_equal(sf.render_mosaic(True), sf.render_mosaic(False)), k
    finally:
        sf.mosaic_shrink = sf.mosaic_scale = None
        sf._drop_plane()
    rng = np.random.RandomState(3)
    plane = rng.normal(0, 1, cases.CATALOGUE_PLANE_SHAPE).astype(np.float32)
    cat = cases.sfinder_for(str(tmp_path / "cat.fits"), plane, cases.catalogue())
    cat.mosaic_shrink = 3
    assert np.array_equal(cat.render_mosaic(True), cat.render_mosaic(False))
    cat.sources = {"sources": []}                                    # an empty catalogue: the bare overview
    assert np.array_equal(cat.render_mosaic(True), cat.render_mosaic(False))


def test_catalogue_past_the_item_cap_goes_to_the_host_statement(tmp_path, caplog):
    from caesar_mrcnn_amd import analyze, draw
    plane = np.random.RandomState(5).normal(0, 1, (40, 120)).astype(np.float32)
    sources = [{"name": "S%d" % (i + 1), "class_name": "compact", "score": 0.9, "merged": False, "pixels": [[i // 120, i % 120]]}
               for i in range(draw.MAX_ITEMS + 1)]
    sf = cases.sfinder_for(str(tmp_path / "many.fits"), plane, sources)
    sf.mosaic_captions, sf.mosaic_scale = "none", 1
    assert sf.mosaic_device is True
    got = sf.render_mosaic(None)
    assert "render_mosaic_device" not in analyze.device_forms_failed              # a refusal, not a failure
    assert "scene_ms" in sf.mosaic_timing                                         # the host statement drew it
    blue = np.array(draw.colour8(draw.CLASS_COLOR_MAP["compact"]), np.uint8)
    assert got.shape == (44, 124, 3) and (got[2, 2:122] == blue).all()
