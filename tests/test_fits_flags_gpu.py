"""The device chain for every read_fits flag combination (ops.fits_to_image, ops.fits_tiles_to_image) against the host branch of
fits.read_fits: uint8 byte for byte, float32 bit for bit, no pixel left out; read_fits(device=) and SFinder's batched front end
with flags other than the run.py ones."""
import itertools
import logging
import warnings

import numpy as np
import pytest

import sfinder_cases as cases

pytestmark = pytest.mark.gpu

# (h, w): 1 pixel; fewer pixels than a lane's four; one short of a 1024-pixel statistics chunk, exactly one, one over; five
# chunks with the last partial (4160 pixels -- a multiple of four, so 63 x 65 = 4095 stands beside it: a partial last group)
SHAPES = [(1, 1), (1, 7), (31, 33), (32, 32), (25, 41), (64, 65), (63, 65)]
CONTRASTS = [(0.25, 0.25, 0.25), (0.1, 0.25, 0.6)]
BIAS_CONTRAST = [(0.5, 1), (0.2, 3.5), (-1, 0.5), (2, 1), (0.5, 0), (0.5, -2)]


def _noise_tile(h, w, seed):
    """Unit noise around zero (negative values in half the pixels), a few bright blobs, about 3 % NaN."""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    img = rng.normal(0.0, 1.0, (h, w)).astype(np.float32)
    for _ in range(3):
        cy, cx, s, a = rng.uniform(0, h), rng.uniform(0, w), rng.uniform(1.5, 4.0), rng.uniform(20.0, 90.0)
        img += (a * np.exp(-0.5 * (((yy - cy) / s) ** 2 + ((xx - cx) / s) ** 2))).astype(np.float32)
    if h * w > 4:
        img[rng.uniform(size=img.shape) < 0.03] = np.nan
    return img


def _tiles():
    out = [("noise %dx%d" % s, _noise_tile(s[0], s[1], 100 + k)) for k, s in enumerate(SHAPES)]
    out.append(("constant", np.full((9, 7), 3.5, np.float32)))
    out.append(("all NaN", np.full((5, 6), np.nan, np.float32)))
    return out


def _configs(out_kind):
    """(zscale, biascontrast, normalize, zscale_contrasts, bias, contrast) of every accepted combination with this out_kind; the
    contrast triples vary only under zscale and the (bias, contrast) pairs only under the bias / contrast stretch."""
    for zscale, bc, normalize in itertools.product((False, True), repeat=3):
        if out_kind == 0 and not zscale and not bc:
            continue
        for zc in (CONTRASTS if zscale else CONTRASTS[:1]):
            for bias, contrast in (BIAS_CONTRAST if bc else BIAS_CONTRAST[:1]):
                yield zscale, bc, normalize, zc, bias, contrast


def _chain(zscale, bc, normalize, out_kind, zc, bias, contrast):
    """The descriptor itself: what the kernels compute is tested here for every combination they take, whichever of them
    fits.device_chain sends to the device."""
    from caesar_mrcnn_amd import fits
    return fits.DeviceChain(zscale, bc, normalize, out_kind, tuple(zc), float(bias), float(contrast))


def _host(path, zscale, bc, normalize, out_kind, zc, bias, contrast, **cut):
    from caesar_mrcnn_amd import fits
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        return fits.read_fits(path, stretch=zscale, normalize=normalize, convertToRGB=out_kind != 2, to_uint8=out_kind == 0,
                              stretch_biascontrast=bc, zscale_contrasts=list(zc), contrast=contrast, bias=bias, **cut)[0]


def _same(got, want):
    """Shape, dtype and every bit."""
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    if got.dtype == np.float32:
        return np.array_equal(got.view(np.uint32), want.view(np.uint32))
    return np.array_equal(got, want)


@pytest.fixture(scope="module")
def tile_files(tmp_path_factory):
    """[(name, array, path of its FITS file)]"""
    from caesar_mrcnn_amd import fits
    d = tmp_path_factory.mktemp("fits_flags")
    out = []
    for k, (name, img) in enumerate(_tiles()):
        path = str(d / ("tile%d.fits" % k))
        fits.write_fits(path, img)
        out.append((name, img, path))
    return out


def _raw(img, big, dev):
    import torch
    if big:
        return torch.from_numpy(np.ascontiguousarray(img.astype(">f4")).view(np.uint8).reshape(-1).copy()).to(dev)
    return torch.from_numpy(np.ascontiguousarray(img)).to(dev)


@pytest.mark.parametrize("out_kind", [0, 1, 2])
def test_every_accepted_combination_equals_the_host(dev, tile_files, out_kind):
    """ops.fits_to_image against the host branch of read_fits on the same tile, native float32 and big-endian bytes: every
    accepted (zscale, biascontrast, normalize) with this out_kind, two contrast triples, six (bias, contrast) pairs, the seven
    noise tiles and the constant tile -- same shape and dtype, uint8 byte for byte, float32 bit for bit (NaNs of 0 / 0 included).
    The tile of NaNs alone is held to the stated rule, not to the host (which raises under zscale): zeros for uint8, NaN for the
    float outputs."""
    from caesar_mrcnn_amd import ops
    configs = list(_configs(out_kind))
    assert len(configs) == {0: 2 * (12 + 2 + 6), 1: 2 * (12 + 2 + 6 + 1), 2: 2 * (12 + 2 + 6 + 1)}[out_kind]
    n = 0
    for name, img, path in tile_files:
        h, w = img.shape
        raws = {big: _raw(img, big, dev) for big in (False, True)}
        for cfg in configs:
            zscale, bc, normalize, zc, bias, contrast = cfg
            chain = _chain(zscale, bc, normalize, out_kind, zc, bias, contrast)
            want = None if name == "all NaN" else _host(path, zscale, bc, normalize, out_kind, zc, bias, contrast)
            for big in (False, True):
                got = ops.fits_to_image(raws[big], h, w, chain, big_endian=big).cpu().numpy()
                tag = "%s %r out_kind=%d big_endian=%s" % (name, cfg, out_kind, big)
                assert got.shape == ((h, w, 3) if out_kind != 2 else (h, w)), tag
                assert got.dtype == (np.uint8 if out_kind == 0 else np.float32), tag
                if want is None:
                    assert (not got.any()) if out_kind == 0 else np.isnan(got).all(), tag
                else:
                    if not _same(got, want):
                        a, b = (got.view(np.uint32), want.view(np.uint32)) if out_kind else (got, want)
                        bad = np.argwhere(a != b)
                        raise AssertionError("%s: %d of %d values differ from read_fits; first at %s: got %r, host %r" % (
                            tag, len(bad), got.size, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])]))
                n += 1
    assert n == len(tile_files) * len(configs) * 2
    # the data are what they claim to be
    for name, img, _ in tile_files[2:len(SHAPES)]:
        assert (img < 0).any() and np.isnan(img).any() and 0.01 < np.isnan(img).mean() < 0.06, name
    assert [im.size for _, im, _ in tile_files[2:7]] == [1023, 1024, 1025, 4160, 4095]


TILED_PLANE = (96, 130)
TILED_RECTS = [(0, 0, 41, 31), (20, 10, 33, 31), (50, 40, 1, 1), (100, 66, 30, 30), (5, 50, 64, 33)]     # (x0, y0, w, h)
TILED_CONFIGS = [(True, True, True, 0, (0.1, 0.25, 0.6), 0.2, 3.5), (False, True, False, 1, (0.25, 0.25, 0.25), 0.5, -2),
                 (True, False, False, 2, (0.1, 0.25, 0.6), 0.5, 1)]


def test_tiled_entry_equals_the_single_tile_entry(dev):
    """ops.fits_tiles_to_image on a 96 x 130 plane with five rectangles -- overlapping, of different sizes, one of 1 x 1, one that
    touches the plane's last row and column; their pool offsets (0, 1271, 2294, 2295, 3195) start tiles at three of the four
    positions of a lane's four-pixel group -- for three combinations and both byte orders: each tile equals fits_to_image of that cut."""
    import torch
    from caesar_mrcnn_amd import ops
    ny, nx = TILED_PLANE
    img = _noise_tile(ny, nx, 7)
    planes = {False: torch.from_numpy(img).to(dev),
              True: torch.from_numpy(np.ascontiguousarray(img.astype(">f4")).view(np.uint8).reshape(ny, nx, 4).copy()).to(dev)}
    assert TILED_RECTS[3][0] + TILED_RECTS[3][2] == nx and TILED_RECTS[3][1] + TILED_RECTS[3][3] == ny
    offsets = np.cumsum([0] + [w * h for _, _, w, h in TILED_RECTS[:-1]])
    assert [int(o) for o in offsets] == [0, 1271, 2294, 2295, 3195] and len(set(int(o) & 3 for o in offsets)) == 3
    for cfg in TILED_CONFIGS:
        chain = _chain(*cfg)
        for big in (False, True):
            outs = ops.fits_tiles_to_image(planes[big], TILED_RECTS, chain, big_endian=big)
            assert len(outs) == len(TILED_RECTS)
            for o, (x0, y0, w, h) in zip(outs, TILED_RECTS):
                cut = np.ascontiguousarray(img[y0:y0 + h, x0:x0 + w])
                single = ops.fits_to_image(torch.from_numpy(cut).to(dev), h, w, chain).cpu().numpy()
                assert o.is_cuda and _same(o.cpu().numpy(), single), (cfg, big, (x0, y0, w, h))


def test_unaligned_output_takes_the_scalar_path_to_the_same_bytes(dev, tile_files):
    """out= a contiguous view one element (1 byte for uint8, 4 bytes for float32) into a sentinel-filled buffer: its base is not
    16-byte aligned, so every group of the pixel pass stores pixel by pixel.  The run.py stretch flags, both contrast triples, the
    three output kinds, tiles of 7, 1025 and 4160 pixels: the image equals the aligned call bit for bit and the host read_fits, and
    the sentinel elements on either side of the view keep their value."""
    import torch
    from caesar_mrcnn_amd import ops
    picked = [tile_files[k] for k in (1, 4, 5)]
    assert [im.shape for _, im, _ in picked] == [(1, 7), (25, 41), (64, 65)]
    n = 0
    for name, img, path in picked:
        h, w = img.shape
        raw = _raw(img, False, dev)
        for zc, out_kind in itertools.product(CONTRASTS, (0, 1, 2)):
            chain = _chain(True, False, True, out_kind, zc, 0.5, 1)
            dtype, sentinel = (torch.uint8, 0xA5) if out_kind == 0 else (torch.float32, -12345.5)
            shape = (h, w) if out_kind == 2 else (h, w, 3)
            count = int(np.prod(shape))
            buf = torch.full((count + 2,), sentinel, dtype=dtype, device=dev)
            view = buf[1:1 + count].view(shape)
            assert buf.data_ptr() % 16 == 0 and view.data_ptr() % 16 != 0 and view.is_contiguous()
            got = ops.fits_to_image(raw, h, w, chain, out=view)
            assert got is view
            aligned = ops.fits_to_image(raw, h, w, chain)
            assert aligned.data_ptr() % 16 == 0
            tag = "%s %r out_kind=%d" % (name, zc, out_kind)
            assert _same(got.cpu().numpy(), aligned.cpu().numpy()), tag
            assert _same(got.cpu().numpy(), _host(path, True, False, True, out_kind, zc, 0.5, 1)), tag
            ends = buf[[0, count + 1]].cpu().numpy()
            assert ends[0] == sentinel and ends[1] == sentinel, tag
            n += 1
    assert n == 3 * 2 * 3


def test_unaligned_pool_through_the_rgb_entry_takes_the_scalar_path_to_the_same_bytes(dev):
    """The C entry mrcnn_fits_tiles_to_rgb with `rgb` one byte into a sentinel pool, the five rectangles of the 96 x 130 plane, both
    contrast triples: every tile equals ops.fits_tiles_to_rgb of the same rectangles (an aligned pool), the byte before the pool
    and the bytes after it stay sentinel."""
    import ctypes as C
    import torch
    from caesar_mrcnn_amd import _hip, ops
    ny, nx = TILED_PLANE
    plane = torch.from_numpy(_noise_tile(ny, nx, 7)).to(dev)
    table = ops.fits_tile_table(TILED_RECTS)
    host = table.ctypes.data_as(C.c_void_p)
    table_dev = torch.from_numpy(table.view(np.uint8)).to(dev)
    total = sum(w * h for _, _, w, h in TILED_RECTS)
    L = _hip.lib()
    nbytes = L.mrcnn_fits_tiles_workspace(host, len(TILED_RECTS), ny, nx)
    assert nbytes > 0
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
    for zc in CONTRASTS:
        want = ops.fits_tiles_to_rgb(plane, TILED_RECTS, zc)
        pool = torch.full((1 + 3 * total + 16,), 0xA5, dtype=torch.uint8, device=dev)
        assert pool.data_ptr() % 16 == 0 and ws.data_ptr() % 16 == 0
        rc = L.mrcnn_fits_tiles_to_rgb(_hip.ptr(plane), 0, ny, nx, host, _hip.ptr(table_dev), len(TILED_RECTS), (C.c_double * 3)(*zc),
                                       C.c_void_p(pool.data_ptr() + 1), 3 * total, _hip.ptr(ws), ws.numel(), _hip.current_stream())
        assert rc == 0
        torch.cuda.synchronize()
        got = pool.cpu().numpy()
        assert got[0] == 0xA5 and (got[1 + 3 * total:] == 0xA5).all(), zc
        for t, (o, (x0, y0, w, h)) in enumerate(zip(want, TILED_RECTS)):
            at = 1 + 3 * int(table["pixel_offset"][t])
            assert np.array_equal(got[at:at + 3 * w * h].reshape(h, w, 3), o.cpu().numpy()), (zc, (x0, y0, w, h))


def _spy(real, log):
    def f(*a, **k):
        log.append(a)
        return real(*a, **k)
    return f


def test_read_fits_takes_the_device_for_other_flags(dev, tile_files, monkeypatch):
    """read_fits(device=) with stretch_biascontrast=True, and with to_uint8=False: the host path's array, and ops.fits_to_image
    ran (before this entry existed the call took the host branch without a word).  With the run.py flags the same entry runs,
    once, with that chain, and not through ops.fits_to_rgb; device_out keeps a device tensor for the uint8 RGB image alone."""
    import torch
    from caesar_mrcnn_amd import fits, ops
    name, img, path = tile_files[5]
    assert name == "noise 64x65"
    new, old = [], []
    monkeypatch.setattr(ops, "fits_to_image", _spy(ops.fits_to_image, new))
    monkeypatch.setattr(ops, "fits_to_rgb", _spy(ops.fits_to_rgb, old))
    for kw in (dict(stretch_biascontrast=True, bias=0.2, contrast=3.5), dict(to_uint8=False), dict(convertToRGB=False, normalize=False),
               dict(stretch=False, stretch_biascontrast=True, bias=0.5, contrast=-2, to_uint8=False)):
        del new[:], old[:]
        with warnings.catch_warnings(), np.errstate(all="ignore"):
            warnings.simplefilter("ignore")
            want = fits.read_fits(path, **kw)[0]
            assert new == [] and old == []
            got = fits.read_fits(path, device=dev, **kw)[0]
        assert len(new) == 1 and old == [], kw
        assert isinstance(got, np.ndarray) and _same(got, want), kw
        kept = fits.read_fits(path, device=dev, device_out=True, **kw)[0]
        if want.dtype == np.uint8:
            assert torch.is_tensor(kept) and kept.is_cuda and kept.dtype == torch.uint8 and np.array_equal(kept.cpu().numpy(), want)
        else:
            assert isinstance(kept, np.ndarray) and _same(kept, want), kw
    # a cut of the file, as the tiled source finder reads it
    del new[:], old[:]
    cut = dict(xmin=3, xmax=50, ymin=10, ymax=41)
    want = fits.read_fits(path, stretch_biascontrast=True, **cut)[0]
    got = fits.read_fits(path, stretch_biascontrast=True, device=dev, **cut)[0]
    assert len(new) == 1 and got.shape == (31, 47, 3) and _same(got, want)
    # the run.py flags: the same entry, with their chain
    del new[:], old[:]
    want = fits.read_fits(path)[0]
    got = fits.read_fits(path, device=dev)[0]
    assert len(new) == 1 and old == [] and _same(got, want)
    chain = new[0][3]
    assert (bool(chain.zscale), bool(chain.biascontrast), bool(chain.normalize), chain.out_kind) == (True, False, True, 0)
    # the refused combination stays on the host
    del new[:], old[:]
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        got = fits.read_fits(path, stretch=False, device=dev)[0]
    assert new == [] and old == [] and got.dtype == np.uint8
    # and so does a chain of a few operations per pixel on a tile this small (fits.DEVICE_LIGHT_CHAIN_MIN_PIXELS)
    got = fits.read_fits(path, stretch=False, convertToRGB=False, device=dev)[0]
    assert new == [] and old == [] and _same(got, fits.read_fits(path, stretch=False, convertToRGB=False)[0])


class _BatchLabelMapModel(cases.LabelMapModel):
    """LabelMapModel for any batch length, host arrays or device tensors."""

    def detect(self, images, verbose=0):
        out = []
        for image in images:
            image = image.cpu().numpy() if hasattr(image, "cpu") else np.asarray(image)
            out.extend(cases.LabelMapModel.detect(self, [image], verbose))
        return out


def test_sfinder_batches_tiles_under_the_bias_contrast_stretch(dev, tmp_path, caplog):
    """The planted label mosaic with BIAS_CONTRAST_STRETCH on (bias 25, contrast 0.02: sky -> 0, label k -> 0.02 k, so the labels
    stay distinct grey levels), no zscale, uint8 RGB: tile_batch = 4 takes the batched front end (groups prepared on the device,
    no "ignored" log line) and its catalogue equals the tile-at-a-time loop's."""
    import torch
    from caesar_mrcnn_amd import fits
    from caesar_mrcnn_amd.sfinder import SFinder
    labels, n = cases.planted_mosaic(3, nx=512, ny=256, n_try=80)          # two 256-tiles
    assert 5 <= n <= 45
    path = str(tmp_path / "labels.fits")
    fits.write_fits(path, labels.astype(np.float32))
    runs = {}
    for batch in (0, 4):
        cfg = cases.label_map_config(path)
        cfg.IMG_TO_RGB = cfg.IMG_TO_UINT8 = cfg.BIAS_CONTRAST_STRETCH = True
        cfg.IMG_BIAS, cfg.IMG_CONTRAST = 25.0, 0.02
        sf = SFinder(_BatchLabelMapModel(cfg), cfg)
        sf.merge_device = False
        sf.write_to_json = sf.write_to_ds9 = False
        sf.tile_batch = batch
        groups = []
        real = sf.prepare_tile_images

        def prepare(tasks, real=real, groups=groups):
            images = real(tasks)
            groups.append(([t.tid for t in tasks], all(torch.is_tensor(im) and im.is_cuda and im.dtype == torch.uint8 for im in images)))
            return images
        sf.prepare_tile_images = prepare
        with caplog.at_level(logging.INFO, logger="mrcnn"):
            caplog.clear()
            assert sf.run_parallel() == 0
            said = [r.getMessage() for r in caplog.records if "tile_batch" in r.getMessage()]
        runs[batch] = (cases.canon(sf.sources["sources"]), groups, said, len(sf.sources["sources"]))
    assert runs[0][1] == [] and runs[4][1] == [([0, 1], True)]
    assert runs[4][2] == [] and runs[0][2] == []
    assert runs[4][0] == runs[0][0] and runs[0][3] == n


def test_refusals_launch_nothing(dev):
    """uint8 output with neither stretch: the package's unsupported error (MRCNN_ERR_UNSUPPORTED from the C check); a tile above
    2048 x 2048 pixels: refused by the layout check -- the check function alone is called, nothing is allocated."""
    import ctypes as C
    import torch
    from caesar_mrcnn_amd import _hip, fits, ops
    bad = fits.DeviceChain(False, False, True, 0, (0.25, 0.25, 0.25), 0.5, 1.0)
    raw = torch.zeros(16, dtype=torch.float32, device=dev)
    out = torch.full((4, 4, 3), 0xA5, dtype=torch.uint8, device=dev)
    with pytest.raises(ops.FitsChainUnsupported):
        ops.fits_to_image(raw, 4, 4, bad, out=out)
    with pytest.raises(ops.FitsChainUnsupported):
        ops.fits_tiles_to_image(raw.view(4, 4), [(0, 0, 2, 2)], bad)
    assert issubclass(ops.FitsChainUnsupported, _hip.HipPathError)
    torch.cuda.synchronize()
    assert bool((out == 0xA5).all())
    L = _hip.lib()
    ok = _hip.FitsChain(1, 1, 1, 0, (C.c_double * 3)(0.25, 0.25, 0.25), 0.5, 1.0)
    assert L.mrcnn_fits_image_check(C.byref(ok), 2048, 2048) == 0
    assert L.mrcnn_fits_image_check(C.byref(ok), 2049, 2048) == ops.ERR_UNSUPPORTED
    assert L.mrcnn_fits_image_check(C.byref(ok), 0, 8) == -1
    neither = _hip.FitsChain(0, 0, 1, 0, (C.c_double * 3)(0.25, 0.25, 0.25), 0.5, 1.0)
    assert L.mrcnn_fits_image_check(C.byref(neither), 8, 8) == ops.ERR_UNSUPPORTED
    for kind in (1, 2):
        neither.out_kind = kind
        assert L.mrcnn_fits_image_check(C.byref(neither), 8, 8) == 0
    neither.out_kind = 3
    assert L.mrcnn_fits_image_check(C.byref(neither), 8, 8) == -1
