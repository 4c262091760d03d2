"""The batched, device-resident tile front end of the tiled source finder on the GPU: mrcnn_fits_tiles_to_rgb (many tiles of one
resident plane per launch) byte for byte against the host statement fits.read_fits and the single-tile kernel; MaskRCNN.detect
on device tensors; SFinder.tile_batch against the tile-at-a-time loop; run.py --tile_batch."""
import glob
import json
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

import sfinder_cases as cases
import sfinder_tiles_cases as tc

pytestmark = pytest.mark.gpu
ROOT = tc.ROOT

NY, NX = 200, 300
# (x0, y0, w, h), what the tile is there for
TILES = [
    ((0, 0, 64, 48), "offset (0, 0), width != NX"),
    ((37, 21, 50, 33), "non-zero offset"),
    ((5, 5, 32, 32), "exactly one 1024-pixel chunk"),
    ((60, 70, 25, 41), "1025 pixels: a second chunk of one pixel"),
    ((3, 60, 20, 31), "fewer pixels than the 1000 samples"),
    ((10, 100, 2, 2), "below min_npixels"),
    ((205, 15, 30, 30), "wholly inside the NaN block"),
    ((240, 140, 40, 30), "holds the -inf pixel and NaNs: the NaN fill is -inf"),
    ((40, 90, 30, 30), "holds the +inf pixel"),
    ((102, 122, 64, 64), "inside the constant region: range 0"),
    ((100, 20, 60, 50), "overlaps the next"),
    ((130, 40, 60, 50), "overlaps the previous"),
    ((255, 163, 45, 37), "touches the plane's last row and column"),
    ((180, 0, 50, 70), "partly NaN"),
]
CONTRASTS = ([0.25, 0.25, 0.25], [0.25, 0.3, 1.0])


def _counted(real, log, what=lambda *a, **k: a[0]):
    """`real`, with what(*args) appended to `log` at every call."""
    def f(*a, **k):
        log.append(what(*a, **k))
        return real(*a, **k)
    return f


def _plane():
    rng = np.random.RandomState(11)
    yy, xx = np.mgrid[0:NY, 0:NX]
    img = rng.normal(0.0, 1.0, (NY, NX)).astype(np.float32)
    for cy, cx, sy, sx, a in ((30, 40, 4, 6, 60), (80, 75, 3, 3, 150), (50, 140, 8, 5, 30), (180, 280, 5, 5, 90), (150, 260, 6, 4, 45),
                              (25, 120, 5, 7, 70), (100, 55, 4, 4, 25)):
        img += (a * np.exp(-0.5 * (((yy - cy) / sy) ** 2 + ((xx - cx) / sx) ** 2))).astype(np.float32)
    img[10:60, 200:260] = np.nan                  # NaN block
    img[148, 245:248] = np.nan
    img[100, 50] = np.inf
    img[150, 250] = -np.inf
    img[120:190, 100:170] = 3.5                   # constant region, 70 x 70
    return img


@pytest.fixture(scope="module")
def plane_file(tmp_path_factory):
    """(path, plane, {contrast index: [host image or None per tile]}): the host statement, computed once.  None: read_fits raises
    on that tile (a tile without a finite pixel: zscale_limits has no sample to index)."""
    from caesar_mrcnn_amd import fits
    path = str(tmp_path_factory.mktemp("fits_tiles") / "plane.fits")
    img = _plane()
    fits.write_fits(path, img)
    want = {}
    for k, zc in enumerate(CONTRASTS):
        want[k] = []
        for (x0, y0, w, h), _ in TILES:
            with warnings.catch_warnings(), np.errstate(all="ignore"):
                warnings.simplefilter("ignore")
                try:
                    want[k].append(fits.read_fits(path, x0, x0 + w, y0, y0 + h, zscale_contrasts=zc)[0])
                except IndexError:
                    want[k].append(None)
    return path, img, want


def _device_planes(path, dev):
    """The plane as the file stores it (big-endian bytes, uint8 [NY, NX, 4]) and as native float32."""
    import torch
    from caesar_mrcnn_amd import fits
    data, _ = fits.read_primary_hdu(path, native=False)
    assert data.dtype == np.dtype(">f4") and data.shape == (NY, NX)
    big = torch.from_numpy(np.array(data, order="C", copy=True).view(np.uint8).reshape(NY, NX, 4)).to(dev)
    native = torch.from_numpy(np.ascontiguousarray(data.astype(np.float32))).to(dev)
    return {True: big, False: native}


def test_tiles_equal_host_statement(dev, plane_file):
    """Every tile of the batch, alone (T = 1) and all in one call, equal and unequal contrasts, big-endian bytes as stored and the
    native plane: np.array_equal to fits.read_fits of that cut on the host and to ops.fits_to_rgb of the same cut; a second call
    gives the same bytes.  The tile wholly inside the NaN block has no host image -- fits.read_fits raises IndexError there
    (zscale_limits indexes an empty sample) -- so for it the single-tile kernel is the statement: all zeros."""
    import torch
    from caesar_mrcnn_amd import ops
    path, img, want = plane_file
    planes = _device_planes(path, dev)
    rects = [t for t, _ in TILES]
    n_host = 0
    for k, zc in enumerate(CONTRASTS):
        single = []
        for (x0, y0, w, h) in rects:                                 # the single-tile kernel on the same cut
            cut = torch.from_numpy(np.ascontiguousarray(img[y0:y0 + h, x0:x0 + w])).to(dev)
            single.append(ops.fits_to_rgb(cut, h, w, zc).cpu().numpy())
        for big in (True, False):
            outs = ops.fits_tiles_to_rgb(planes[big], rects, zc, big_endian=big)
            assert len(outs) == len(rects)
            base = outs[0].data_ptr()
            off = 0
            for o, (x0, y0, w, h) in zip(outs, rects):               # views into one pool, back to back
                assert o.dtype == torch.uint8 and tuple(o.shape) == (h, w, 3) and o.is_cuda and o.data_ptr() == base + off
                off += 3 * w * h
            got = [o.cpu().numpy() for o in outs]
            again = [o.cpu().numpy() for o in ops.fits_tiles_to_rgb(planes[big], rects, zc, big_endian=big)]
            for i, ((rect, why), g) in enumerate(zip(TILES, got)):
                tag = "%s %r zc=%s big_endian=%s" % (why, rect, zc, big)
                assert np.array_equal(g, again[i]), "second call differs: " + tag
                assert np.array_equal(g, single[i]), "differs from ops.fits_to_rgb: " + tag
                if want[k][i] is not None:
                    n_host += 1
                    diff = int((g != want[k][i]).sum())
                    assert diff == 0, "%s: %d of %d bytes differ from fits.read_fits" % (tag, diff, g.size)
                else:
                    assert "NaN block" in why and not g.any(), tag
                alone = ops.fits_tiles_to_rgb(planes[big], [rect], zc, big_endian=big)
                assert len(alone) == 1 and np.array_equal(alone[0].cpu().numpy(), g), "T = 1 differs: " + tag
    assert n_host == 2 * 2 * (len(TILES) - 1)
    # the cases are what they claim to be
    inside = lambda x0, y0, w, h, r, c: y0 <= r < y0 + h and x0 <= c < x0 + w
    assert inside(*rects[7], 150, 250) and inside(*rects[8], 100, 50) and np.isnan(img[15:45, 205:235]).all()
    assert len(np.unique(img[122:186, 102:166])) == 1 and 25 * 41 == 1025 and 20 * 31 < 1000
    assert want[0][9].max() == 0 and want[0][0].max() == 255


def test_bad_tiles_are_refused_without_a_write(dev, plane_file):
    """T = 0, empty or negative rectangles, rectangles that leave the plane and a tile above the size limit: refused by the
    argument check (ValueError / FitsTileUnsupported from ops; MRCNN_ERR_ARG / MRCNN_ERR_UNSUPPORTED from the C entry), and the
    output pool keeps its bytes.  The size limit is tested through the check alone: the 2049 x 2048 tile is only claimed."""
    import ctypes as C
    import torch
    from caesar_mrcnn_amd import _hip, ops
    path, img, _ = plane_file
    plane = _device_planes(path, dev)[False]
    bad = [[], [(0, 0, 0, 10)], [(0, 0, 10, -1)], [(-1, 0, 10, 10)], [(0, -1, 10, 10)], [(291, 0, 10, 10)], [(0, 191, 10, 10)],
           [(0, 0, 301, 10)], [(0, 0, 16, 16), (0, 0, 10, 201)]]
    for rects in bad:
        with pytest.raises(ValueError):
            ops.fits_tiles_to_rgb(plane, rects)
    with pytest.raises(ValueError):
        ops.fits_tiles_to_rgb(plane.view(-1), [(0, 0, 8, 8)])
    with pytest.raises(_hip.HipPathError):                                         # a column slice: rows are not NX apart
        ops.fits_tiles_to_rgb(plane[:, :100], [(0, 0, 8, 8)])
    huge = torch.empty((4096, 4096), dtype=torch.float32, device=dev)             # never read: the call is refused before a launch
    with pytest.raises(ops.FitsTileUnsupported):
        ops.fits_tiles_to_rgb(huge, [(0, 0, 16, 16), (0, 0, 2049, 2048)])
    del huge
    # the C entry itself, with a sentinel-filled pool
    L = _hip.lib()
    pool = torch.full((3 * 64 * 64,), 0xA5, dtype=torch.uint8, device=dev)
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device=dev)
    zc = (C.c_double * 3)(0.25, 0.25, 0.25)
    ok_table = ops.fits_tile_table([(0, 0, 16, 16)])
    table_dev = torch.from_numpy(ok_table.view(np.uint8)).to(dev)

    def call(table, T, ny=NY, nx=NX, layout_ok=False):
        host = table.ctypes.data_as(C.c_void_p) if table is not None else None
        assert (L.mrcnn_fits_tiles_workspace(host, T, ny, nx) > 0) == layout_ok == (L.mrcnn_fits_tiles_check(host, T, ny, nx) == 0)
        return L.mrcnn_fits_tiles_to_rgb(_hip.ptr(plane), 0, ny, nx, host, _hip.ptr(table_dev), T, zc, _hip.ptr(pool), pool.numel(),
                                         _hip.ptr(ws), ws.numel(), _hip.current_stream())
    assert call(ok_table, 0) == -1 and call(None, 1) == -1
    for rects in bad[1:]:
        assert call(ops.fits_tile_table(rects), len(rects)) == -1, rects
    shifted = ops.fits_tile_table([(0, 0, 16, 16)])
    shifted["pixel_offset"][0] = 5                                                   # a layout that is not back to back
    assert call(shifted, 1) == -1
    assert call(ops.fits_tile_table([(0, 0, 2049, 2048)]), 1, 4096, 4096) == -4      # 4098 chunks > 4096
    assert call(ops.fits_tile_table([(0, 0, 2048, 2048)]), 1, 4096, 4096, layout_ok=True) == -1      # within the limit; the pool is too small
    torch.cuda.synchronize()
    assert bool((pool == 0xA5).all())
    # and a good call into the same pool writes exactly its tile
    assert L.mrcnn_fits_tiles_workspace(ok_table.ctypes.data_as(C.c_void_p), 1, NY, NX) > 0
    rc = L.mrcnn_fits_tiles_to_rgb(_hip.ptr(plane), 0, NY, NX, ok_table.ctypes.data_as(C.c_void_p), _hip.ptr(table_dev), 1, zc, _hip.ptr(pool),
                                   pool.numel(), _hip.ptr(ws), ws.numel(), _hip.current_stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert bool((pool[3 * 256:] == 0xA5).all())
    assert np.array_equal(pool[:3 * 256].view(16, 16, 3).cpu().numpy(), ops.fits_tiles_to_rgb(plane, [(0, 0, 16, 16)])[0].cpu().numpy())


# ---- detect on device tensors --------------------------------------------------------------------------------
def test_detect_on_device_tensors(dev):
    """detect([t0, t1]) on uint8 device tensors = detect on the same bytes as host arrays (same batch size, same HIP-graph
    setting): rois, class ids, scores and masks value for value; the device masks are kept per slot.  A float tensor, a CPU tensor
    and a 2-D tensor raise ValueError instead of taking the host molding."""
    import torch
    from model_cases import _small_cfg, _weights
    from caesar_mrcnn_amd.model import MaskRCNN
    cfg = _small_cfg("custom", 128, mode="inference")
    cfg.IMAGES_PER_GPU = 2
    cfg.DETECTION_MIN_CONFIDENCE = 0.0
    assert cfg.BATCH_SIZE == 2
    model = MaskRCNN("inference", cfg, "/tmp/mrcnn_logs", device=dev, weights=_weights(cfg, 3))
    rng = np.random.RandomState(2)
    images = []
    for shape in ((128, 128, 3), (100, 90, 3)):
        im = rng.normal(40, 10, shape)
        im[30:60, 20:70] += 120
        im[70:90, 50:80] += 80
        images.append(np.clip(im, 0, 255).astype(np.uint8))
    host = model.detect(images)
    tensors = [torch.from_numpy(im).to(dev) for im in images]
    got = model.detect(tensors)
    assert len(model.last_masks_device) == 2
    assert sum(r["rois"].shape[0] for r in host) > 0
    for a, b, im in zip(host, got, images):
        assert b["masks"].shape[:2] == im.shape[:2]
        for key in ("rois", "class_ids", "scores", "masks"):
            assert a[key].dtype == b[key].dtype and np.array_equal(a[key], b[key]), key
    mixed = model.detect([tensors[0], images[1]])                     # a host array beside a device tensor
    for a, b in zip(host, mixed):
        assert all(np.array_equal(a[key], b[key]) for key in ("rois", "class_ids", "scores", "masks"))
    for bad in (tensors[0].float(), tensors[0].cpu(), tensors[0][:, :, 0], tensors[0].to(torch.int8)):
        with pytest.raises(ValueError):
            model.detect([tensors[1], bad])


# ---- SFinder ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mosaic_path(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("tiles_gpu") / "mosaic.fits")
    tc.write_mosaic(path)
    return path


@pytest.fixture(scope="module")
def baseline(mosaic_path, tmp_path_factory):
    out = {}
    for step in (1.0, 0.5):
        d = str(tmp_path_factory.mktemp("base"))
        sf = tc.run(mosaic_path, 0, step, outdir=d)
        out[step] = (sf, cases.canon(sf.sources["sources"]), open(sf.outfile_json).read(), open(sf.outfile_ds9).read())
    return out


@pytest.mark.parametrize("step", [1.0, 0.5])
@pytest.mark.parametrize("batch", [1, 3, 4])
def test_sfinder_batched_equals_tile_at_a_time(dev, mosaic_path, baseline, tmp_path, monkeypatch, batch, step):
    """The device front end (plane uploaded once, ops.fits_tiles_to_rgb per group, device tensors into detect) against the
    tile-at-a-time loop with the stub whose detections are a pure function of the tile's bytes: equal catalogue, JSON and region
    file at steps 1.0 (9 tiles; seed 4: 49 sources, 4 merged, 5 edge-flagged) and 0.5 (30 tiles: 35, 31, 33); batch 4 pads the
    last group at both.  The file is read once (fits.read_primary_hdu: 1 call), no tile takes the old path, and every image the
    model sees is a device tensor."""
    import torch
    from caesar_mrcnn_amd import fits
    from caesar_mrcnn_amd.sfinder import TileTask
    base_sf, base_canon, base_json, base_reg = baseline[step]
    src = base_sf.sources["sources"]
    assert sum(1 for s in src if s["merged"]) >= 1 and sum(1 for s in src if s["edge"]) >= 1
    ntiles = len(base_sf.tasks_per_worker[0])
    reads, singles, kinds = [], [], []
    monkeypatch.setattr(fits, "read_primary_hdu", _counted(fits.read_primary_hdu, reads))
    monkeypatch.setattr(TileTask, "find_sources", _counted(TileTask.find_sources, singles, lambda task: task.tid))

    class Model(tc.ThresholdModel):
        def detect(self, images, verbose=0):
            kinds.extend(torch.is_tensor(im) and im.is_cuda and im.dtype == torch.uint8 for im in images)
            return tc.ThresholdModel.detect(self, images, verbose)
    sf = tc.run(mosaic_path, batch, step, outdir=str(tmp_path), model=Model(tc.config(mosaic_path, step)))
    assert len(reads) == 1 and singles == []
    assert sf.model.batches == [batch] * (-(-ntiles // batch)) and all(kinds) and len(kinds) == batch * len(sf.model.batches)
    assert cases.canon(sf.sources["sources"]) == base_canon
    assert open(sf.outfile_json).read() == base_json
    assert open(sf.outfile_ds9).read() == base_reg
    assert sf._plane is None and sf._plane_dev is None


def test_sfinder_batched_shares_the_upload_with_source_params(dev, mosaic_path, monkeypatch):
    """compute_params on the device path after a batched run: the plane is uploaded once for both, read once, and the 24
    parameter keys of every source equal those of the tile_batch = 0 run."""
    from caesar_mrcnn_amd import fits
    from caesar_mrcnn_amd.sfinder import SFinder
    uploads, reads = [], []
    monkeypatch.setattr(SFinder, "_upload_plane", _counted(SFinder._upload_plane, uploads, lambda self, plane: tuple(plane.shape)))
    monkeypatch.setattr(fits, "read_primary_hdu", _counted(fits.read_primary_hdu, reads))

    def setup(sf):
        sf.compute_params, sf.params_device, sf.params_device_min_sources = True, True, 0
    runs = {}
    for batch in (0, 4):
        del uploads[:], reads[:]
        sf = tc.run(mosaic_path, batch, 1.0, setup=setup)
        assert sf.params_timing["device_sources"] > 0
        runs[batch] = (sf.sources["sources"], list(uploads), len(reads))
        assert sf._plane is None and sf._plane_dev is None
    assert runs[4][1] == [(tc.NY, tc.NX)] and runs[4][2] == 1
    assert runs[0][1] == [(tc.NY, tc.NX)] and runs[0][2] > 9
    assert len(runs[0][0]) == len(runs[4][0]) == 49
    for a, b in zip(runs[0][0], runs[4][0]):
        assert set(SFinder.PARAM_KEYS) <= set(b)
        assert {k: a[k] for k in SFinder.PARAM_KEYS} == {k: b[k] for k in SFinder.PARAM_KEYS}, a["name"]
    assert cases.canon(runs[0][0]) == cases.canon(runs[4][0])


# ---- command line ------------------------------------------------------------------------------------------------
def test_cli_tile_batch(dev, tmp_path):
    """run.py detect --split_img_in_tiles --merge_tile_sources --tile_batch 4 on the mosaic of test_cli_merge_tile_sources (custom
    backbone at 128, score threshold 0): exit 0, one out_mosaic.json with the catalogue's key set.  (The catalogue is not
    compared with the batch-1 run: a real network's results may differ between batch sizes in the last bits.)"""
    from caesar_mrcnn_amd import fits
    d = str(tmp_path)
    rng = np.random.RandomState(0)
    yy, xx = np.mgrid[0:256, 0:256]
    img = rng.normal(0, 1, (256, 256)).astype(np.float32)
    for cy, cx in ((128, 128), (60, 127), (200, 40), (128, 200)):            # blobs on the tile borders of a 2 x 2 grid
        img += 80 * np.exp(-0.5 * (((yy - cy) / 6.0) ** 2 + ((xx - cx) / 9.0) ** 2))
    fits.write_fits(os.path.join(d, "mosaic.fits"), img, {"BUNIT": "JY/BEAM"})
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "run.py"), "detect", "--imgsize", "128", "--backbone", "custom",
                        "--logs", os.path.join(d, "logs"), "--image", os.path.join(d, "mosaic.fits"), "--scoreThr", "0.0",
                        "--split_img_in_tiles", "--tile_xsize", "128", "--tile_ysize", "128", "--merge_tile_sources", "--tile_batch", "4"],
                       cwd=d, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=280)
    out = r.stdout.decode()
    assert r.returncode == 0, out[-3000:]
    assert "taking them one at a time" not in out and "tile_batch = 4 ignored" not in out, out[-3000:]
    assert glob.glob(os.path.join(d, "*.json")) == [os.path.join(d, "out_mosaic.json")]
    res = json.load(open(os.path.join(d, "out_mosaic.json")))
    assert res["image_id"] == "mosaic" and isinstance(res["objs"], list)
    keys = {"name", "x1", "x2", "y1", "y2", "class_id", "class_name", "score", "pixels", "vertexes", "edge", "merged"}
    for s in res["objs"]:
        assert set(s) == keys
    assert [s["name"] for s in res["objs"]] == ["S%d" % (i + 1) for i in range(len(res["objs"]))]
    assert "sources (" in out and "written to out_mosaic.json" in out
