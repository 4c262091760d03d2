"""The mosaic, the configuration and the stub model of the batched-tile tests of the tiled source finder.  Not a test module:
imported by test_sfinder_tiles_cpu.py and test_fits_tiles_gpu.py.

The stub answers every image with the 4-connected components of `image[..., 0] >= 200`, so its detections are a pure function
of the tile's bytes: two front ends that hand it the same bytes get the same catalogue, and one that differs in a single grey
level near the threshold does not."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SEED = 4
NY, NX, TILE = 384, 320, 128          # 320 is no multiple of the tile: the last column of tiles is 64 wide


def mosaic(seed=SEED):
    """[NY, NX] float32: unit noise, Gaussian blobs and a NaN strip that crosses a tile border.  One blob per 64 x 64 cell
    (jittered, so some straddle cell borders -- the tile borders at steps 1.0 and 0.5) plus four planted on the borders x = 128,
    256 / y = 128, 256 and the corner (128, 128).  A blob in every tile keeps the zscale range wide, so that no noise pixel
    reaches the stub's threshold and the catalogue stays small."""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:NY, 0:NX]
    img = rng.normal(0.0, 1.0, (NY, NX)).astype(np.float32)
    centres = [(128, 128), (60, 127), (200, 256), (256, 60)]
    centres += [(32 + 64 * gy + rng.randint(-20, 21), 32 + 64 * gx + rng.randint(-20, 21)) for gy in range(NY // 64) for gx in range(NX // 64)]
    for cy, cx in centres:
        sy, sx = rng.uniform(3.0, 7.0), rng.uniform(3.0, 7.0)
        img += np.float32(rng.uniform(40.0, 120.0)) * np.exp(-0.5 * (((yy - cy) / sy) ** 2 + ((xx - cx) / sx) ** 2)).astype(np.float32)
    img[90:96, 100:180] = np.nan
    return img


def write_mosaic(path, seed=SEED):
    from caesar_mrcnn_amd import fits
    img = mosaic(seed)
    fits.write_fits(path, img, {"BUNIT": "JY/BEAM", "CTYPE1": "RA---SIN", "CTYPE2": "DEC--SIN", "CRPIX1": 160.0, "CRPIX2": 192.0,
                                "CRVAL1": 254.0, "CRVAL2": -41.0, "CDELT1": -0.000277, "CDELT2": 0.000277, "BMAJ": 0.002,
                                "BMIN": 0.0015, "BPA": 10.0})
    return img


def config(path, step=1.0):
    """The run.py stretch flags (zscale, normalise, RGB, uint8, no bias / contrast stretch), 128 x 128 tiles."""
    from caesar_mrcnn_amd.config import SDetectorConfig
    cfg = SDetectorConfig()
    cfg.CLASS_NAMES, cfg.NUM_CLASSES = ["bkg", "source"], 2
    cfg.IMG_PATH = path
    cfg.SPLIT_IMG_IN_TILES = True
    cfg.TILE_XSIZE = cfg.TILE_YSIZE = TILE
    cfg.TILE_XSTEP = cfg.TILE_YSTEP = step
    cfg.ZSCALE_STRETCH = cfg.NORMALIZE_IMG = cfg.IMG_TO_RGB = cfg.IMG_TO_UINT8 = True
    cfg.BIAS_CONTRAST_STRETCH = False
    cfg.ZSCALE_CONTRASTS = [0.25, 0.25, 0.25]
    cfg.SCORE_THR, cfg.IOU_THR = 0.7, 0.6
    cfg.IMG_XMIN = cfg.IMG_XMAX = cfg.IMG_YMIN = cfg.IMG_YMAX = -1
    return cfg


class ThresholdModel(object):
    """Stand-in for MaskRCNN: host arrays or device tensors, any batch length; records the batch lengths it was given."""

    def __init__(self, config):
        self.config = config
        self.batches = []

    def detect(self, images, verbose=0):
        from caesar_mrcnn_amd import analyze, utils
        self.batches.append(len(images))
        out = []
        for image in images:
            image = image.cpu().numpy() if hasattr(image, "cpu") else np.asarray(image)
            labels, n = analyze.label_components((image[..., 0] >= 200).astype(np.uint8))
            masks = np.stack([labels == k for k in range(1, n + 1)], axis=-1) if n else np.zeros(image.shape[:2] + (0,), bool)
            out.append({"rois": utils.extract_bboxes(masks), "class_ids": np.ones(n, np.int32),
                        "scores": np.full(n, 0.99, np.float32), "masks": masks})
        return out


def run(path, tile_batch, step=1.0, outdir=None, model=None, setup=None, tag=None):
    """One SFinder.run_parallel on the host merge path; returns the SFinder.  `setup(sf)` runs before it."""
    from caesar_mrcnn_amd.sfinder import SFinder
    cfg = config(path, step)
    sf = SFinder(model or ThresholdModel(cfg), cfg)
    sf.merge_device = False
    sf.params_device = False
    sf.tile_batch = tile_batch
    tag = tag or ("b%d" % tile_batch)
    if outdir is None:
        sf.write_to_json = sf.write_to_ds9 = False
    else:
        sf.outfile_json = os.path.join(outdir, "cat_%s.json" % tag)
        sf.outfile_ds9 = os.path.join(outdir, "cat_%s.reg" % tag)
    if setup:
        setup(sf)
    assert sf.run_parallel() == 0
    return sf


def host_prepare(sf):
    """The seam's "prepare" step on the host: fits.read_fits per tile (what the device chain must reproduce)."""
    from caesar_mrcnn_amd import fits

    def prepare(tasks):
        cfg = sf.config
        return [fits.read_fits(cfg.IMG_PATH, t.ix_min, t.ix_max, t.iy_min, t.iy_max, zscale_contrasts=cfg.ZSCALE_CONTRASTS)[0] for t in tasks]
    return prepare
