"""Tiled source finding: cut a mosaic into tiles, detect per tile, stitch the sources that straddle tile borders back
together and write one catalogue.  Restates ``TileTask`` and ``SFinder`` of mrcnn/sfinder.py for the path scripts/run.py
uses (create_tile_tasks :1216, find_sources_at_edge :643, merge_edge_sources :711, run_parallel :549), rule by rule, quirks
included (each carries the reference line).  The merge has two implementations behind ``SFinder.merge_device``:

  * ``merge_edge_sources_host``    the literal statement in Python / NumPy -- the CPU-testable statement and the yardstick of
                                   the kernels;
  * ``merge_edge_sources_device``  the pixel-pair test and the pixel union on bit masks on the GPU (csrc/tilemerge.hip through
                                   ops.tile_adjacency / ops.tile_union); candidate pairs, the component search, contours and
                                   JSON stay on the host.

Both give equal catalogues (tests/test_sfinder_gpu.py).  Ranks are RANK / WORLD_SIZE processes (no mpi4py): tiles go round
robin over the ranks, the per-tile result dicts are gathered on rank 0 with torch.distributed.gather_object, rank 0 merges
and writes.

The step between merging and saving, compute_source_params (:613-622, :994-1211: pixel count, flux statistics, centroids, sky
positions per source), runs when ``SFinder.compute_params`` is set (run.py --compute_source_params; the reference always runs
it).  It has two implementations as well, behind ``SFinder.params_device``:

  * ``compute_source_params``      the per-source statement in NumPy, rule by rule;
  * ``compute_sources_params``     all sources at once: the image plane uploaded once, the masked reductions and the clipping
                                   loop in one launch (csrc/srcparams.hip through ops.source_params), every ratio and the dicts
                                   formed by the host code that also finishes the per-source statement.

The front of a tiled run -- read the tile, stretch it, detect -- has a batched form behind ``SFinder.tile_batch`` (default 0:
the per-tile loop of the reference; run.py --tile_batch N): the mosaic plane is read and uploaded once, the tiles of a group of
N are cut and stretched on the GPU in one ops.fits_tiles_to_image call and go to ONE model.detect call as device tensors
(``prepare_tile_images`` / ``_detect_images``); every tile's Analyzer then takes its own result (TileTask.accept_detection).

astropy.stats.sigma_clipped_stats and astropy.wcs.WCS are restated in fits.py (sigma_clipped_stats, SimpleWCS), unpinned;
cv.moments is its defining sums.  Not restated: plots.
"""
import logging
import os
import time

import numpy as np

from . import analyze
from . import fits
from .analyze import Analyzer

logger = logging.getLogger("mrcnn")


class MergedSourceInfo(object):
    """Helper of merge_edge_sources (sfinder.py:44-49): source index within its tile entry, index of the tile entry."""

    def __init__(self, sindex, tindex):
        self.sindex = sindex
        self.tindex = tindex


# ===============================
#        TileTask
# ===============================
class TileTask(object):
    """One tile of the mosaic (sfinder.py:54-259)."""

    def __init__(self, tile_coords, model, config):
        self.model = model
        self.config = config
        self.coords = tile_coords
        self.ix_min, self.ix_max, self.iy_min, self.iy_max = tile_coords[0], tile_coords[1], tile_coords[2], tile_coords[3]
        self.wid = -1
        self.tid = 0
        self.sname_tag = ""
        self.neighborTaskId = []
        self.neighborTaskIndex = []
        self.neighborWorkerId = []
        self.imgdata = None
        self.imgheader = None
        self.image_id = os.path.splitext(os.path.basename(os.path.abspath(self.config.IMG_PATH)))[0]
        self.det_sources = {}
        self.bboxes_det = self.scores_det = self.classid_det = self.masks_det = None
        self.save_json = False
        self.save_regions = False
        self.results_device = False       # handed to the Analyzer (SFinder.results_device)
        self.components_device = False    # likewise (SFinder.components_device)
        self.procId = 0

    def set_worker_id(self, wid):
        self.wid = wid

    def set_task_id(self, tid):
        self.tid = tid
        self.sname_tag = "t" + str(tid)

    def is_task_tile_adjacent(self, aTask):
        # sfinder.py:127-129: "adjacent" = touching in x AND in y, where an identical span counts as touching
        ax = (self.ix_max == aTask.ix_min - 1 or self.ix_min == aTask.ix_max + 1 or
              (self.ix_min == aTask.ix_min and self.ix_max == aTask.ix_max))
        ay = (self.iy_max == aTask.iy_min - 1 or self.iy_min == aTask.iy_max + 1 or
              (self.iy_min == aTask.iy_min and self.iy_max == aTask.iy_max))
        return ax and ay

    def is_task_tile_overlapping(self, aTask):
        # sfinder.py:141-150: strict tests on inclusive-looking corners; tiles that only share their border column overlap
        if self.ix_max < aTask.ix_min or self.ix_min > aTask.ix_max:
            return False
        if self.iy_max < aTask.iy_min or self.iy_min > aTask.iy_max:
            return False
        return True

    def is_task_tile_neighbor(self, aTask):
        return self.is_task_tile_adjacent(aTask) or self.is_task_tile_overlapping(aTask)      # sfinder.py:153-159

    def add_neighbor_info(self, tid, tindex, wid):
        self.neighborTaskId.append(tid)
        self.neighborTaskIndex.append(tindex)
        self.neighborWorkerId.append(wid)

    def find_sources(self):
        """Read the tile and run the Analyzer on it (sfinder.py:169-259); fills det_sources.  0 / -1."""
        cfg = self.config
        self.bboxes_det = self.scores_det = self.classid_det = self.masks_det = None
        res = fits.read_fits(cfg.IMG_PATH, self.ix_min, self.ix_max, self.iy_min, self.iy_max, stretch=cfg.ZSCALE_STRETCH,
                             zscale_contrasts=cfg.ZSCALE_CONTRASTS, normalize=cfg.NORMALIZE_IMG, convertToRGB=cfg.IMG_TO_RGB,
                             to_uint8=cfg.IMG_TO_UINT8, stretch_biascontrast=cfg.BIAS_CONTRAST_STRETCH, bias=cfg.IMG_BIAS,
                             contrast=cfg.IMG_CONTRAST)
        if res is None:
            logger.warning("[PROC %d] Failed to read tile image for task %d!" % (self.procId, self.tid))
            return -1
        self.imgdata, self.imgheader = res
        analyzer = self._analyzer()
        if analyzer.predict(self.imgdata, self.image_id, header=self.imgheader, xmin=self.ix_min, ymin=self.iy_min) < 0:
            logger.error("[PROC %d] Failed to run model prediction on tile image for task %d!" % (self.procId, self.tid))
            return -1
        return self._take(analyzer)

    def accept_detection(self, image_shape, header, r, masks_device=None):
        """find_sources for a tile whose image was made and detected elsewhere (SFinder's batched front end): `r` is the tile's
        entry of model.detect's result, `masks_device` the device tensor behind r['masks'] (or None).  The image itself is not
        needed -- only its shape is."""
        self.bboxes_det = self.scores_det = self.classid_det = self.masks_det = None
        self.imgdata, self.imgheader = None, header
        analyzer = self._analyzer()
        if analyzer.accept_detection(tuple(image_shape), r, masks_device, self.image_id, header=header, xmin=self.ix_min,
                                     ymin=self.iy_min) < 0:
            logger.error("[PROC %d] Failed to run model prediction on tile image for task %d!" % (self.procId, self.tid))
            return -1
        return self._take(analyzer)

    def _analyzer(self):
        cfg = self.config
        analyzer = Analyzer(self.model, cfg)
        analyzer.draw = False
        analyzer.iou_thr, analyzer.score_thr = cfg.IOU_THR, cfg.SCORE_THR
        analyzer.write_to_json = self.save_json
        analyzer.outfile_json = 'catalog_' + self.image_id + '_tid' + str(self.tid) + '.json'
        analyzer.write_to_ds9 = self.save_regions
        analyzer.outfile_ds9 = 'catalog_' + self.image_id + '_tid' + str(self.tid) + '.reg'
        analyzer.obj_name_tag = self.sname_tag
        analyzer.results_device = self.results_device
        analyzer.components_device = self.components_device
        return analyzer

    def _take(self, analyzer):
        """The Analyzer's results + the tile info (sfinder.py:221-259)."""
        if not analyzer.bboxes:                                   # sfinder.py:221-224: det_sources stays empty
            logger.info("[PROC %d] No object detected in tile image for task %d ..." % (self.procId, self.tid))
            return 0
        self.bboxes_det, self.scores_det = analyzer.bboxes, analyzer.scores_final
        self.classid_det, self.masks_det = analyzer.class_ids_final, analyzer.masks_final
        self.det_sources = analyzer.results
        self.det_sources["workerId"] = self.wid
        self.det_sources["tileId"] = self.tid
        self.det_sources["neighborTileIds"] = self.neighborTaskId
        self.det_sources["xmin"], self.det_sources["xmax"] = self.ix_min, self.ix_max
        self.det_sources["ymin"], self.det_sources["ymax"] = self.iy_min, self.iy_max
        logger.info("[PROC %d] #%d objects found in tile image for task %d ..." % (self.procId, len(self.bboxes_det), self.tid))
        return 0


# ===============================
#        bit masks of the edge sources
# ===============================
def pack_sources(pixel_lists):
    """Edge sources -> the layout of include/mrcnn_hip.h (mrcnn_tile_source): every source as the row-major bit mask of the
    bounding box of its pixels ([y, x] lists, mosaic coordinates), numpy.packbits little-endian, rows padded to 32-bit words,
    all in one pool.  Returns (pool uint32 [words], desc int32 [n, 6] = x0, y0, w, h, word_offset, words_per_row).  A source
    without pixels becomes an empty 1 x 1 box at the origin."""
    n = len(pixel_lists)
    desc = np.zeros((n, 6), np.int32)
    chunks, off = [], 0
    for s, pixels in enumerate(pixel_lists):
        p = np.asarray(pixels, dtype=np.int64).reshape(-1, 2)
        if p.shape[0] == 0:
            y0 = x0 = 0
            h = w = 1
        else:
            y0, x0 = p.min(axis=0)
            h, w = p.max(axis=0) - (y0, x0) + 1
        wpr = (int(w) + 31) // 32
        m = np.zeros((int(h), wpr * 32), np.uint8)
        if p.shape[0]:
            m[p[:, 0] - y0, p[:, 1] - x0] = 1
        chunks.append(np.packbits(m, axis=1, bitorder="little").view("<u4").reshape(-1))
        desc[s] = (x0, y0, w, h, off, wpr)
        off += int(h) * wpr
    if off > 0x7FFFFFFF:
        raise ValueError("edge sources need %d mask words: more than one pool holds" % off)
    pool = np.concatenate(chunks).astype(np.uint32) if chunks else np.zeros(0, np.uint32)
    return pool, desc


def unpack_bitmap(words, h, w, wpr):
    """Inverse of one pack_sources entry: h * wpr uint32 words -> bool [h, w]."""
    b = np.unpackbits(np.ascontiguousarray(words, dtype="<u4").view(np.uint8).reshape(h, wpr * 4), axis=1, bitorder="little")
    return b[:, :w].astype(bool)


def source_planes_host(pool, desc, shrink, h, w):
    """pack_sources' sources as planes of a frame shrunk by k = shrink, the statement ops.sources_to_planes is held to: bool
    [n, h, w]; plane i has bit (Y, X) set exactly when source i has a pixel (y, x) with y // k == Y and x // k == X.  Pixels
    outside [0, k h) x [0, k w) are dropped; a source without pixels gives a zero plane."""
    k, h, w = int(shrink), int(h), int(w)
    pool = np.asarray(pool).reshape(-1).view(np.uint32)
    desc = np.asarray(desc, dtype=np.int64).reshape(-1, 6)
    planes = np.zeros((desc.shape[0], h, w), bool)
    for i, (x0, y0, sw, sh, off, wpr) in enumerate(desc):
        if sw <= 0 or sh <= 0:
            continue
        ys, xs = np.nonzero(unpack_bitmap(pool[off:off + sh * wpr], sh, sw, wpr))
        ys, xs = ys + y0, xs + x0
        keep = (ys >= 0) & (ys < k * h) & (xs >= 0) & (xs < k * w)
        planes[i, ys[keep] // k, xs[keep] // k] = True
    return planes


def plane_boxes_host(planes):
    """(y1, x1, y2, x2) per plane as utils.extract_bboxes: upper corner exclusive, zeros for an empty plane.  int32 [n, 4]."""
    boxes = np.zeros((len(planes), 4), np.int32)
    for i, m in enumerate(planes):
        ys, xs = np.nonzero(m)
        if ys.size:
            boxes[i] = (ys.min(), xs.min(), ys.max() + 1, xs.max() + 1)
    return boxes


# ===============================
#        SFinder
# ===============================
class SFinder(object):
    """sfinder.py:264-1500 for the run.py path.  ``tile_sources`` holds the per-tile result dicts (Analyzer.results + tile
    info), ``sources`` the final catalogue {"sources": [...]}."""

    # Fewer edge sources than this are merged on the host even with merge_device on.  0: measured, the device path wins from
    # the smallest merging case up (4 edge sources: 2.1 ms against 48 ms).
    MERGE_DEVICE_MIN_SOURCES = 0
    # Fewer sources than this get their parameters from the host statement even with params_device on.  Measured (DESIGN.md
    # 4.8): on a 1024 x 1024 image the device path is behind at 1 and 4 sources (0.78 against 0.42 ms, 1.16 against 1.05 ms) and
    # ahead at 116 (30.5 against 41.2 ms); 116 is the smallest count at which it was measured ahead on every mosaic.
    PARAMS_DEVICE_MIN_SOURCES = 116
    MOSAIC_CAPTIONS = ("name", "score", "none")
    PARAM_KEYS = ("nPix", "X0", "Y0", "X0w", "Y0w", "X0_wcs", "Y0_wcs", "X0w_wcs", "Y0w_wcs", "Xmin", "Xmax", "Ymin", "Ymax",
                  "Xmin_wcs", "Xmax_wcs", "Ymin_wcs", "Ymax_wcs", "S", "Smin", "Smax", "Smean", "Smedian", "Sstddev", "flux")

    def __init__(self, model, config):
        self.config = config
        self.model = model
        self.header = None
        self.image_id = ""
        self.nx = self.ny = -1
        self.read_subimg = False
        self.xmin = self.xmax = self.ymin = self.ymax = -1
        self.tileSizeX = self.tileSizeY = -1
        self.tileStepSizeX = self.tileStepSizeY = 1
        self.mpiEnabled = False
        self.comm = None                  # the gather's process group when WORLD_SIZE > 1
        self.nproc = 1
        self.tasks_per_worker = []
        self.procId = 0
        self.MASTER_ID = 0
        self.tile_sources = {"sources": []}
        self.sources = {"sources": []}
        self.save_tile_regions = False    # the reference defaults to one JSON + region file per tile as well (:314, :331)
        self.save_tile_json = False
        self.write_to_ds9 = True
        self.use_polygon_regions = True
        self.sregions = []
        self.outfile_ds9 = ""
        self.write_to_json = True
        self.outfile_json = ""
        self.merge_device = self._has_gpu()
        self.merge_device_min_sources = self.MERGE_DEVICE_MIN_SOURCES
        self.merge_timing = {}
        # Contours and pixel lists on the GPU (csrc/outline.hip): in every Analyzer the tiles build (Analyzer.results_device) and
        # for the merged sources of merge_edge_sources_device.  Off by default.
        self.results_device = False
        # Connected components on the GPU (csrc/components.hip) in every Analyzer the tiles build (Analyzer.components_device): the
        # pieces of split_masks.  Off by default.
        self.components_device = False
        self.compute_params = False       # the reference always computes them (:613-622); here run.py --compute_source_params
        self.params_device = self._has_gpu()
        self.params_device_min_sources = self.PARAMS_DEVICE_MIN_SOURCES
        self.params_sigma, self.params_maxiters = 3.0, 5          # astropy's sigma_clipped_stats defaults
        self.params_timing = {}
        self.beamArea = 0
        self.wcs = None
        self._plane = None                # (image plane as stored, path, header) while tiles / compute_sources_params need it
        self._plane_dev = None            # (its device copy, big-endian bytes?, path): uploaded once, shared by both
        # Tiles per model.detect call of run_parallel.  0: the reference's loop, one file read / host stretch / detect per tile.
        # N >= 1: the batched, device-resident front end (needs read_fits flags that end in a uint8 RGB image on the device, see
        # _tiles_batched(), and a model built for batches of N).
        self.tile_batch = 0
        self._wcs_warned = False
        # The overview picture of the mosaic with the merged catalogue on it: off by default.
        self.draw_mosaic = False
        self.mosaic_outfile = ""          # "": mosaic_<image_id>.png
        self.mosaic_shrink = None         # None: max(1, ceil(max(ny, nx) / 1024))
        self.mosaic_scale = None          # None: draw.default_scale(h, w)
        self.mosaic_captions = "name"     # "name", "score" or "none"
        self.mosaic_shaded = False
        self.mosaic_device = self._has_gpu()
        self.mosaic_timing = {}

    def _device(self):
        return analyze.model_device(self.model)

    def _has_gpu(self):
        return analyze.model_has_gpu(self.model)

    # ---- image / tile parameters (sfinder.py:336-444) -------------------------------------------------------
    def set_img_size_params(self):
        cfg = self.config
        self.header = self._read_header()
        if self.header is None:
            logger.error("[PROC %d] Header read from image %s is None!" % (self.procId, cfg.IMG_PATH))
            return -1
        xmin, xmax, ymin, ymax = cfg.IMG_XMIN, cfg.IMG_XMAX, cfg.IMG_YMIN, cfg.IMG_YMAX
        if xmin >= 0 and xmax >= 0 and ymin >= 0 and ymax >= 0:
            self.read_subimg = True
            # sfinder.py:353-354: the size is taken from the range BEFORE it is assigned (1 x 1 on a fresh object); as written
            self.nx = (self.xmax - self.xmin + 1)
            self.ny = (self.ymax - self.ymin + 1)
            self.xmin, self.xmax, self.ymin, self.ymax = xmin, xmax, ymin, ymax
        else:
            self.read_subimg = False
            if 'NAXIS1' not in self.header or 'NAXIS2' not in self.header:
                logger.error("[PROC %d] NAXIS1 / NAXIS2 keyword missing in header!" % self.procId)
                return -1
            self.nx, self.ny = self.header['NAXIS1'], self.header['NAXIS2']
            self.xmin, self.xmax, self.ymin, self.ymax = 0, self.nx - 1, 0, self.ny - 1
        self.tileSizeX, self.tileSizeY = self.nx, self.ny
        self.tileStepSizeX = self.tileStepSizeY = 1
        if cfg.SPLIT_IMG_IN_TILES:
            self.tileSizeX, self.tileSizeY = cfg.TILE_XSIZE, cfg.TILE_YSIZE
            self.tileStepSizeX, self.tileStepSizeY = cfg.TILE_XSTEP, cfg.TILE_YSTEP
        self.image_id = os.path.splitext(os.path.basename(os.path.abspath(cfg.IMG_PATH)))[0]
        # :400-439: the beam area in pixels, 0 unless all five keywords are there
        self.beamArea = 0
        found = True
        for key, attr in (("CDELT1", "dX"), ("CDELT2", "dY"), ("BMAJ", "bmaj"), ("BMIN", "bmin"), ("BPA", "pa")):
            if key not in self.header:
                # (the reference warns on every run; here only a run that asked for the parameters hears about it)
                logger.log(logging.WARNING if self.compute_params else logging.DEBUG,
                           "[PROC %d] %s keyword missing in header!" % (self.procId, key))
                found = False
            else:
                setattr(self, attr, self.header[key])
        try:
            if found:
                self.pixelArea = np.abs(self.dX * self.dY)
                self.beamArea = (np.pi * self.bmaj * self.bmin / (4 * np.log(2))) / self.pixelArea
        except Exception as e:              # a non-numeric keyword must not fail a run that never asked for the parameters
            logger.warning("[PROC %d] Beam area not computed (%s: %s)" % (self.procId, type(e).__name__, e))
            self.beamArea = 0
        self.wcs = fits.SimpleWCS.from_header(self.header)                # :442
        if not self._tiles_batched():
            self._drop_plane()
        return 0

    def _tiles_chain(self):
        """(DeviceChain, None) of this run's read_fits flags, or (None, why): fits.device_chain decides, as for read_fits(device=)."""
        cfg = self.config
        return fits.device_chain(cfg.ZSCALE_STRETCH, cfg.NORMALIZE_IMG, cfg.IMG_TO_RGB, cfg.IMG_TO_UINT8, cfg.BIAS_CONTRAST_STRETCH,
                                 cfg.ZSCALE_CONTRASTS, cfg.IMG_CONTRAST, cfg.IMG_BIAS)

    def _tiles_batched(self):
        """True when run_parallel takes the batched front end: tile_batch set and read_fits flags the device chain computes
        (fits.device_chain: uint8 RGB, float32 RGB or float32 gray tiles).  A chain whose image does not have the model's input
        channels -- gray tiles for an RGB model or the reverse -- is a configuration error: ValueError, no fallback.  The channels
        are those of the MaskRCNN's stem; an object without an engine (a test's stand-in for the model) is handed uint8 RGB tiles
        only, as before."""
        if self.tile_batch < 1:
            return False
        chain, _ = self._tiles_chain()
        if chain is None:
            return False
        layout = getattr(getattr(self.model, "engine", None), "layout", None)
        if layout is None:                       # not a MaskRCNN (stand-in models of the tests): uint8 RGB tiles, what it always got
            return chain.out_kind == 0
        model_c = int(layout.by_name["conv1"].shape[2])
        if (1 if chain.out_kind == 2 else 3) != model_c:
            raise ValueError("tile_batch: the read_fits flags give %s tiles, the model's first layer takes %d channel(s) (IMG_TO_RGB %r)"
                             % ("gray" if chain.out_kind == 2 else "RGB", model_c, self.config.IMG_TO_RGB))
        return True

    def _read_header(self):
        """The header of the image; on the batched path from the ONE read of the file that also gives the plane."""
        if self._tiles_batched():
            self._drop_plane()
            try:
                self._image_plane()
                return self._plane[2]
            except Exception as e:
                logger.warning("[PROC %d] Image plane of %s not read (%s: %s)" % (self.procId, self.config.IMG_PATH, type(e).__name__, e))
                self._drop_plane()
        return fits.get_fits_header(self.config.IMG_PATH)

    def _drop_plane(self):
        self._plane = self._plane_dev = None

    # ---- single image (sfinder.py:450-523) ------------------------------------------------------------------
    def run(self):
        cfg = self.config
        batch, self.tile_batch = self.tile_batch, 0           # one image, no tiles: nothing here would use a resident plane
        try:
            rc = self.set_img_size_params()
        finally:
            self.tile_batch = batch
        if rc < 0:
            logger.error("Failed to set image size parameters!")
            return -1
        res = fits.read_fits(cfg.IMG_PATH, cfg.IMG_XMIN, cfg.IMG_XMAX, cfg.IMG_YMIN, cfg.IMG_YMAX, stretch=cfg.ZSCALE_STRETCH,
                             zscale_contrasts=cfg.ZSCALE_CONTRASTS, normalize=cfg.NORMALIZE_IMG, convertToRGB=cfg.IMG_TO_RGB,
                             to_uint8=cfg.IMG_TO_UINT8, stretch_biascontrast=cfg.BIAS_CONTRAST_STRETCH, bias=cfg.IMG_BIAS,
                             contrast=cfg.IMG_CONTRAST)
        if res is None:
            logger.error("Failed to read image %s!" % cfg.IMG_PATH)
            return -1
        image_data, _ = res
        analyzer = Analyzer(self.model, cfg)
        analyzer.write_to_json = True
        analyzer.outfile_json = self.outfile_json or cfg.OUTFILE_JSON
        analyzer.outfile_ds9 = self.outfile_ds9
        analyzer.iou_thr, analyzer.score_thr = cfg.IOU_THR, cfg.SCORE_THR
        analyzer.results_device = self.results_device
        analyzer.components_device = self.components_device
        if analyzer.predict(image_data, self.image_id) < 0:               # sfinder.py:493: no offsets, no header
            logger.error("Failed to run model prediction on image %s!" % cfg.IMG_PATH)
            return -1
        if not analyzer.bboxes:
            logger.info("No object detected in image %s ..." % cfg.IMG_PATH)
            return 0
        logger.info("#%d objects found in image %s ..." % (len(analyzer.bboxes), cfg.IMG_PATH))
        return 0

    # ---- ranks ------------------------------------------------------------------------------------------------
    def init_mpi(self):
        """The reference's MPI set-up (sfinder.py:528-546) with RANK / WORLD_SIZE processes: torch.distributed from
        parallel.init_distributed(); the gather runs over a gloo group (object collectives need no GPU)."""
        world = int(os.environ.get("WORLD_SIZE", "1"))
        if world <= 1:
            self.mpiEnabled, self.nproc, self.procId, self.comm = False, 1, 0, None
            return
        import torch.distributed as dist
        from . import parallel
        rank, _, world = parallel.init_distributed()
        self.comm = dist.group.WORLD if dist.get_backend() == "gloo" else dist.new_group(backend="gloo")
        self.mpiEnabled, self.nproc, self.procId = True, world, rank

    # ---- tiles (sfinder.py:549-638) ---------------------------------------------------------------------------
    def run_parallel(self):
        try:
            return self._run_parallel()
        finally:
            self._drop_plane()                  # the whole image, host and device copy: never kept beyond the run

    def _run_parallel(self):
        self.init_mpi()
        t0 = time.time()
        status = 0
        if self.set_img_size_params() < 0:
            logger.error("[PROC %d] Failed to set image size parameters!" % self.procId)
            status = -2
        elif self.create_tile_tasks() < 0:
            logger.warning("[PROC %d] Failure in create tile tasks, exit..." % self.procId)
            status = -2
        if status == 0:
            tasks = self.tasks_per_worker[self.procId]
            if self._tiles_batched():
                status = self._run_tasks_batched(tasks)
            else:
                if self.tile_batch >= 1:
                    logger.info("[PROC %d] tile_batch = %d ignored: %s; tiles are read and detected one at a time" % (
                        self.procId, self.tile_batch, self._tiles_chain()[1] or "the model has no engine to read its input channels "
                        "from, and the tiles are not uint8 RGB"))
                for j, task in enumerate(tasks):
                    logger.info("[PROC %d] Start processing of task id %d (%d/%d) ..." % (self.procId, task.tid, j + 1, len(tasks)))
                    if self._run_task(j, task, task.find_sources) < 0:
                        status = -1
            if status < 0:
                logger.warning("[PROC %d] One or more errors occurred in source finding tasks..." % self.procId)
            if self.procId != self.MASTER_ID or not (self.compute_params or self.draw_mosaic):
                self._drop_plane()
            elif not ((self.compute_params and self.params_device) or (self.draw_mosaic and self.mosaic_device)):
                self._plane_dev = None          # the host statements (parameters, overview) cut from the host copy
        # every rank arrives here, whatever happened above (the reference returns early on a set-up error and leaves the others
        # in the barrier): a rank whose set-up failed contributes nothing
        if self.gather_task_data_from_workers(skip_local=(status == -2)) < 0:
            return -1
        if status == -2:
            return -1
        if self.procId == self.MASTER_ID:
            logger.info("[PROC %d] Merging sources at tile edges ..." % self.procId)
            self.merge_edge_sources()
            if self.compute_params:                                       # :613-622 (the reference: always)
                logger.info("[PROC %d] Computing source parameters ..." % self.procId)
                self.compute_sources_params()
            self.save()
            if self.draw_mosaic:
                self.draw_mosaic_results()
            logger.info("[PROC %d] Run completed in %d seconds" % (self.procId, time.time() - t0))
        return 0

    def _run_task(self, j, task, find):
        """One tile: find() fills task.det_sources (0 / -1), then the edge flags.  -1 when the tile failed."""
        try:
            rc = find()
        except Exception as e:              # a failing tile must not keep this rank out of the gather below
            logger.error("[PROC %d] Task id %d raised %s: %s" % (self.procId, task.tid, type(e).__name__, e))
            task.det_sources = {}
            rc = -1
        if rc < 0:                          # sfinder.py:583-586: log, remember, next tile
            logger.error("[PROC %d] Failed to find sources in task no. %d, skip to next!" % (self.procId, j))
            return -1
        self.find_sources_at_edge(j)
        return 0

    # ---- tiles, N per detect call ---------------------------------------------------------------------------------
    def _run_tasks_batched(self, tasks):
        """This rank's tiles in task order, in groups of tile_batch: one prepare_tile_images + one _detect_images per group, then
        per tile the Analyzer and the edge flags as in the loop above.  A tile read_fits would refuse (xmax <= xmin) fails alone;
        a tile the device chain does not take (above its size limit, a negative corner) and every tile of a group whose prepare or
        detect raised go through task.find_sources(), so that a bad tile or batch costs what it costs today."""
        N = int(self.tile_batch)
        status = 0
        for g0 in range(0, len(tasks), N):
            group = list(range(g0, min(g0 + N, len(tasks))))
            refused = [j for j in group if tasks[j].ix_max <= tasks[j].ix_min or tasks[j].iy_max <= tasks[j].iy_min]
            batched = [j for j in group if j not in refused and self._tile_batchable(tasks[j])]
            results = {}
            if batched:
                try:
                    images = self.prepare_tile_images([tasks[j] for j in batched])
                    results = dict(zip(batched, self._detect_images(images)))
                except Exception as e:
                    logger.error("[PROC %d] Tiles %s: batched read / detect raised %s: %s; taking them one at a time" % (
                        self.procId, [tasks[j].tid for j in batched], type(e).__name__, e))
                    results = {}
            for j in group:
                task = tasks[j]
                logger.info("[PROC %d] Start processing of task id %d (%d/%d) ..." % (self.procId, task.tid, j + 1, len(tasks)))
                if j in refused:
                    logger.error("xmax/ymax must be > xmin/ymin for tile reading!")
                    logger.warning("[PROC %d] Failed to read tile image for task %d!" % (self.procId, task.tid))
                    find = lambda: -1
                elif j in results:
                    find = lambda task=task, res=results[j]: task.accept_detection(res[0], self.header, res[1], res[2])
                else:
                    find = task.find_sources
                if self._run_task(j, task, find) < 0:
                    status = -1
        return status

    def _tile_batchable(self, task):
        return min(task.ix_min, task.ix_max, task.iy_min, task.iy_max) >= 0 and \
            (task.ix_max - task.ix_min) * (task.iy_max - task.iy_min) <= fits.DEVICE_TILE_MAX_PIXELS

    def prepare_tile_images(self, tasks):
        """The network input images of `tasks`' tiles, in order: device tensors -- uint8 [h, w, 3], float32 [h, w, 3] or, gray,
        float32 [h, w, 1] -- cut from the resident plane (as NumPy slicing cuts: clipped to the plane), NaN-filled, stretched,
        normalised and converted in one ops.fits_tiles_to_image call (any combination _tiles_batched() accepts) -- value for value
        what fits.read_fits gives per tile."""
        from . import ops
        plane_t, big = self._plane_device()
        ny, nx = int(plane_t.shape[0]), int(plane_t.shape[1])
        rects = []
        for t in tasks:
            x0, x1, y0, y1 = min(t.ix_min, nx), min(t.ix_max, nx), min(t.iy_min, ny), min(t.iy_max, ny)
            rects.append((x0, y0, x1 - x0, y1 - y0))
        chain, why = self._tiles_chain()
        if chain is None:
            raise RuntimeError("prepare_tile_images: the read_fits flags are not the device chain's (%s)" % why)
        images = ops.fits_tiles_to_image(plane_t, rects, chain, big_endian=big)
        if chain.out_kind == 2:
            images = [im.view(im.shape[0], im.shape[1], 1) for im in images]      # the model's gray image is [h, w, 1]
        return images

    def _detect_images(self, images):
        """One model.detect call on a group of tile images (host arrays or device tensors).  The model takes exactly tile_batch
        images: a short group is padded by repeating its last image, and what the padding produced is dropped, the device masks
        the model keeps (last_masks_device) included.  Returns per image (shape, result dict, device masks or None)."""
        n, N = len(images), int(self.tile_batch)
        padded = list(images) + [images[-1]] * (N - n)
        res = self.model.detect(padded, verbose=0)
        kept = getattr(self.model, "last_masks_device", None)
        if isinstance(kept, list) and len(kept) > n:
            del kept[n:]
        return [(tuple(int(v) for v in images[i].shape), res[i], kept[i] if kept and i < len(kept) else None) for i in range(n)]

    # ---- edge flags (sfinder.py:643-706) ----------------------------------------------------------------------
    def find_sources_at_edge(self, tindex):
        tileData = self.tasks_per_worker[self.procId][tindex]
        sourceTileData = tileData.det_sources
        if not sourceTileData or not sourceTileData["objs"]:
            logger.warning("[PROC %d] No sources for this tile, nothing to be done..." % self.procId)
            return
        sources = sourceTileData["objs"]
        xmin, xmax, ymin, ymax = tileData.ix_min, tileData.ix_max, tileData.iy_min, tileData.iy_max
        for source in sources:
            xmin_s, xmax_s, ymin_s, ymax_s = source["x1"], source["x2"], source["y1"], source["y2"]
            # sfinder.py:676-682: the box touches the tile's own frame (x2 / y2 are exclusive, ix_max / iy_max as generated)
            if xmin_s == xmin or xmax_s == xmax or ymin_s == ymin or ymax_s == ymax:
                source["edge"] = True
                continue
            # sfinder.py:685-706: the box intersects a neighbour tile.  A flag the Analyzer already set is never cleared.
            for tindex_n, windex_n in zip(tileData.neighborTaskIndex, tileData.neighborWorkerId):
                t = self.tasks_per_worker[windex_n][tindex_n]
                if xmax_s < t.ix_min or xmin_s > t.ix_max or ymax_s < t.iy_min or ymin_s > t.iy_max:
                    continue
                source["edge"] = True
                break

    # ---- gather (sfinder.py:940-988) --------------------------------------------------------------------------
    def gather_task_data_from_workers(self, skip_local=False):
        """tile_sources = the non-empty det_sources of every worker's tasks, worker by worker (rank 0 only when there are
        several ranks).  The serial reference never fills tile_sources (the call sits under `if self.mpiEnabled`, :599) and so
        merges nothing; here one process runs the local half of the gather, which is what the MPI run of one rank does."""
        self.tile_sources = {"sources": []}
        if not skip_local and self.tasks_per_worker:
            for task in self.tasks_per_worker[self.procId]:
                if task.det_sources:
                    self.tile_sources["sources"].append(task.det_sources)
        if not self.mpiEnabled:
            return 0
        import torch.distributed as dist
        gathered = [None] * self.nproc if self.procId == self.MASTER_ID else None
        dist.gather_object(self.tile_sources, gathered, dst=self.MASTER_ID, group=self.comm)
        if self.procId == self.MASTER_ID:
            for i in range(1, self.nproc):                  # :963-972: appended in rank order
                self.tile_sources["sources"].extend(gathered[i]["sources"])
        return 0

    # ---- merge (sfinder.py:711-935) ---------------------------------------------------------------------------
    def merge_edge_sources(self):
        if self.procId != self.MASTER_ID:
            return 0
        # measured: the device path wins from the smallest merging case up (4 edge sources: 2.1 ms against 48 ms),
        # so there is no size below which the host statement is preferred
        return self.merge_edge_sources_device() if self.merge_device else self.merge_edge_sources_host()

    def _split_edge_sources(self):
        """:719-730: non-edge sources go to the catalogue as they are (merged = False), edge sources are listed for merging."""
        sourcesToBeMerged = []
        self.sources["sources"] = []
        for tile_index, tileData in enumerate(self.tile_sources["sources"]):
            for j, s in enumerate(tileData["objs"]):
                if not s["edge"]:
                    s["merged"] = False
                    self.sources["sources"].append(s)
                    continue
                sourcesToBeMerged.append(MergedSourceInfo(j, tile_index))
        return sourcesToBeMerged

    def _edge_source(self, info):
        return self.tile_sources["sources"][info.tindex]["objs"][info.sindex]

    def _finish_merge(self, sourcesToBeMerged, cc, merged_of):
        """:821-933: components of one keep their object; larger ones become the object merged_of(i, members) builds; then
        every source is renamed S1..Sn."""
        for i, comp in enumerate(cc):
            if not comp:
                continue
            if len(comp) == 1:
                source = self._edge_source(sourcesToBeMerged[comp[0]])
                source["name"] = "S" + str(i + 1) + "_merged"
                source["merged"] = False
                self.sources["sources"].append(source)
            else:
                self.sources["sources"].append(merged_of(i, comp))
        for i, s in enumerate(self.sources["sources"]):                   # :928-933
            s["name"] = "S" + str(i + 1)
        return 0

    @staticmethod
    def _merged_source(name, last, pixels_merged, mask, xmin, ymin, contours=None):
        """:864-924 from the union's pixels: `mask` = the union in its tight box [ymin.., xmin..].  contours: the mask's contours
        as float64 (x, y) arrays in the box's own frame (ops.bitmap_outlines), which replace the find_contours call."""
        dy, dx = mask.shape
        xmax, ymax = xmin + dx - 1, ymin + dy - 1                         # :879-882: pixel max, i.e. INCLUSIVE (unmerged: exclusive)
        if contours is not None:
            vertexes = [(c + np.array([xmin, ymin])).tolist() for c in contours]
        else:
            offset = 10                                                       # :887
            padded_mask = np.zeros((dy + 2 * offset, dx + 2 * offset), dtype=np.uint8)
            padded_mask[offset:offset + dy, offset:offset + dx] = mask
            vertexes = []
            for verts in analyze.find_contours(padded_mask, 0.5):
                verts = np.fliplr(verts)                                      # :902: (y, x) -> (x, y), padding kept ...
                verts = verts.tolist()
                for v in verts:                                               # :906-909: ... and removed here
                    v[0] += xmin - offset
                    v[1] += ymin - offset
                vertexes.append(verts)
        # :865-870: class / score of `sourcesToBeMerged[index]` with index the LAST member visited (index_largest is computed
        # and never used)
        return {"name": name, "x1": int(xmin), "x2": int(xmax), "y1": int(ymin), "y2": int(ymax), "edge": True, "merged": True,
                "score": last["score"], "class_name": last["class_name"], "class_id": last["class_id"],
                "pixels": pixels_merged, "vertexes": vertexes}

    # -- host statement ------------------------------------------------------------------------------------------
    def merge_edge_sources_host(self):
        """The reference's algorithm as written: every pair j > i of edge sources, neighbour-tile test, box test, pixel-pair
        test, components, first-seen pixel union.  The two innermost loops are NumPy expressions of the same predicates (the
        pixel-pair test by broadcasting, the `x not in pixels_merged` scan through a set): same results, same order."""
        if self.procId != self.MASTER_ID:
            return 0
        todo = self._split_edge_sources()
        N = len(todo)
        tiles = self.tile_sources["sources"]
        srcs = [self._edge_source(t) for t in todo]
        pix = [np.asarray(s["pixels"], dtype=np.int64).reshape(-1, 2) for s in srcs]
        edges = []
        for i in range(N):
            s = srcs[i]
            tids_neighbor = tiles[todo[i].tindex]["neighborTileIds"]
            xmin, xmax, ymin, ymax = s["x1"], s["x2"], s["y1"], s["y2"]
            for j in range(i + 1, N):
                sj = srcs[j]
                if tiles[todo[j].tindex]["tileId"] not in tids_neighbor:             # :771: one-sided, as written
                    continue
                if xmax < sj["x1"] or xmin > sj["x2"] or ymax < sj["y1"] or ymin > sj["y2"]:     # :776-781
                    continue
                if self._pixels_adjacent(pix[i], pix[j]):                            # :787-810
                    edges.append((i, j))
        cc = analyze.connected_components(N, edges)                                  # :820, mrcnn/graph.py

        def merged_of(i, comp):
            pixels_merged, seen = [], set()
            for index in comp:                                                        # :848-862: first-seen order
                for p in srcs[index]["pixels"]:
                    key = (p[0], p[1])
                    if key not in seen:
                        seen.add(key)
                        pixels_merged.append(p)
            arr = np.asarray(pixels_merged, dtype=np.int64)
            ymin, xmin = arr.min(axis=0)
            ymax, xmax = arr.max(axis=0)
            mask = np.zeros((ymax - ymin + 1, xmax - xmin + 1), np.uint8)
            mask[arr[:, 0] - ymin, arr[:, 1] - xmin] = 1
            return self._merged_source("S" + str(i + 1) + "_merged", srcs[comp[-1]], pixels_merged, mask, int(xmin), int(ymin))

        return self._finish_merge(todo, cc, merged_of)

    @staticmethod
    def _pixels_adjacent(a, b, chunk=512):
        """:787-810: some pixel of a and some pixel of b with |dx| <= 1 and |dy| <= 1 ([y, x] rows)."""
        if a.shape[0] == 0 or b.shape[0] == 0:
            return False
        for k in range(0, a.shape[0], chunk):
            d = np.abs(a[k:k + chunk, None, :] - b[None, :, :])
            if np.any((d[..., 0] <= 1) & (d[..., 1] <= 1)):
                return True
        return False

    # -- device path ---------------------------------------------------------------------------------------------
    def candidate_pairs(self, todo):
        """The pairs the reference's double loop hands to the pixel test (:756-781), without visiting all N^2: per pair of
        tile entries (a before b in tile_sources, b's tile id among a's neighbour ids) the box test on integer arrays.
        Returned sorted by (i, j), the order in which the reference adds graph edges."""
        tiles = self.tile_sources["sources"]
        by_tile = {}
        for k, t in enumerate(todo):
            by_tile.setdefault(t.tindex, []).append(k)
        box = np.array([[s["x1"], s["x2"], s["y1"], s["y2"]] for s in (self._edge_source(t) for t in todo)], dtype=np.int64).reshape(-1, 4)
        order = sorted(by_tile)
        out = []
        for ai, ta in enumerate(order):
            ia = np.asarray(by_tile[ta])
            neighbors = set(tiles[ta]["neighborTileIds"])
            for tb in order[ai + 1:]:
                if tiles[tb]["tileId"] not in neighbors:
                    continue
                ib = np.asarray(by_tile[tb])
                A, B = box[ia][:, None, :], box[ib][None, :, :]
                disjoint = (A[..., 1] < B[..., 0]) | (A[..., 0] > B[..., 1]) | (A[..., 3] < B[..., 2]) | (A[..., 2] > B[..., 3])
                ii, jj = np.nonzero(~disjoint)
                if ii.size:
                    out.append(np.stack([ia[ii], ib[jj]], axis=1))
        if not out:
            return np.zeros((0, 2), np.int32)
        pairs = np.concatenate(out)
        return pairs[np.lexsort((pairs[:, 1], pairs[:, 0]))].astype(np.int32)

    def merge_edge_sources_device(self):
        """Same catalogue as merge_edge_sources_host; the pixel-pair test and the pixel union run on the GPU on bit masks."""
        if self.procId != self.MASTER_ID:
            return 0
        import torch
        from . import ops
        clock = time.perf_counter
        t = [clock()]
        todo = self._split_edge_sources()
        N = len(todo)
        srcs = [self._edge_source(t_) for t_ in todo]
        if N == 0:
            return self._finish_merge(todo, [], None)
        dev = self._device()
        pairs = self.candidate_pairs(todo)
        t.append(clock())
        pool, desc = pack_sources([s["pixels"] for s in srcs])
        t.append(clock())
        pool_t, desc_t = ops.tile_upload(pool, desc, dev)
        adj = ops.tile_adjacency(pool_t, desc_t, pairs).cpu().numpy() if len(pairs) else np.zeros(0, np.int32)
        t.append(clock())
        edges = [(int(i), int(j)) for i, j in pairs[adj != 0]]
        cc = analyze.connected_components(N, edges)
        multi = [k for k, comp in enumerate(cc) if len(comp) > 1]
        t.append(clock())
        result = {}
        if multi:
            members = [cc[k] for k in multi]
            comp_offsets = np.concatenate([[0], np.cumsum([len(m) for m in members])]).astype(np.int32)
            member_ids = np.concatenate(members).astype(np.int32)
            u = ops.tile_union(pool_t, desc_t, desc, comp_offsets, member_ids)
            out_desc = u["out_desc"].cpu().numpy()
            out_count = u["out_count"].cpu().numpy()
            out_pool = u["out_pool"].cpu().numpy().view(np.uint32)
            fresh_pool = u["fresh_pool"].cpu().numpy().view(np.uint32)        # .cpu() synchronises with the launches
            outlines = self._union_outlines(u, out_desc) if self.results_device else None
            t.append(clock())
            for c, k in enumerate(multi):
                parts = []
                for q in range(comp_offsets[c], comp_offsets[c + 1]):
                    x0, y0, w, h, _, wpr = (int(v) for v in desc[member_ids[q]])
                    fo = int(u["fresh_offsets"][q])
                    parts.append(np.argwhere(unpack_bitmap(fresh_pool[fo:fo + h * wpr], h, w, wpr)) + (y0, x0))
                pixels = np.concatenate(parts)
                x0, y0, w, h, off, wpr = (int(v) for v in out_desc[c])
                assert pixels.shape[0] == int(out_count[c]), "tile_union: fresh bitmaps and union count disagree"
                result[k] = (pixels.tolist(), unpack_bitmap(out_pool[off:off + h * wpr], h, w, wpr), x0, y0,
                             None if outlines is None else outlines[c])
        else:
            t.append(clock())
        t.append(clock())
        self.merge_timing = {"edge_sources": N, "pairs": int(len(pairs)), "edges": len(edges), "components_merged": len(multi),
                             "pool_words": int(pool.size)}
        for name, a, b in zip(("candidate_pairs", "pack", "upload_adjacency_download", "components", "union_download", "pixel_lists"),
                              t[:-1], t[1:]):
            self.merge_timing[name + "_ms"] = round(1e3 * (b - a), 3)

        def merged_of(i, comp):
            pixels, mask, x0, y0, contours = result[i]
            return self._merged_source("S" + str(i + 1) + "_merged", srcs[comp[-1]], pixels, mask.astype(np.uint8), x0, y0, contours)

        return self._finish_merge(todo, cc, merged_of)

    def _union_outlines(self, u, out_desc):
        """The contours of all unions of ops.tile_union's result `u`, outlined where they lie (out_pool / out_desc, one call, one
        download): per component a list of float64 (x, y) arrays in the union's own box.  None when the device form has failed
        in this process (analyze.device_or_host): the merged sources then take find_contours, as with the switch off.  A table
        the check calls malformed would be a bug of tile_union: that ValueError is not caught."""
        def outlines():
            from . import ops
            got = ops.bitmap_outlines(u["out_pool"], u["out_desc"], out_desc).host()
            sc, co = got["source_contours"].tolist(), got["contour_offsets"].tolist()
            points = got["points"].astype(np.float64)
            return [[points[co[k]:co[k + 1]] for k in range(sc[c], sc[c + 1])] for c in range(len(sc) - 1)]
        return analyze.device_or_host("bitmap_outlines", outlines, lambda: None)

    # ---- source parameters (sfinder.py:994-1211) --------------------------------------------------------------
    def _image_plane(self):
        """The plane utils.read_fits cuts from (utils.py:1061-1078: [0, 0] of a 4-D cube, a 2-D image as it is), read once and
        left as the file stores it (an unscaled float32 image: the read-only big-endian view of the file's bytes -- the host
        statement converts the cut-outs it takes, the device path uploads the bytes as they are).  compute_sources_params drops
        it when it is done."""
        path = self.config.IMG_PATH
        if self._plane is None or self._plane[1] != path:
            data, header = fits.read_primary_hdu(path, native=False)
            if data.ndim == 4:
                data = data[0, 0]
            elif data.ndim != 2:
                raise ValueError("Invalid/unsupported number of channels found in file %s (nchan=%d)!" % (path, data.ndim))
            self._plane = (data, path, header)
        return self._plane[0]

    def _plane_device(self):
        """(_image_plane() on the device, big-endian?), uploaded once per run: an unscaled float32 image as the file's big-endian
        bytes (uint8 [ny, nx, 4]: the kernels swap what they read), anything else as float32 converted on the host once -- value for
        value what read_fits's per-tile astype(float32) gives."""
        path = self.config.IMG_PATH
        if self._plane_dev is None or self._plane_dev[2] != path:
            plane = self._image_plane()
            self._plane_dev = (self._upload_plane(plane), plane.dtype == np.dtype(">f4"), path)
        return self._plane_dev[0], self._plane_dev[1]

    def _upload_plane(self, plane):
        import torch
        ny, nx = plane.shape
        if plane.dtype == np.dtype(">f4"):
            raw = torch.from_numpy(np.array(plane, order="C", copy=True).view(np.uint8).reshape(ny, nx, 4))     # (the file view is read-only)
        else:
            raw = torch.from_numpy(np.ascontiguousarray(plane, dtype=np.float32))
        return raw.to(self._device())

    def _cutout_geometry(self, source, offset=10):
        """:1006-1016: (xmin, xmax, ymin, ymax, dx, dy, img_offset_x, img_offset_y).  dx = x2 - x1 + 1 whether x2 is the inclusive
        pixel maximum (merged sources) or the exclusive box corner (all others), as written."""
        xmin, xmax, ymin, ymax = source["x1"], source["x2"], source["y1"], source["y2"]
        dx, dy = xmax - xmin + 1, ymax - ymin + 1
        ox = min(min(offset, self.nx - 1 - xmax), min(offset, xmin))      # :1013
        oy = min(min(offset, self.ny - 1 - ymax), min(offset, ymin))      # :1014
        return xmin, xmax, ymin, ymax, dx, dy, ox, oy

    def _finish_params(self, source, xoffset, yoffset, npix, S, Smin, Smax, clipped, m, mw):
        """:1058-1211 from the sums: m = (sum 1, sum x, sum y) of the byte mask (cv.moments(smask, True)), mw = (sum I, sum x I,
        sum y I) in float64 over the cut-out that is zero outside the mask (cv.moments(simg, False)); x, y relative to the
        cut-out.  Values are plain Python numbers: write_json_results uses json.dump as it is."""
        x0 = m[1] / m[0] + xoffset                                        # :1061-1063 (m00 == 0: ZeroDivisionError, as cv's dict gives)
        y0 = m[2] / m[0] + yoffset
        if mw[0] == 0:                                                    # :1068-1071
            logger.warning("[PROC %d] Moment 00 is =0 for source %s, setting weighted centroid to non-weighted one..." % (
                self.procId, source["name"]))
            x0_w, y0_w = x0, y0
        else:
            x0_w = float(mw[1] / mw[0] + xoffset)                         # :1073-1075
            y0_w = float(mw[2] / mw[0] + yoffset)
        sky = [-999, -999, -999, -999]
        wcs = self.wcs
        if wcs is not None and wcs.valid:
            pad = [0] * (wcs.naxis - 2) if wcs.naxis in (3, 4) else []   # :1079-1095
            c, cw = wcs.all_pix2world([[x0, y0] + pad], 0), wcs.all_pix2world([[x0_w, y0_w] + pad], 0)
            sky = [float(c[0][0]), float(c[0][1]), float(cw[0][0]), float(cw[0][1])]
        elif not self._wcs_warned:
            self._wcs_warned = True
            logger.warning("[PROC %d] No sky positions (%s): the *_wcs keys are -999" % (
                self.procId, wcs.why if wcs is not None else "set_img_size_params was not run"))
        S = float(S)
        return {"nPix": int(npix), "X0": float(x0), "Y0": float(y0), "X0w": x0_w, "Y0w": y0_w, "X0_wcs": sky[0], "Y0_wcs": sky[1],
                "X0w_wcs": sky[2], "Y0w_wcs": sky[3], "Xmin": int(source["x1"]), "Xmax": int(source["x2"]), "Ymin": int(source["y1"]),
                "Ymax": int(source["y2"]), "Xmin_wcs": -999, "Xmax_wcs": -999, "Ymin_wcs": -999, "Ymax_wcs": -999,      # :1195-1198
                "S": S, "Smin": float(Smin), "Smax": float(Smax), "Smean": float(clipped[0]), "Smedian": float(clipped[1]),
                "Sstddev": float(clipped[2]), "flux": float(S / self.beamArea) if self.beamArea > 0 else S}              # :1206-1209

    def compute_source_params(self, source, offset=10):
        """The reference's statement for one source (:994-1211), on the host.  Raises where the reference's arithmetic does (a
        sub-image run: nx = ny = 1 makes the offsets hugely negative); compute_sources_params catches that per source."""
        if self.procId != self.MASTER_ID:
            return None
        xmin, xmax, ymin, ymax, dx, dy, ox, oy = self._cutout_geometry(source, offset)
        xoffset, yoffset = xmin - ox, ymin - oy                          # :1015-1016
        smask = np.zeros((dy + 2 * oy, dx + 2 * ox), dtype=np.uint8)     # :1019
        p = np.asarray(source["pixels"], dtype=np.int64).reshape(-1, 2)
        smask[p[:, 0] - yoffset, p[:, 1] - xoffset] = 1                  # :1021-1026 (a negative index wraps, as in the loop)
        # :1031-1042 = utils.read_fits with every stretch off (utils.py:1051-1091): the cut is made only when all four limits
        # are >= 0, float32, NaN -> the nanmin of THIS cut-out
        x0, x1, y0, y1 = xmin - ox, xmax + ox + 1, ymin - oy, ymax + oy + 1
        plane = self._image_plane()
        if x0 >= 0 and x1 >= 0 and y0 >= 0 and y1 >= 0:
            if x1 <= x0 or y1 <= y0:
                raise ValueError("xmax/ymax must be > xmin/ymin for tile reading!")
            plane = plane[y0:y1, x0:x1]
        simg = plane.astype(np.float32)
        with np.errstate(all="ignore"):
            simg[np.isnan(simg)] = np.nanmin(simg)
            simg[smask == 0] = 0                                          # :1046
            sdata = simg[smask > 0]                                       # :1047
            S = np.nansum(sdata)                                          # :1052-1055, float32 as NumPy does them
            npix = sdata.size - np.isnan(sdata).sum()
            Smin, Smax = np.nanmin(sdata), np.nanmax(sdata)
            clipped = fits.sigma_clipped_stats(sdata, self.params_sigma, self.params_maxiters)               # :1056
            ys, xs = np.nonzero(smask)
            m = (int(xs.size), int(xs.sum()), int(ys.sum()))              # :1060 cv.moments(smask, True)
            I = simg.astype(np.float64)                                   # :1067 cv.moments(simg, False)
            mw = (I.sum(), (I * np.arange(I.shape[1], dtype=np.float64)[None, :]).sum(),
                  (I * np.arange(I.shape[0], dtype=np.float64)[:, None]).sum())
            return self._finish_params(source, xoffset, yoffset, npix, S, Smin, Smax, clipped, m, mw)

    def _host_params(self, source):
        """The host statement for one catalogue entry; a source the reference's arithmetic fails on is logged and left without
        parameters (the reference itself would stop the run there)."""
        try:
            sparams = self.compute_source_params(source)
        except Exception as e:
            logger.error("[PROC %d] Source %s: parameters not computed (%s: %s)" % (self.procId, source.get("name", "?"), type(e).__name__, e))
            return False
        if sparams:                                                       # :621-622
            source.update(sparams)
        return True

    def compute_sources_params(self):
        """:613-622 for the whole catalogue.  With params_device: one upload of the image plane, one launch for all sources
        (ops.source_params), the dicts by _finish_params; sources whose offsets are negative (the wrap quirk), that have no pixels
        or whose pixels leave their own cut-out take the host statement, as does everything when the device path is not there."""
        if self.procId != self.MASTER_ID:
            return 0
        clock = time.perf_counter
        sources = self.sources["sources"]
        self.params_timing = {"sources": len(sources), "device_sources": 0, "host_sources": len(sources)}
        t0 = clock()
        host = list(range(len(sources)))
        if self.params_device and len(sources) >= max(1, self.params_device_min_sources):
            try:
                host = self._params_device(sources)
            except Exception as e:
                from ._hip import HipPathError
                if not isinstance(e, HipPathError):
                    raise
                logger.warning("[PROC %d] Source parameters on the host: %s" % (self.procId, e))
        t1 = clock()
        failed = sum(0 if self._host_params(sources[i]) else 1 for i in host)
        if not self.draw_mosaic:
            self._drop_plane()                                            # the whole image: not kept beyond this step
        self.params_timing.update({"host_sources": len(host), "device_sources": len(sources) - len(host), "failed_sources": failed,
                                   "device_path_ms": round(1e3 * (t1 - t0), 3), "host_statement_ms": round(1e3 * (clock() - t1), 3)})
        return 0

    def _params_device(self, sources):
        """Fills the sources the device path covers; returns the indices left to the host statement."""
        import torch
        from . import ops
        clock = time.perf_counter
        t = [clock()]
        dev = self._device()
        geo, pix, todo, host = [], [], [], []
        for i, s in enumerate(sources):
            p = np.asarray(s["pixels"], dtype=np.int64).reshape(-1, 2)
            try:
                g = self._cutout_geometry(s)
            except Exception:
                host.append(i)
                continue
            xmin, xmax, ymin, ymax, dx, dy, ox, oy = g
            x0, x1, y0, y1 = xmin - ox, xmax + ox + 1, ymin - oy, ymax + oy + 1
            inside = p.shape[0] and p[:, 1].min() >= x0 and p[:, 1].max() < x1 and p[:, 0].min() >= y0 and p[:, 0].max() < y1
            if ox < 0 or oy < 0 or not inside or x1 > self.nx or y1 > self.ny:
                host.append(i)
                continue
            todo.append(i)
            pix.append(p)
            geo.append((x0, y0, x1, y1))
        if not todo:
            return host
        t.append(clock())
        plane = self._image_plane()
        if tuple(plane.shape) != (self.ny, self.nx):
            from ._hip import HipPathError
            raise HipPathError("image plane %r is not the %d x %d the header states" % (plane.shape, self.ny, self.nx))
        img_t, big = self._plane_device()                                  # the batched tile front end's upload, when it made one
        t.append(clock())
        pool, desc = pack_sources(pix)
        t.append(clock())
        pool_t, desc_t = ops.tile_upload(pool, desc, dev)
        rec_t = ops.source_params(img_t, pool_t, desc_t, np.asarray(geo, np.int32), self.params_sigma, self.params_maxiters,
                                  big_endian=big, desc_host=desc)
        rec = rec_t.cpu().numpy().view(ops.source_record_dtype()).reshape(-1)          # .cpu() synchronises with the launch
        t.append(clock())
        for k, i in enumerate(todo):
            r, s = rec[k], sources[i]
            if int(r["n_gathered"]) != int(r["n_mask"]) or int(r["n_mask"]) == 0:
                host.append(i)
                continue
            try:
                s.update(self._finish_params(s, geo[k][0], geo[k][1], int(r["npix"]), np.float32(r["s64"]), r["smin"], r["smax"],
                                             (r["clip_mean"], r["clip_median"], r["clip_std"]),
                                             (int(r["m00"]), int(r["m10"]), int(r["m01"])), (r["w00"], r["w10"], r["w01"])))
            except Exception:
                host.append(i)
        t.append(clock())
        for name, a, b in zip(("select", "read_upload", "pack", "launch_download", "dicts"), t[:-1], t[1:]):
            self.params_timing[name + "_ms"] = round(1e3 * (b - a), 3)
        return sorted(host)

    # ---- the overview picture of the mosaic (no counterpart in the reference) -----------------------------
    def _mosaic_geometry(self):
        """(ny, nx, k, h, w, scale) of the overview frame, or None (logged) for settings that cannot be drawn."""
        from . import draw as overlay
        ny, nx = (int(v) for v in self._image_plane().shape)
        k = max(1, -(-max(ny, nx) // 1024)) if self.mosaic_shrink is None else self.mosaic_shrink
        if int(k) != k or k < 1:
            logger.error("Invalid mosaic_shrink %r (need an integer >= 1): nothing is drawn ..." % (self.mosaic_shrink,))
            return None
        k = int(k)
        h, w = -(-ny // k), -(-nx // k)
        scale = overlay.default_scale(h, w) if self.mosaic_scale is None else self.mosaic_scale
        if int(scale) != scale or scale < 1:
            logger.error("Invalid mosaic_scale %r (need an integer >= 1): nothing is drawn ..." % (self.mosaic_scale,))
            return None
        if self.mosaic_captions not in self.MOSAIC_CAPTIONS:
            logger.error("Invalid mosaic_captions %r (need one of %r): nothing is drawn ..." % (self.mosaic_captions, self.MOSAIC_CAPTIONS))
            return None
        return ny, nx, k, h, w, int(scale)

    def _mosaic_contrast(self):
        return float(self.config.ZSCALE_CONTRASTS[0])

    def _mosaic_pixel_lists(self):
        return [np.asarray(s["pixels"], dtype=np.int64).reshape(-1, 2) for s in self.sources["sources"]]

    def _mosaic_scene_of(self, image, masks, boxes, scale):
        """The scene dict of draw.py from the overview frame, the sources' planes (None: the device form keeps them) and the
        planes' boxes: colours by class_name from the map the Analyzer draws with, no ground truth, the captions at the upper
        left corner of the planes' boxes."""
        from . import draw as overlay
        sources = self.sources["sources"]
        colours = [overlay.CLASS_COLOR_MAP.get(s.get("class_name"), overlay.UNKNOWN_COLOUR) for s in sources]
        texts = []
        for s, (y1, x1, y2, x2) in zip(sources, boxes):
            if self.mosaic_captions == "name":
                texts.append((str(s.get("name", "")), int(x1), int(y1) - 1, overlay.CAPTION_COLOUR))
            elif self.mosaic_captions == "score":
                texts.append(("%.2f" % s["score"], int(x1), int(y1) - 1, overlay.CAPTION_COLOUR))
        return {"image": image, "scale": scale, "shaded": bool(self.mosaic_shaded), "masks": masks, "colours": colours,
                "boxes": [[int(v) for v in b] for b in boxes], "gt_boxes": [], "gt_colours": [], "texts": texts}

    def mosaic_scene(self):
        """The scene of draw.render_host for the mosaic and its catalogue: fits.mosaic_overview_host of the image plane with
        the contrast ZSCALE_CONTRASTS[0], source_planes_host of the catalogue's pixel lists, the planes' boxes (extract_bboxes
        convention -- not the catalogue's x1 .. y2, whose upper corner is inclusive for merged sources and exclusive for the
        others).  None (logged) for settings that cannot be drawn."""
        geo = self._mosaic_geometry()
        if geo is None:
            return None
        ny, nx, k, h, w, scale = geo
        image = fits.mosaic_overview_host(self._image_plane(), k, self._mosaic_contrast())
        pool, desc = pack_sources(self._mosaic_pixel_lists())
        planes = source_planes_host(pool, desc, k, h, w)
        return self._mosaic_scene_of(image, [m.astype(np.uint8) for m in planes], plane_boxes_host(planes), scale)

    def _render_mosaic_device(self):
        import torch
        from . import draw as overlay
        from . import ops
        clock = time.perf_counter
        timing = {"sources": len(self.sources["sources"])}
        geo = self._mosaic_geometry()
        if geo is None:
            return None
        ny, nx, k, h, w, scale = geo
        t0 = clock()
        plane_t, big = self._plane_device()                              # resident after a tile_batch / params_device run
        torch.cuda.synchronize(plane_t.device)
        t1 = clock()
        frame = ops.mosaic_overview(plane_t, k, self._mosaic_contrast(), big_endian=big)
        torch.cuda.synchronize(plane_t.device)
        t2 = clock()
        planes, boxes = None, np.zeros((0, 4), np.int32)
        if self.sources["sources"]:
            pool, desc = pack_sources(self._mosaic_pixel_lists())
            pool_t, desc_t = ops.tile_upload(pool, desc, plane_t.device)
            planes = ops.sources_to_planes(pool_t, desc_t, k, h, w)
            boxes = planes.box.cpu().numpy()
        t3 = clock()
        scene = self._mosaic_scene_of(None, None, boxes, scale)
        canvas = ops.draw_overlay(frame, planes, overlay.device_tables(scene), scale)
        torch.cuda.synchronize(canvas.device)
        t4 = clock()
        out = canvas.cpu().numpy()
        t5 = clock()
        for name, a, b in (("plane", t0, t1), ("overview", t1, t2), ("planes", t2, t3), ("render", t3, t4), ("download", t4, t5)):
            timing[name + "_ms"] = round(1e3 * (b - a), 3)
        self.mosaic_timing = timing
        return out

    def _render_mosaic_host(self):
        from . import draw as overlay
        clock = time.perf_counter
        t0 = clock()
        scene = self.mosaic_scene()
        if scene is None:
            return None
        t1 = clock()
        out = overlay.render_host(scene)
        self.mosaic_timing = {"sources": len(self.sources["sources"]), "scene_ms": round(1e3 * (t1 - t0), 3),
                              "render_ms": round(1e3 * (clock() - t1), 3)}
        return out

    def render_mosaic(self, device=None):
        """The overview picture as a uint8 array [s (h + 4), s (w + 4), 3], without writing a file: the whole plane stretched as
        read_fits stretches a tile and shrunk by block maxima to the frame [h, w], under the catalogue's sources drawn as
        Analyzer.draw_results draws detections (contours, boxes, captions; shaded with ``mosaic_shaded``).  None (logged) when it
        cannot be drawn.  device: None -- on the GPU where ``mosaic_device`` is on (measured ahead from a 384 x 320 mosaic with 5
        sources up: no size threshold), with the fallback of analyze.device_or_host; True -- the device form, errors raised;
        False -- the host statement.
        Both forms give the same bytes."""
        self.mosaic_timing = {}
        if device is True:
            return self._render_mosaic_device()
        if device is None and self.mosaic_device and self._has_gpu():
            from .ops import DrawUnsupported, MosaicUnsupported           # this picture only: a catalogue past MAX_ITEMS, ...
            return analyze.device_or_host("render_mosaic_device", self._render_mosaic_device, self._render_mosaic_host,
                                          refusal=(DrawUnsupported, MosaicUnsupported))
        return self._render_mosaic_host()

    def draw_mosaic_results(self, device=None):
        """Write render_mosaic() as an 8-bit RGB PNG to ``mosaic_outfile`` (default mosaic_<image_id>.png).  Rank 0 only.  0, or
        -1 when nothing could be drawn."""
        if self.procId != self.MASTER_ID:
            return 0
        from . import draw as overlay
        try:
            canvas = self.render_mosaic(device)
        except Exception as e:                      # a picture must not fail a run whose catalogue is already written
            logger.error("[PROC %d] The mosaic picture could not be drawn (%s: %s)" % (self.procId, type(e).__name__, e))
            canvas = None
        if canvas is None:
            return -1
        outfile = self.mosaic_outfile or "mosaic_%s.png" % self.image_id
        t0 = time.perf_counter()
        overlay.write_png(outfile, canvas)
        self.mosaic_timing["encode_ms"] = round(1e3 * (time.perf_counter() - t0), 3)
        logger.info("[PROC %d] Mosaic picture %r written to %s" % (self.procId, tuple(canvas.shape), outfile))
        return 0

    # ---- tile grid (sfinder.py:1216-1384) ---------------------------------------------------------------------
    def create_tile_tasks(self):
        tileGrid = fits.generate_tiles(self.xmin, self.xmax, self.ymin, self.ymax, self.tileSizeX, self.tileSizeY,
                                       self.tileStepSizeX, self.tileStepSizeY)
        if tileGrid is None:
            return -1
        self.tasks_per_worker = [[] for _ in range(self.nproc)]
        workerCounter = 0
        for tid, coords in enumerate(tileGrid):                           # :1235-1251: round robin
            tileTask = TileTask(coords, self.model, self.config)
            tileTask.set_worker_id(workerCounter)
            tileTask.set_task_id(tid)
            tileTask.procId = self.procId
            tileTask.save_regions = self.save_tile_regions
            tileTask.save_json = self.save_tile_json
            tileTask.results_device = self.results_device
            tileTask.components_device = self.components_device
            self.tasks_per_worker[workerCounter].append(tileTask)
            workerCounter = 0 if workerCounter >= self.nproc - 1 else workerCounter + 1
        for i in range(len(self.tasks_per_worker)):                       # :1256-1293: neighbour lists, in this insertion order
            tasks_i = self.tasks_per_worker[i]
            for j, task in enumerate(tasks_i):
                for k in range(j + 1, len(tasks_i)):                      # first the later tasks of the same worker
                    task_N = tasks_i[k]
                    if task.is_task_tile_neighbor(task_N):
                        task.add_neighbor_info(task_N.tid, k, i)
                        task_N.add_neighbor_info(task.tid, j, i)
                for s in range(i + 1, len(self.tasks_per_worker)):        # then the tasks of the later workers
                    for t, task_N in enumerate(self.tasks_per_worker[s]):
                        if task.is_task_tile_neighbor(task_N):
                            task.add_neighbor_info(task_N.tid, t, s)
                            task_N.add_neighbor_info(task.tid, j, i)
        for tasks in self.tasks_per_worker:                               # :1372-1382
            if len(tasks) > self.config.MAX_NTASKS_PER_WORKER:
                logger.warning("[PROC %d] Too many tasks per worker exceeded (thr=%d)!" % (self.procId, self.config.MAX_NTASKS_PER_WORKER))
                return -1
        return 0

    # ---- output (sfinder.py:1389-1500), through the Analyzer's writers -------------------------------------
    def save(self):
        if self.procId != self.MASTER_ID:
            return
        writer = Analyzer(self.model, self.config)
        writer.results = {"image_id": self.image_id, "objs": self.sources["sources"]}
        if self.write_to_json:
            writer.write_json_results(self.outfile_json or 'catalog_' + str(self.image_id) + '.json')
        writer.make_ds9_regions(self.use_polygon_regions)
        self.sregions = writer.obj_regions
        if self.write_to_ds9:
            writer.write_ds9_regions(self.outfile_ds9 or 'ds9_' + str(self.image_id) + '.reg')
