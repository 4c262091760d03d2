"""Hand-built tile results for the tiled source finder: the scenarios of tests/golden/sfinder_merge.npz, the driver that
feeds them to an SFinder (this package's, or -- in tests/golden/make_sfinder_fixtures.py -- the reference's) and the codec of
the fixture.  Not a test module: imported by test_sfinder_cpu.py, test_sfinder_gpu.py and the fixture generator.

A scenario states what every tile's detector reported: (tile id, class id, score, pixels in mosaic coordinates).  The per-tile
result dict is built with Analyzer.make_json_results (pinned elsewhere), the tile info is added as TileTask.find_sources does,
then find_sources_at_edge runs per worker, the tile dicts are concatenated worker by worker (the gather) and merged."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden", "sfinder_merge.npz")
CLASS_NAMES = ["bkg", "sidelobe", "source", "galaxy"]


def make_config(img_path="mosaic.fits"):
    from caesar_mrcnn_amd.config import SDetectorConfig
    cfg = SDetectorConfig()
    cfg.NUM_CLASSES = len(CLASS_NAMES)
    cfg.CLASS_NAMES = list(CLASS_NAMES)
    cfg.IMG_PATH = img_path
    cfg.SPLIT_IMG_IN_TILES = True
    return cfg


def rect(y0, y1, x0, x1):
    """Pixels [y, x] of rows y0..y1 and columns x0..x1, both inclusive, raster order."""
    yy, xx = np.mgrid[y0:y1 + 1, x0:x1 + 1]
    return np.stack([yy.ravel(), xx.ravel()], axis=1)


def union(*parts):
    p = np.unique(np.concatenate(parts), axis=0)
    return p[np.lexsort((p[:, 1], p[:, 0]))]


def clip(pixels, tile):
    """What a perfect detector sees of `pixels` in tile (xmin, xmax, ymin, ymax): columns xmin..xmax-1, rows ymin..ymax-1."""
    xmin, xmax, ymin, ymax = tile
    keep = (pixels[:, 1] >= xmin) & (pixels[:, 1] < xmax) & (pixels[:, 0] >= ymin) & (pixels[:, 0] < ymax)
    return pixels[keep]


def tiles_of(sc):
    from caesar_mrcnn_amd import fits
    return fits.generate_tiles(sc["xmin"], sc["xmax"], sc["ymin"], sc["ymax"], sc["tile"], sc["tile"], sc["step"], sc["step"])


def _scenario(name, dets, step=1.0, workers=1, nx=768, ny=512, tile=256, sub=None):
    xmin, xmax, ymin, ymax = sub if sub else (0, nx - 1, 0, ny - 1)
    return {"name": name, "xmin": xmin, "xmax": xmax, "ymin": ymin, "ymax": ymax, "tile": tile, "step": step, "workers": workers,
            "dets": dets}


def grid_scenarios():
    """Scenario 1: tile grids of a 1000 x 800 mosaic (ids, workers, neighbour lists)."""
    out = []
    for step in (1.0, 0.5):
        for sub in (None, (100, 899, 50, 649)):
            for workers in (1, 3):
                name = "grid_s%d_%s_w%d" % (int(step * 10), "sub" if sub else "full", workers)
                out.append(_scenario(name, [], step=step, workers=workers, nx=1000, ny=800, sub=sub))
    return out


def merge_scenarios():
    """Scenarios 2-7.  768 x 512 mosaics, 256-tiles: step 1.0 -> 3 x 2 tiles (id = 3 row + col), step 0.5 -> 6 x 4 tiles
    (id = 6 row + col; x spans 0, 128, .. 640; y spans 0, 128, 256, 384)."""
    out = []
    t10 = tiles_of(_scenario("", []))

    def seen(pixels, tiles, ids, cls, score):
        return [(tid, cls, score, clip(pixels, tiles[tid])) for tid in ids]

    # 2a: one source cut in two by the vertical border x = 256
    out.append(_scenario("vsplit", seen(rect(100, 120, 240, 270), t10, (0, 1), 2, 0.95)))
    # 2b: one source cut in four at the corner (256, 256): component of four
    out.append(_scenario("corner4", seen(rect(250, 262, 248, 265), t10, (0, 1, 3, 4), 3, 0.9), workers=3))
    # 3a: contact only through one diagonal pixel pair (dx = dy = 1) -> merged
    out.append(_scenario("diag", [(0, 2, 0.9, rect(50, 60, 250, 255)), (1, 2, 0.8, rect(61, 70, 256, 260))]))
    # 3b: distance exactly 2 in x (rows 150..160) and in y (rows 149 / 151), boxes overlapping -> not merged
    out.append(_scenario("gap2", [(1, 2, 0.9, union(rect(150, 160, 506, 510), rect(140, 149, 506, 511))),
                                  (2, 2, 0.8, rect(151, 160, 512, 516))]))
    # 4: interlocking L-shapes in the overlap of two step-0.5 tiles: boxes overlap, pixels never closer than 8 -> not merged
    la = union(rect(20, 80, 150, 152), rect(78, 80, 150, 220))
    lb = union(rect(20, 22, 160, 230), rect(20, 70, 228, 230))
    out.append(_scenario("interlock", [(0, 2, 0.9, la), (1, 3, 0.85, lb)], step=0.5))
    # 5: chain a-b-c over three tiles, a and c far apart, three classes / scores, the largest member (b) not the last one
    chain = [(0, 1, 0.9, rect(200, 210, 230, 255)), (1, 2, 0.8, rect(200, 210, 256, 511)), (2, 3, 0.75, rect(200, 210, 512, 520))]
    out.append(_scenario("chain", chain))
    out.append(_scenario("chain_w3", chain, workers=3))
    # 6: step 0.5 -- one source seen by two overlapping tiles and one by four, every view slightly different
    p2 = [(0, 2, 0.9, rect(30, 50, 140, 170)), (1, 2, 0.85, union(rect(31, 51, 141, 171), rect(40, 42, 172, 173)))]
    q4 = [(0, 3, 0.9, rect(140, 170, 140, 170)), (1, 3, 0.8, rect(141, 171, 139, 169)),
          (6, 3, 0.7, union(rect(140, 170, 141, 171), rect(171, 172, 150, 151))), (7, 3, 0.95, rect(139, 169, 140, 170))]
    out.append(_scenario("overlap", p2 + q4, step=0.5))
    out.append(_scenario("overlap_w3", p2 + q4, step=0.5, workers=3))
    # 7a: an edge source that touches only the mosaic's outer frame, next to an interior one; tiles 1..5 report nothing
    out.append(_scenario("frame", [(0, 2, 0.9, rect(0, 10, 50, 60)), (0, 1, 0.8, rect(100, 110, 100, 120))]))
    # 7b: no edge source at all
    out.append(_scenario("noedge", [(0, 2, 0.9, rect(100, 110, 100, 120)), (4, 3, 0.8, rect(300, 320, 300, 330))]))
    # everything of step 1.0 in one mosaic, three workers (the scenarios above sit at distinct places)
    allin = []
    for sc in out:
        if sc["step"] == 1.0 and sc["name"] not in ("chain_w3", "noedge"):
            allin += sc["dets"]
    out.append(_scenario("all_w3", sorted(allin, key=lambda d: d[0]), workers=3))
    return out


def tile_result(cfg, tile, tid, dets):
    """The Analyzer's result dict of one tile for detections [(class id, score, mosaic pixels)] (empty dict: none)."""
    from caesar_mrcnn_amd import utils
    from caesar_mrcnn_amd.analyze import Analyzer
    if not dets:
        return {}
    xmin, xmax, ymin, ymax = tile
    an = Analyzer(None, cfg)
    an.image = np.zeros((ymax - ymin, xmax - xmin, 3), np.uint8)
    an.image_id, an.image_xmin, an.image_ymin, an.obj_name_tag = "mosaic", xmin, ymin, "t%d" % tid
    an.masks_final, an.class_ids_final, an.scores_final, an.bboxes = [], [], [], []
    for cls, score, pixels in dets:
        m = np.zeros(an.image.shape[:2], np.int64)
        m[pixels[:, 0] - ymin, pixels[:, 1] - xmin] = 1
        an.masks_final.append(m)
        an.class_ids_final.append(cls)
        an.scores_final.append(score)
        an.bboxes.append(utils.extract_bboxes(m.astype(bool)[:, :, None])[0])
    an.make_json_results()
    return an.results


def drive(sf, sc, cfg, merge=None):
    """Feed scenario `sc` to SFinder-like `sf` (attribute names of the reference); returns (grid, sources)."""
    sf.nproc = sc["workers"]
    sf.xmin, sf.xmax, sf.ymin, sf.ymax = sc["xmin"], sc["xmax"], sc["ymin"], sc["ymax"]
    sf.tileSizeX = sf.tileSizeY = sc["tile"]
    sf.tileStepSizeX = sf.tileStepSizeY = sc["step"]
    sf.procId = 0
    assert sf.create_tile_tasks() == 0
    grid = [[(t.tid, t.wid, tuple(int(v) for v in t.coords), list(t.neighborTaskId), list(t.neighborTaskIndex), list(t.neighborWorkerId))
             for t in tasks] for tasks in sf.tasks_per_worker]
    per_tile = {}
    for tid, cls, score, pixels in sc["dets"]:
        per_tile.setdefault(tid, []).append((cls, score, pixels))
    for w, tasks in enumerate(sf.tasks_per_worker):
        sf.procId = w
        for j, t in enumerate(tasks):
            res = tile_result(cfg, t.coords, t.tid, per_tile.get(t.tid, []))
            if res:                                           # TileTask.find_sources (sfinder.py:230-239)
                res.update({"workerId": t.wid, "tileId": t.tid, "neighborTileIds": t.neighborTaskId, "xmin": t.ix_min,
                            "xmax": t.ix_max, "ymin": t.iy_min, "ymax": t.iy_max})
            t.det_sources = res
            sf.find_sources_at_edge(j)
    sf.procId = 0
    sf.tile_sources = {"sources": [t.det_sources for tasks in sf.tasks_per_worker for t in tasks if t.det_sources]}
    (merge or sf.merge_edge_sources)()
    return grid, sf.sources["sources"]


def canon(sources):
    """Plain Python values (the reference leaves NumPy integers in merged boxes)."""
    out = []
    for s in sources:
        out.append({"name": str(s["name"]), "x1": int(s["x1"]), "x2": int(s["x2"]), "y1": int(s["y1"]), "y2": int(s["y2"]),
                    "edge": bool(s["edge"]), "merged": bool(s["merged"]), "class_id": int(s["class_id"]),
                    "class_name": str(s["class_name"]), "score": float(s["score"]),
                    "pixels": [[int(p[0]), int(p[1])] for p in s["pixels"]],
                    "vertexes": [[[float(v[0]), float(v[1])] for v in c] for c in s["vertexes"]]})
    return out


# ---- fixture codec ------------------------------------------------------------------------------------------
def _offsets(lengths):
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)


def encode(name, sc, grid, sources, out):
    k = name + "__"
    out[k + "params"] = np.array([sc["xmin"], sc["xmax"], sc["ymin"], sc["ymax"], sc["tile"], sc["workers"]], np.int32)
    out[k + "step"] = np.array(sc["step"], np.float64)
    # inputs: the detections, masks bit-packed in their boxes
    boxes, chunks = [], []
    for tid, cls, score, p in sc["dets"]:
        y0, x0 = p.min(axis=0)
        h, w = p.max(axis=0) - (y0, x0) + 1
        m = np.zeros((h, w), np.uint8)
        m[p[:, 0] - y0, p[:, 1] - x0] = 1
        chunks.append(np.packbits(m.ravel(), bitorder="little"))
        boxes.append((tid, cls, x0, y0, w, h))
    out[k + "det_boxes"] = np.array(boxes, np.int32).reshape(-1, 6)
    out[k + "det_scores"] = np.array([d[2] for d in sc["dets"]], np.float64)
    out[k + "det_mask_offsets"] = _offsets([c.size for c in chunks])
    out[k + "det_masks"] = np.concatenate(chunks) if chunks else np.zeros(0, np.uint8)
    # outputs: the grid ...
    flat = [t for tasks in grid for t in tasks]
    out[k + "grid_tiles"] = np.array([(t[0], t[1]) + t[2] for t in flat], np.int32).reshape(-1, 6)
    out[k + "grid_nb_offsets"] = _offsets([len(t[3]) for t in flat])
    out[k + "grid_nb"] = np.array([v for t in flat for v in zip(t[3], t[4], t[5])], np.int32).reshape(-1, 3)
    # ... and the catalogue
    src = canon(sources)
    out[k + "names"] = np.array([s["name"] for s in src], dtype="U16")
    out[k + "class_names"] = np.array([s["class_name"] for s in src], dtype="U32")
    out[k + "ints"] = np.array([(s["x1"], s["x2"], s["y1"], s["y2"], s["class_id"], s["edge"], s["merged"]) for s in src],
                               np.int32).reshape(-1, 7)
    out[k + "scores"] = np.array([s["score"] for s in src], np.float64)
    out[k + "pix_offsets"] = _offsets([len(s["pixels"]) for s in src])
    out[k + "pixels"] = np.array([p for s in src for p in s["pixels"]], np.int16).reshape(-1, 2)
    contours = [c for s in src for c in s["vertexes"]]
    out[k + "contour_offsets"] = _offsets([len(s["vertexes"]) for s in src])
    out[k + "point_offsets"] = _offsets([len(c) for c in contours])
    out[k + "points"] = np.array([v for c in contours for v in c], np.float64).reshape(-1, 2)


def decode(name, z):
    """(scenario, grid, sources) of one fixture entry, in the shapes drive() / canon() return."""
    k = name + "__"
    xmin, xmax, ymin, ymax, tile, workers = (int(v) for v in z[k + "params"])
    dets = []
    mo, packed = z[k + "det_mask_offsets"], z[k + "det_masks"]
    for d, (tid, cls, x0, y0, w, h) in enumerate(z[k + "det_boxes"].tolist()):
        m = np.unpackbits(packed[mo[d]:mo[d + 1]], bitorder="little")[:h * w].reshape(h, w)
        dets.append((tid, cls, float(z[k + "det_scores"][d]), np.argwhere(m) + (y0, x0)))
    sc = {"name": name, "xmin": xmin, "xmax": xmax, "ymin": ymin, "ymax": ymax, "tile": tile, "step": float(z[k + "step"]),
          "workers": workers, "dets": dets}
    grid = [[] for _ in range(workers)]
    nbo, nb = z[k + "grid_nb_offsets"], z[k + "grid_nb"]
    for t, row in enumerate(z[k + "grid_tiles"].tolist()):
        n = nb[nbo[t]:nbo[t + 1]]
        grid[row[1]].append((row[0], row[1], tuple(row[2:]), n[:, 0].tolist(), n[:, 1].tolist(), n[:, 2].tolist()))
    po, pix = z[k + "pix_offsets"], z[k + "pixels"].astype(np.int64)
    co, pto, pts = z[k + "contour_offsets"], z[k + "point_offsets"], z[k + "points"]
    sources = []
    for s, (x1, x2, y1, y2, cid, edge, merged) in enumerate(z[k + "ints"].tolist()):
        sources.append({"name": str(z[k + "names"][s]), "x1": x1, "x2": x2, "y1": y1, "y2": y2, "edge": bool(edge),
                        "merged": bool(merged), "class_id": cid, "class_name": str(z[k + "class_names"][s]),
                        "score": float(z[k + "scores"][s]), "pixels": pix[po[s]:po[s + 1]].tolist(),
                        "vertexes": [pts[pto[c]:pto[c + 1]].tolist() for c in range(co[s], co[s + 1])]})
    return sc, grid, sources


def fixture_names(z):
    return sorted({key.split("__")[0] for key in z.files})


# ---- planted mosaics for the tiling-invariance test -------------------------------------------------------
def planted_mosaic(seed, nx=768, ny=512, n_try=400, rmin=2, rmax=25):
    """Label map [ny, nx] int32 (0 = sky, k = source k) of random ellipses no two of which are 8-adjacent -- kept two
    dilations apart, and asserted.  Returns (labels, n_sources)."""
    rng = np.random.RandomState(seed)
    labels = np.zeros((ny, nx), np.int32)
    blocked = np.zeros((ny, nx), bool)
    yy, xx = np.mgrid[0:ny, 0:nx]
    n = 0
    for _ in range(n_try):
        cy, cx = rng.uniform(0, ny), rng.uniform(0, nx)
        a, b, th = rng.uniform(rmin, rmax), rng.uniform(rmin, rmax), rng.uniform(0, np.pi)
        u = (xx - cx) * np.cos(th) + (yy - cy) * np.sin(th)
        v = -(xx - cx) * np.sin(th) + (yy - cy) * np.cos(th)
        m = (u / a) ** 2 + (v / b) ** 2 <= 1.0
        if m.sum() < 4 or (m & blocked).any():
            continue
        n += 1
        labels[m] = n
        grown = m.copy()
        for _ in range(2):                                    # two 3 x 3 dilations
            g = np.pad(grown, 1)
            grown = np.zeros_like(grown)
            for dy in (0, 1, 2):
                for dx in (0, 1, 2):
                    grown |= g[dy:dy + ny, dx:dx + nx]
        blocked |= grown
    # no two distinct sources 8-adjacent: every 2 x 2 window and every row / column neighbour pair holds at most one label
    for a, b in ((labels[:, :-1], labels[:, 1:]), (labels[:-1, :], labels[1:, :]), (labels[:-1, :-1], labels[1:, 1:]),
                 (labels[:-1, 1:], labels[1:, :-1])):
        assert not np.any((a != b) & (a > 0) & (b > 0)), "planted sources touch"
    return labels, n


class LabelMapModel(object):
    """Stand-in for MaskRCNN on the SFinder path: answers a tile (the label map itself, read with every stretch off) with one
    mask per label present in it, class 1, score 0.99."""

    def __init__(self, config):
        self.config = config

    def detect(self, images, verbose=0):
        from caesar_mrcnn_amd import utils
        tile = np.asarray(images[0])
        if tile.ndim == 3:
            tile = tile[:, :, 0]
        ids = [v for v in np.unique(tile) if v > 0]             # (labels may arrive rescaled: distinct values are what counts)
        masks = np.stack([tile == k for k in ids], axis=-1) if ids else np.zeros(tile.shape + (0,), bool)
        return [{"rois": utils.extract_bboxes(masks), "class_ids": np.ones(len(ids), np.int32),
                 "scores": np.full(len(ids), 0.99, np.float32), "masks": masks}]


def label_map_config(path):
    cfg = make_config(path)
    cfg.ZSCALE_STRETCH = cfg.NORMALIZE_IMG = cfg.IMG_TO_RGB = cfg.IMG_TO_UINT8 = False
    cfg.BIAS_CONTRAST_STRETCH = False
    cfg.CLASS_NAMES, cfg.NUM_CLASSES = ["bkg", "source"], 2
    cfg.TILE_XSIZE = cfg.TILE_YSIZE = 256
    cfg.SCORE_THR, cfg.IOU_THR = 0.7, 0.6
    cfg.IMG_XMIN = cfg.IMG_XMAX = cfg.IMG_YMIN = cfg.IMG_YMAX = -1
    return cfg
