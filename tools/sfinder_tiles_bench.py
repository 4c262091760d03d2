"""The front of a tiled source-finder run (SFinder.run_parallel up to the gather): the tile-at-a-time loop -- one file read, host
stretch and batch-1 detect per tile, tile_batch = 0, the loop of the commit before the batched front end, which that setting
leaves untouched -- against the batched, device-resident front end at tile_batch = 1, 4 and 8, on a seeded synthetic mosaic.
Prints one JSON object and writes it with --out (default profiles/sfinder_tiles_bench.json).

    python tools/sfinder_tiles_bench.py [--sizes 2304[,4352]] [--max-instances 10] [--tile 512] [--step 0.5] [--backbone resnet101] [--imgsize 256]
                                        [--reps 3] [--batches 1,4,8] [--bias-contrast BIAS,CONTRAST] [--no-uint8 | --gray] [--out FILE]

One process, one GPU, one set of seeded weights: a model per batch size (1 serves the loop and tile_batch = 1), every model
warmed on a few tiles first (library load, graph capture, allocator).  Per mosaic size:
  wall     the wall time from the header read to the last tile's edge flags (run_parallel up to the gather; the batched front
           end's one read of the file is inside), perf_counter with the device synchronised before and after, the variants
           alternating within every repetition; median of --reps;
  stages   from ONE further run per variant that synchronises after every stage (so its sum is not the wall time):
           read_cut  (loop: fits.read_primary_hdu per tile + the cut; batched: the one read + upload of the plane),
           stretch   (loop: the rest of fits.read_fits on the host; batched: ops.fits_tiles_to_image),
           mold_graph (MaskRCNN.detect up to the end of the inference graph), unmold (the rest of detect),
           analyzer  (Analyzer.accept_detection: mask selection, JSON, regions), edge (find_sources_at_edge);
  equal    the tile_batch = 1 catalogue of tile results equals the loop's (same model, same bytes); larger batches are not
           compared (a network's results may differ between batch sizes in the last bits): their detection counts are listed.
The weights are random (seeded): such a model fills whatever DETECTION_MAX_INSTANCES allows, and the Analyzer's host statement
then costs seconds per 512 x 512 tile at the default cap of 100, so the cap is --max-instances (default 10); the
number of objects per tile, which sets the Analyzer's share, is reported."""
import argparse
import json
import logging
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def synth_mosaic(size, seed):
    """[size, size] float32: unit noise + one Gaussian blob per 128 x 128 cell on average, a few NaN strips."""
    rng = np.random.RandomState(seed)
    img = rng.normal(0.0, 1.0, (size, size)).astype(np.float32)
    n = (size // 128) ** 2
    r = 24
    yy, xx = np.mgrid[-r:r + 1, -r:r + 1]
    for _ in range(n):
        cy, cx = rng.randint(r, size - r, 2)
        sy, sx = rng.uniform(2.0, 7.0, 2)
        img[cy - r:cy + r + 1, cx - r:cx + r + 1] += (rng.uniform(10.0, 200.0) * np.exp(-0.5 * ((yy / sy) ** 2 + (xx / sx) ** 2))).astype(np.float32)
    for k in range(4):
        y = rng.randint(0, size - 8)
        img[y:y + 3, rng.randint(0, size // 2):] = np.nan
    return img


class Stages(object):
    """Accumulates seconds per stage name; wrap(f, name) times f with a device synchronise after it when `sync` is set."""

    def __init__(self, torch):
        self.torch, self.t, self.sync = torch, {}, False

    def add(self, name, dt):
        self.t[name] = self.t.get(name, 0.0) + dt

    def wrap(self, f, name, minus=()):
        def g(*a, **k):
            if not self.sync:
                return f(*a, **k)
            before = [self.t.get(m, 0.0) for m in minus]
            t0 = time.perf_counter()
            out = f(*a, **k)
            self.torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            self.add(name, dt - sum(self.t.get(m, 0.0) - b for m, b in zip(minus, before)))     # nested stages are not counted twice
            return out
        return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="2304")
    ap.add_argument("--max-instances", type=int, default=10,
                    help="DETECTION_MAX_INSTANCES: random weights fill whatever the cap allows, and the Analyzer's host statement "
                         "costs seconds per tile at the default 100")
    ap.add_argument("--tile", type=int, default=512)
    ap.add_argument("--step", type=float, default=0.5)
    ap.add_argument("--backbone", default="resnet101")
    ap.add_argument("--imgsize", type=int, default=256)
    ap.add_argument("--batches", default="1,4,8")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--bias-contrast", default=None,
                    help="BIAS,CONTRAST: BIAS_CONTRAST_STRETCH on (after zscale) with these values in every variant; the batched front end "
                         "then runs ops.fits_tiles_to_image")
    ap.add_argument("--no-uint8", action="store_true", help="IMG_TO_UINT8 off in every variant: float32 RGB tiles (run.py --no_uint8)")
    ap.add_argument("--gray", action="store_true",
                    help="a gray-level model and gray tiles in every variant (run.py --grayimg): one input channel, IMG_TO_RGB off")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sfinder_tiles_bench.json"))
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a GPU: a CPU run gives no time"
    logging.getLogger("mrcnn").setLevel(logging.CRITICAL)
    from caesar_mrcnn_amd import fits
    from caesar_mrcnn_amd.analyze import Analyzer
    from caesar_mrcnn_amd.config import run_py_config
    from caesar_mrcnn_amd.model import MaskRCNN
    from caesar_mrcnn_amd.sfinder import SFinder
    dev = torch.device("cuda:0")
    batches = [int(v) for v in args.batches.split(",")]
    st = Stages(torch)
    t_start = time.perf_counter()

    def say(what):
        sys.stderr.write("[sfinder_tiles_bench %7.1f s] %s\n" % (time.perf_counter() - t_start, what))
        sys.stderr.flush()
    tmp = tempfile.mkdtemp(prefix="sfinder_tiles_bench_")

    def config(path, n):
        cfg = run_py_config(num_classes=4, imgsize=args.imgsize, backbone=args.backbone, mode="inference")
        cfg.IMAGES_PER_GPU = n
        cfg.DETECTION_MAX_INSTANCES = args.max_instances
        cfg.CLASS_NAMES = ["bkg", "sidelobe", "source", "galaxy"]
        cfg.IMG_PATH = path
        cfg.SPLIT_IMG_IN_TILES = True
        cfg.TILE_XSIZE = cfg.TILE_YSIZE = args.tile
        cfg.TILE_XSTEP = cfg.TILE_YSTEP = args.step
        cfg.MAX_NTASKS_PER_WORKER = 1 << 30
        cfg.IMG_XMIN = cfg.IMG_XMAX = cfg.IMG_YMIN = cfg.IMG_YMAX = -1
        if args.no_uint8:
            cfg.IMG_TO_UINT8 = False
        if args.gray:
            cfg.IMAGE_CHANNEL_COUNT, cfg.MEAN_PIXEL, cfg.IMG_TO_RGB = 1, 0, False
            cfg.IMAGE_SHAPE = np.array([args.imgsize, args.imgsize, 1])
        if args.bias_contrast:
            cfg.BIAS_CONTRAST_STRETCH = True
            cfg.IMG_BIAS, cfg.IMG_CONTRAST = [float(v) for v in args.bias_contrast.split(",")]
        return cfg

    models = {}
    for n in sorted(set([1] + batches)):
        m = MaskRCNN("inference", config("", n), os.path.join(tmp, "logs"), device=dev, seed=args.seed)
        real_detect = m.detect

        def detect(images, verbose=0, _real=real_detect):
            if not st.sync:
                return _real(images, verbose)
            tm = {}
            out = _real(images, verbose, timing=tm)
            st.add("mold_graph", tm["graph_done"] - tm["start"])
            st.add("unmold", tm["end"] - tm["graph_done"])
            return out
        m.detect = detect
        models[n] = m
        say("model for batches of %d built" % n)
    # the stage seams
    fits.read_primary_hdu = st.wrap(fits.read_primary_hdu, "read_cut")
    fits.read_fits = st.wrap(fits.read_fits, "stretch", minus=("read_cut",))
    Analyzer.accept_detection = st.wrap(Analyzer.accept_detection, "analyzer")
    SFinder.find_sources_at_edge = st.wrap(SFinder.find_sources_at_edge, "edge")
    SFinder._plane_device = st.wrap(SFinder._plane_device, "read_cut")
    SFinder.prepare_tile_images = st.wrap(SFinder.prepare_tile_images, "stretch", minus=("read_cut",))

    def tile_loop(path, batch, limit=None):
        """run_parallel up to the gather, on one rank: returns (seconds, SFinder)."""
        cfg = config(path, max(batch, 1))
        sf = SFinder(models[max(batch, 1)], cfg)
        sf.tile_batch = batch
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        assert sf.set_img_size_params() == 0 and sf.create_tile_tasks() == 0      # (the batched front end reads the file here, once)
        tasks = sf.tasks_per_worker[0][:limit]                      # (a prefix: the neighbour indices of the edge flags stay valid)
        if batch:
            sf._run_tasks_batched(tasks)
        else:
            for j, task in enumerate(tasks):
                sf._run_task(j, task, task.find_sources)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        sf._drop_plane()
        return dt, sf

    def tile_results(sf):
        return [(t.tid, json.dumps(t.det_sources.get("objs", []), sort_keys=True)) for t in sf.tasks_per_worker[0]]

    res = {"device": torch.cuda.get_device_name(0), "backbone": args.backbone, "imgsize": args.imgsize, "tile": args.tile, "step": args.step,
           "reps": args.reps, "weights": "random, seed %d" % args.seed, "detection_max_instances": args.max_instances, "hip_graph": True,
           "bias_contrast": [float(v) for v in args.bias_contrast.split(",")] if args.bias_contrast else None,
           "tiles_kind": "float32 gray" if args.gray else ("float32 RGB" if args.no_uint8 else "uint8 RGB"), "mosaics": []}
    variants = [0] + batches
    for size in [int(v) for v in args.sizes.split(",")]:
        path = os.path.join(tmp, "mosaic_%d.fits" % size)
        fits.write_fits(path, synth_mosaic(size, args.seed), {"BUNIT": "JY/BEAM"})
        for b in variants:                                         # warm-up: every model, both front ends, full and short tiles
            say("warm-up, tile_batch %d: %.2f s" % (b, tile_loop(path, b, limit=2 * max(b, 1) + 1)[0]))
        wall = {b: [] for b in variants}
        last = {}
        for _ in range(args.reps):
            for b in variants:
                dt, sf = tile_loop(path, b)
                wall[b].append(dt)
                last[b] = sf
                say("%d x %d, tile_batch %d: %.2f s" % (size, size, b, dt))
        ntiles = len(last[0].tasks_per_worker[0])
        entry = {"mosaic": [size, size], "file_mb": round(os.path.getsize(path) / 2.0 ** 20, 1), "tiles": ntiles, "variants": {}}
        if 1 in last:
            entry["tile_batch_1_equals_loop"] = tile_results(last[1]) == tile_results(last[0])
            assert entry["tile_batch_1_equals_loop"], "tile_batch = 1 and the loop disagree"
        base = float(np.median(wall[0]))
        for b in variants:
            st.t, st.sync = {}, True
            staged, _ = tile_loop(path, b)
            st.sync = False
            say("%d x %d, tile_batch %d, synchronised stages: %.2f s" % (size, size, b, staged))
            med = float(np.median(wall[b]))
            dets = [len(t.det_sources.get("objs", [])) for t in last[b].tasks_per_worker[0]]
            entry["variants"]["loop" if b == 0 else "tile_batch_%d" % b] = {
                "wall_s": [round(v, 3) for v in wall[b]], "wall_median_s": round(med, 3), "ms_per_tile": round(1e3 * med / ntiles, 2),
                "loop_over_this": round(base / med, 2),
                "stages_ms_per_tile_synchronised_run": {k: round(1e3 * v / ntiles, 3) for k, v in sorted(st.t.items())},
                "synchronised_run_s": round(staged, 3), "objects_per_tile_mean": round(float(np.mean(dets)), 2),
                "objects_total": int(np.sum(dets))}
        res["mosaics"].append(entry)
        os.remove(path)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
