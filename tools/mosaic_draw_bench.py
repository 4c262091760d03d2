"""The overview picture of a mosaic (SFinder.draw_mosaic_results) on the synthetic mosaic of tools/sfinder_bench.py
with the catalogue of tools/sfinder_params_bench.py; prints one JSON object (and writes it with --out).

    python tools/mosaic_draw_bench.py [--grid 16] [--tile 512] [--sources 900] [--reps 3] [--out FILE] [--no-large]

Timed on the same machine in the same run, device form and host statement alternating, medians of --reps runs after one warm-up
run of each; the two canvases are compared byte for byte first and nothing is reported unless they are equal:
  (a) the host statement: fits.mosaic_overview_host, source_planes_host, draw.render_host, PNG encode;
  (b) the device form end to end with its stages (plane upload, overview, planes, render, download, PNG encode), the device
      synchronised between stages;
  (c) the launches alone from device events, inputs resident: the four of the overview, the two of the planes, the raster.
The overview reads the plane twice (statistics, pixels): `overview_read_GBps` is 2 * 4 ny nx bytes over its event time and
`overview_share_of_hbm` that rate over 6300 GB/s (what streaming kernels reach on the MI355X).  A 4352 x 4352 plane (76 MB) fits
the 256 MiB Infinity Cache, so its second pass may be served on the die; --no-large skips the 16384 x 16384 plane (1 GiB,
generated on the device) that cannot.  The small case is the 384 x 320 mosaic of the tests with 5 sources."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from sfinder_bench import plant                   # noqa: E402
from sfinder_params_bench import catalogue        # noqa: E402

HBM_GBPS = 6300.0


def finder(path, sources):
    from caesar_mrcnn_amd.config import SDetectorConfig
    from caesar_mrcnn_amd.sfinder import SFinder
    cfg = SDetectorConfig()
    cfg.IMG_PATH = path
    cfg.IMG_XMIN = cfg.IMG_XMAX = cfg.IMG_YMIN = cfg.IMG_YMAX = -1
    sf = SFinder(None, cfg)
    sf.image_id = os.path.splitext(os.path.basename(path))[0]
    sf.sources = {"sources": sources}
    return sf


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=16)
    ap.add_argument("--tile", type=int, default=512)
    ap.add_argument("--sources", type=int, default=900)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--no-large", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import logging
    logging.getLogger("mrcnn").setLevel(logging.ERROR)
    import torch
    from caesar_mrcnn_amd import draw, fits, ops
    from caesar_mrcnn_amd.sfinder import pack_sources
    assert torch.cuda.is_available(), "needs a GPU"
    tmp = tempfile.mkdtemp(prefix="mosaic_draw_bench_")
    dev = torch.device("cuda", torch.cuda.current_device())

    def measure(sf, tag):
        png = os.path.join(tmp, tag + ".png")
        sf.mosaic_outfile = png
        sf._drop_plane()
        want = sf.render_mosaic(False)
        sf._drop_plane()
        got = sf.render_mosaic(True)
        assert np.array_equal(got, want), "device and host canvases differ"
        ms = {"device": [], "host": []}
        stages = {}
        for rep in range(args.reps + 1):                       # the first run of each warms up
            for name, device in (("device", True), ("host", False)):
                sf._drop_plane()                                # every run reads (and uploads) the plane anew
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                assert sf.draw_mosaic_results(device) == 0
                torch.cuda.synchronize()
                if rep:
                    ms[name].append(1e3 * (time.perf_counter() - t0))
                stages[name] = dict(sf.mosaic_timing)
        ny, nx, k, h, w, scale = sf._mosaic_geometry()
        out = {"mosaic": [ny, nx], "shrink": k, "frame": [h, w], "scale": scale, "canvas": list(want.shape), "sources": len(sf.sources["sources"]),
               "canvases_equal": True, "png_bytes": os.path.getsize(png),
               "host_ms": [round(v, 2) for v in ms["host"]], "device_ms": [round(v, 2) for v in ms["device"]],
               "host_median_ms": round(float(np.median(ms["host"])), 2), "device_median_ms": round(float(np.median(ms["device"])), 2),
               "device_stages_last_run": stages["device"], "host_stages_last_run": stages["host"]}
        out["host_over_device"] = round(out["host_median_ms"] / out["device_median_ms"], 2)
        # the launches alone, inputs resident
        plane_t, big = sf._plane_device()
        pool, desc = pack_sources(sf._mosaic_pixel_lists())
        pool_t, desc_t = ops.tile_upload(pool, desc, dev)
        kern = {"overview": [], "planes": [], "render": []}
        for _ in range(10):
            t = {}
            frame = ops.mosaic_overview(plane_t, k, sf._mosaic_contrast(), big_endian=big, timing=t)
            planes = ops.sources_to_planes(pool_t, desc_t, k, h, w, timing=t)
            scene = sf._mosaic_scene_of(None, None, planes.box.cpu().numpy(), scale)
            ops.draw_overlay(frame, planes, draw.device_tables(scene), scale, timing=t)
            kern["overview"].append(t["overview_kernels_ms"])
            kern["planes"].append(t["planes_kernels_ms"])
            kern["render"].append(t["render_kernel_ms"])
        out["kernels_ms"] = {n: round(float(np.median(v)), 4) for n, v in kern.items()}
        rate = 2 * 4.0 * ny * nx / (out["kernels_ms"]["overview"] * 1e-3) / 1e9
        out["overview_read_GBps"] = round(rate, 1)
        out["overview_share_of_hbm"] = round(rate / HBM_GBPS, 3)
        out["plane_bytes"] = 4 * ny * nx
        out["plane_words"] = int(planes.words.numel())
        sf._drop_plane()
        return out

    res = {"reps": args.reps, "hbm_GBps_assumed": HBM_GBPS}
    # the mosaic and catalogue of DESIGN 4.8, with a frame of NaNs around it as mosaics have
    size = (args.grid + 1) * args.tile // 2
    labels, _ = plant(size, args.sources, args.seed)
    img, sources = catalogue(labels, args.seed)
    img[:48], img[-48:], img[:, :48], img[:, -48:] = np.nan, np.nan, np.nan, np.nan
    path = os.path.join(tmp, "big.fits")
    fits.write_fits(path, img)
    res["full"] = measure(finder(path, sources), "big")
    del img, labels

    # the small mosaic of the tests with 5 sources
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import sfinder_tiles_cases as tiles
    small = os.path.join(tmp, "small.fits")
    tiles.write_mosaic(small)
    rng = np.random.RandomState(args.seed)
    few = []
    for i in range(5):
        cy, cx = rng.randint(20, tiles.NY - 20), rng.randint(20, tiles.NX - 20)
        few.append({"name": "S%d" % (i + 1), "class_name": "source", "score": 0.9, "merged": False,
                    "pixels": [[y, x] for y in range(cy - 4, cy + 5) for x in range(cx - 6, cx + 7)]})
    res["small"] = measure(finder(small, few), "small")

    if not args.no_large:
        # 16384 x 16384 (1 GiB, 262144 chunks, 256 super-chunks): the overview alone, from events
        n = 16384
        plane = torch.randn((n, n), dtype=torch.float32, device=dev)
        plane[:512] = float("nan")
        plane[:, -512:] = float("nan")
        plane[5000:5003, 100:9000] = float("nan")
        ms = []
        for _ in range(6):
            t = {}
            ops.mosaic_overview(plane, 16, 0.25, timing=t)
            ms.append(t["overview_kernels_ms"])
        med = float(np.median(ms[1:]))
        rate = 2 * 4.0 * n * n / (med * 1e-3) / 1e9
        res["large_overview"] = {"plane": [n, n], "shrink": 16, "overview_kernels_ms": [round(v, 3) for v in ms[1:]],
                                 "median_ms": round(med, 3), "overview_read_GBps": round(rate, 1),
                                 "overview_share_of_hbm": round(rate / HBM_GBPS, 3),
                                 "workspace_bytes": int(ops._hip.lib().mrcnn_mosaic_overview_workspace(n, n))}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
