"""The source-parameter step of the tiled source finder (SFinder.compute_sources_params) on the synthetic mosaic of
tools/sfinder_bench.py with Gaussian flux planted under its labels; prints one JSON object (and writes it with --out).

    python tools/sfinder_params_bench.py [--grid 16] [--tile 512] [--sources 900] [--reps 5] [--out FILE] [--no-sweep]

The catalogue is one entry per planted label (boxes as the Analyzer writes them: x2 / y2 exclusive).  Timed, on the same machine
in the same run, every run from a cold image cache of the SFinder (so each includes reading the file):
  (a) the host statement for every source (params_device off) -- the yardstick;
  (b) the device path end to end (read, upload, pack, launch, download, dicts), device synchronised before and after, with its
      stages;
  (c) the launch alone (device events, inputs resident).
The two catalogues are compared first with the bounds of the tests (tests/sfinder_params_cases.assert_params_close); nothing is
reported unless they agree.  The sweep repeats (a) and (b) on the first 1, 4 and 116 sources
of the big mosaic and on a small one, for the break-even of SFinder.PARAMS_DEVICE_MIN_SOURCES.  Medians of --reps runs after one
warm-up run."""
import argparse
import copy
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

sys.path.insert(0, os.path.join(ROOT, "tests"))
import sfinder_params_cases as cases              # noqa: E402  (the float64 brute force and the derived comparison bounds)


def catalogue(labels, seed):
    """(image float32, sources): noise of sigma 1e-4 plus, under every label, a Gaussian of peak 1e-3 .. 1e-1 at its centroid."""
    rng = np.random.RandomState(seed)
    img = rng.normal(0.0, 1e-4, labels.shape)
    ys, xs = np.nonzero(labels)
    ids = labels[ys, xs]
    order = np.argsort(ids, kind="stable")
    ys, xs, ids = ys[order], xs[order], ids[order]
    cuts = np.flatnonzero(np.diff(ids)) + 1
    sources = []
    for k, (y, x) in enumerate(zip(np.split(ys, cuts), np.split(xs, cuts))):
        s2 = max(y.size / 9.0, 1.0)
        img[y, x] += 10.0 ** rng.uniform(-3, -1) * np.exp(-0.5 * ((y - y.mean()) ** 2 + (x - x.mean()) ** 2) / s2)
        sources.append({"name": "S%d" % (k + 1), "x1": int(x.min()), "x2": int(x.max()) + 1, "y1": int(y.min()), "y2": int(y.max()) + 1,
                        "class_id": 1, "class_name": "source", "score": 0.9, "edge": False, "merged": False,
                        "pixels": np.stack([y, x], axis=1).tolist(), "vertexes": []})
    return img.astype(np.float32), sources


def finder(path):
    from caesar_mrcnn_amd.config import SDetectorConfig
    from caesar_mrcnn_amd.sfinder import SFinder
    cfg = SDetectorConfig()
    cfg.IMG_PATH = path
    cfg.IMG_XMIN = cfg.IMG_XMAX = cfg.IMG_YMIN = cfg.IMG_YMAX = -1
    sf = SFinder(None, cfg)
    assert sf.set_img_size_params() == 0 and sf.wcs.valid and sf.beamArea > 0
    return sf


def agree(sf, img, dev, host):
    """The two catalogues source by source, with the bounds the tests derive (sfinder_params_cases.assert_params_close: exact
    keys equal, sums within the recursive-summation bounds computed from a math.fsum brute force of every source)."""
    assert len(dev) == len(host)
    keys = sf.PARAM_KEYS
    for d, h in zip(dev, host):
        g = sf._cutout_geometry(d)
        rec = cases.brute_record(img, d["pixels"], (g[0] - g[6], g[2] - g[7], g[1] + g[6] + 1, g[3] + g[7] + 1))
        # the sky positions go through SimpleWCS, whose slope in degrees per pixel is below |CDELT| / cos(dec) < 1e-3
        cases.assert_params_close({k: d[k] for k in keys}, {k: h[k] for k in keys}, rec, float(sf.beamArea), (1e-3, 1e-3))
    return True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=16)
    ap.add_argument("--tile", type=int, default=512)
    ap.add_argument("--sources", type=int, default=900)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--no-sweep", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import logging
    logging.getLogger("mrcnn").setLevel(logging.ERROR)
    import torch
    from caesar_mrcnn_amd import ops
    from caesar_mrcnn_amd.sfinder import pack_sources
    assert torch.cuda.is_available(), "needs a GPU"
    tmp = tempfile.mkdtemp(prefix="sfinder_params_bench_")
    cards = {"CDELT1": -0.0005, "CDELT2": 0.0005, "BMAJ": 0.004, "BMIN": 0.003, "BPA": 12.5, "CTYPE1": "RA---SIN", "CTYPE2": "DEC--SIN",
             "CRVAL1": 255.0, "CRVAL2": -40.0, "BUNIT": "JY/BEAM"}

    def case(size, n_sources, tag):
        from caesar_mrcnn_amd import fits
        labels, _ = plant(size, n_sources, args.seed)
        img, sources = catalogue(labels, args.seed)
        path = os.path.join(tmp, tag + ".fits")
        fits.write_fits(path, img, dict(cards, CRPIX1=size / 2.0, CRPIX2=size / 2.0))
        return finder(path), sources, img

    def run(sf, sources, device):
        sf.params_device, sf.params_device_min_sources = device, 0
        times, out, stages = [], None, None
        for rep in range(args.reps + 1):                     # the first run warms up (library load, allocator, page cache)
            sf.sources = {"sources": copy.deepcopy(sources)}
            sf._plane = None
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            sf.compute_sources_params()
            torch.cuda.synchronize()
            if rep:
                times.append(1e3 * (time.perf_counter() - t0))
            out, stages = sf.sources["sources"], dict(sf.params_timing)
        assert stages["failed_sources"] == 0 and (stages["device_sources"] > 0) == device
        return times, out, stages

    def measure(sf, sources, img):
        dev_ms, dev_out, stages = run(sf, sources, True)
        host_ms, host_out, _ = run(sf, sources, False)
        agree(sf, img, dev_out, host_out)
        return {"sources": len(sources), "host_ms": [round(v, 2) for v in host_ms], "device_ms": [round(v, 2) for v in dev_ms],
                "host_median_ms": round(float(np.median(host_ms)), 2), "device_median_ms": round(float(np.median(dev_ms)), 2),
                "host_over_device": round(float(np.median(host_ms) / np.median(dev_ms)), 2), "agree": True,
                "device_stages_last_run": stages}

    size = (args.grid + 1) * args.tile // 2
    sf, sources, img = case(size, args.sources, "big")
    npix = np.array([len(s["pixels"]) for s in sources])
    res = {"mosaic": [size, size], "sources": len(sources), "reps": args.reps,
           "source_pixels": {"min": int(npix.min()), "median": int(np.median(npix)), "max": int(npix.max())}}
    res["full"] = measure(sf, sources, img)

    # the launch alone, inputs resident
    dev = sf._device()
    geo = []
    for s in sources:
        g = sf._cutout_geometry(s)
        geo.append((g[0] - g[6], g[2] - g[7], g[1] + g[6] + 1, g[3] + g[7] + 1))
    pool, desc = pack_sources([s["pixels"] for s in sources])
    pool_t, desc_t = ops.tile_upload(pool, desc, dev)
    img_t = torch.from_numpy(np.ascontiguousarray(sf._image_plane(), dtype=np.float32)).to(dev)
    cut_t = torch.from_numpy(np.asarray(geo, np.int32)).to(dev)
    us = []
    for _ in range(20):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        keep = ops.source_params(img_t, pool_t, desc_t, cut_t, 3.0, 5, desc_host=desc)
        b.record()
        b.synchronize()
        us.append(1e3 * a.elapsed_time(b))
        del keep
    res["launch_with_its_uploads_us"] = round(float(np.median(us)), 1)

    if not args.no_sweep:
        res["sweep_big_mosaic"] = [measure(sf, sources[:k], img) for k in (1, 4, 116) if k <= len(sources)]
        sf_s, sources_s, img_s = case(1024, 116, "small")
        res["sweep_small_mosaic"] = {"mosaic": [1024, 1024],
                                     "cases": [measure(sf_s, sources_s[:k], img_s) for k in (1, 4, len(sources_s)) if k <= len(sources_s)]}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
