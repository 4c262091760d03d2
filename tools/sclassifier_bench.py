"""The source classifier's device forms against their host statements, on a seeded catalogue and a mosaic with a NaN border.
Prints one JSON object and writes it with --out (default profiles/sclassifier_bench.json).

    python tools/sclassifier_bench.py [--sizes 100,1000,10000,100000] [--host-rows 2000] [--mosaic 2048] [--sources 256] [--batches 1,4,8]
                                      [--run-sources 48] [--run-batch 8] [--max-instances 10] [--reps 3] [--no-run] [--out FILE]

  member_scan   the member lists of a whole catalogue of S sources, cut-out 132: the host statement (one vectorised NumPy
                comparison per source, SClassifier.members_host) against ops.catalog_members (upload, two launches and a scan,
                download).  The host statement is quadratic: above --host-rows sources it is timed on the first --host-rows rows
                and scaled to S (stated per entry); the two are compared on the rows that were run.
  front_end     per planned cut-out, the pixels up to the network's input image: sequential fits.crop_img on the host (cut,
                in-place NaN fill, zscale, RGB) against upload + ops.catalog_window_flags + ops.catalog_nan_fill +
                ops.fits_tiles_to_rgb in groups of N, device synchronised at the end; the upload of the mosaic is inside.
  fill_forms    ops.catalog_nan_fill on the fill list of that plan: one workgroup walking the table against one launch per window.
  run           SClassifier.classify_all on --run-sources sources with a seeded random-weight model (detections capped at
                --max-instances, as tools/sfinder_tiles_bench.py does): the loop against cutout_batch = --run-batch.
Every figure is the median of --reps runs after one warm-up run, perf_counter around a synchronised device."""
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
SIZE = 132


def catalogue(S, seed, extent=None):
    """float64 [S, 6]: centres uniform over extent^2 pixels (default: about five neighbours per 132-pixel window), boxes of 3 to 20
    pixels half-width."""
    rng = np.random.RandomState(seed)
    extent = extent or max(400.0, 60.0 * np.sqrt(S))
    c = rng.uniform(0, extent, (S, 2))
    h = rng.uniform(3, 20, (S, 2))
    return np.stack([c[:, 0], c[:, 1], c[:, 0] - h[:, 0], c[:, 0] + h[:, 0], c[:, 1] - h[:, 1], c[:, 1] + h[:, 1]], axis=1)


def mosaic(size, seed, border=48):
    rng = np.random.RandomState(seed)
    img = rng.normal(0.0, 1.0, (size, size)).astype(np.float32)
    r = 16
    yy, xx = np.mgrid[-r:r + 1, -r:r + 1]
    for _ in range((size // 128) ** 2):
        cy, cx = rng.randint(r, size - r, 2)
        img[cy - r:cy + r + 1, cx - r:cx + r + 1] += (rng.uniform(20.0, 200.0) * np.exp(-0.5 * ((yy / 4.0) ** 2 + (xx / 4.0) ** 2))).astype(np.float32)
    img[:border] = img[-border:] = np.nan
    img[:, :border] = img[:, -border:] = np.nan
    for k in range(4):
        y = rng.randint(border, size - border)
        img[y:y + 3, rng.randint(0, size // 2):] = np.nan
    return img


def make_classifier(table, img, model=None, config=None):
    from caesar_mrcnn_amd import classifier

    class Cfg(object):
        NUM_CLASSES, CLASS_NAMES = 5, ["bkg", "sidelobe", "source", "galaxy_C2", "galaxy_C3"]
    clf = classifier.SClassifier(model, config or Cfg())
    for k, row in enumerate(table):
        s = classifier.SData()
        s.name = "S%d" % (k + 1)
        s.x0, s.y0, s.xmin, s.xmax, s.ymin, s.ymax = [float(v) for v in row]
        clf.sources.append(s)
    clf.img_data, clf.scutout_size = img, SIZE
    return clf


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="100,1000,10000,100000")
    ap.add_argument("--host-rows", type=int, default=2000)
    ap.add_argument("--mosaic", type=int, default=2048)
    ap.add_argument("--sources", type=int, default=256)
    ap.add_argument("--batches", default="1,4,8")
    ap.add_argument("--run-sources", type=int, default=48)
    ap.add_argument("--run-batch", type=int, default=8)
    ap.add_argument("--max-instances", type=int, default=10)
    ap.add_argument("--backbone", default="resnet101")
    ap.add_argument("--imgsize", type=int, default=256)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--no-run", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sclassifier_bench.json"))
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a GPU: a CPU run gives no time"
    logging.getLogger("mrcnn").setLevel(logging.CRITICAL)
    import warnings
    warnings.simplefilter("ignore")
    from caesar_mrcnn_amd import fits, ops
    dev = torch.device("cuda:0")
    t_start = time.perf_counter()

    def say(what):
        sys.stderr.write("[sclassifier_bench %7.1f s] %s\n" % (time.perf_counter() - t_start, what))
        sys.stderr.flush()

    def timed(f, reps=args.reps, warm=1):
        out = None
        for _ in range(warm):
            out = f()
        ts = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = f()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        return float(np.median(ts)), [round(t, 6) for t in ts], out

    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "cutout": SIZE, "member_scan": [], "front_end": {}, "fill_forms": {}}
    # ---- member scan ----------------------------------------------------------------------------------------------------
    for S in [int(v) for v in args.sizes.split(",")]:
        table = catalogue(S, args.seed)
        clf = make_classifier(table, None)
        clf._table()
        rows = min(S, args.host_rows)

        def host():
            return [clf.members_host(i, clf.window(i)) for i in range(rows)]
        t_host, _, lists = timed(host, warm=0 if S > 10000 else 1)
        t_dev, dev_runs, got = timed(lambda: ops.catalog_members(table, SIZE, SIZE, dev))
        for i in range(rows):
            assert tuple(got[0][i]) == clf.window(i)
            assert np.array_equal(got[2][got[1][i]:got[1][i + 1]], lists[i][0]) and np.array_equal(got[3][got[1][i]:got[1][i + 1]].astype(bool), lists[i][1])
        host_full = t_host * S / rows
        res["member_scan"].append({"sources": S, "member_entries": int(got[1][-1]), "host_rows_timed": rows,
                                   "host_s": round(host_full, 6), "host_s_is_scaled_from_rows": rows < S,
                                   "device_s": round(t_dev, 6), "device_runs_s": dev_runs, "host_over_device": round(host_full / t_dev, 2)})
        say("member scan S=%d: host %.4f s%s, device %.4f s" % (S, host_full, " (scaled)" if rows < S else "", t_dev))
    ahead = [e["sources"] for e in res["member_scan"] if e["host_over_device"] > 1.0]
    res["member_scan_device_ahead_from_sources"] = min(ahead) if ahead else None
    # ---- front end ------------------------------------------------------------------------------------------------------
    img0 = mosaic(args.mosaic, args.seed)
    table = catalogue(args.sources, args.seed + 1, extent=float(args.mosaic))
    clf = make_classifier(table, img0.copy())
    win_all = np.array([clf.window(i) for i in range(len(clf.sources))], dtype=np.int64)

    def plan_for(img):
        clf.img_data = img
        failed = frozenset(i for i in range(len(clf.sources)) if clf.window_fails(clf.window(i)))
        return [c for c in clf.plan(failed) if not c.failed]
    cuts = plan_for(img0)
    ny, nx = img0.shape

    def sequential():
        data = img0.copy()
        return [fits.crop_img(data, clf.sources[c.index].x0, clf.sources[c.index].y0, SIZE, SIZE, True, True, True) for c in cuts], data

    def batched(N, form=0):
        plane = torch.from_numpy(img0).to(dev)
        flags = ops.catalog_window_flags(plane, win_all)
        fill = [c.window for c in cuts if flags[c.index, 1] > 0]
        ops.catalog_nan_fill(plane, fill, form)
        out = []
        for g0 in range(0, len(cuts), N):
            rects = [(c.window[0], c.window[2], min(c.window[1], nx) - c.window[0], min(c.window[3], ny) - c.window[2]) for c in cuts[g0:g0 + N]]
            out.extend(ops.fits_tiles_to_rgb(plane, rects))
        return out, plane
    t_seq, seq_runs, (want, want_plane) = timed(sequential)
    res["front_end"] = {"mosaic": [args.mosaic, args.mosaic], "sources": args.sources, "cutouts": len(cuts),
                        "sequential_s": round(t_seq, 6), "sequential_ms_per_cutout": round(1e3 * t_seq / len(cuts), 4), "batched": {}}
    for N in [int(v) for v in args.batches.split(",")]:
        t_b, b_runs, (got, plane) = timed(lambda: batched(N))
        assert all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(got, want)), "batched cut-outs differ from crop_img"
        assert np.array_equal(plane.cpu().numpy().view(np.uint32), want_plane.view(np.uint32)), "the filled planes differ"
        res["front_end"]["batched"]["N=%d" % N] = {"s": round(t_b, 6), "ms_per_cutout": round(1e3 * t_b / len(cuts), 4), "runs_s": b_runs,
                                                   "sequential_over_this": round(t_seq / t_b, 2)}
        say("front end N=%d: %.4f s against %.4f s sequential (%d cut-outs)" % (N, t_b, t_seq, len(cuts)))
    # ---- the two forms of the fill ----------------------------------------------------------------------------------------
    pristine = torch.from_numpy(img0).to(dev)
    flags = ops.catalog_window_flags(pristine, win_all)
    fill = [c.window for c in cuts if flags[c.index, 1] > 0]
    planes = {}
    for form, name in ((ops.CATALOG_FILL_WALK, "one_workgroup_walks"), (ops.CATALOG_FILL_LAUNCHES, "launch_per_window")):
        def run_fill():
            plane = pristine.clone()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ops.catalog_nan_fill(plane, fill, form)
            torch.cuda.synchronize()
            return time.perf_counter() - t0, plane
        run_fill()
        ts = [run_fill() for _ in range(args.reps)]
        planes[name] = ts[-1][1].cpu().numpy()
        res["fill_forms"][name] = {"s": round(float(np.median([t for t, _ in ts])), 6), "runs_s": [round(t, 6) for t, _ in ts]}
    res["fill_forms"]["windows"] = len(fill)
    res["fill_forms"]["same_plane"] = bool(np.array_equal(planes["one_workgroup_walks"].view(np.uint32), planes["launch_per_window"].view(np.uint32)))
    assert res["fill_forms"]["same_plane"]
    say("fill forms over %d windows: %s" % (len(fill), {k: v["s"] for k, v in res["fill_forms"].items() if isinstance(v, dict)}))
    # ---- whole run ----------------------------------------------------------------------------------------------------------
    if not args.no_run:
        from caesar_mrcnn_amd.config import run_py_config
        from caesar_mrcnn_amd.model import MaskRCNN
        tmp = tempfile.mkdtemp(prefix="sclassifier_bench_")
        size = 1024
        img_run = mosaic(size, args.seed + 2)
        table_run = catalogue(args.run_sources, args.seed + 3, extent=float(size))
        walls = {}
        for batch in (0, args.run_batch):
            cfg = run_py_config(num_classes=5, imgsize=args.imgsize, backbone=args.backbone, mode="inference")
            cfg.IMAGES_PER_GPU = max(1, batch)
            cfg.DETECTION_MAX_INSTANCES = args.max_instances
            cfg.CLASS_NAMES = ["bkg", "sidelobe", "source", "galaxy_C2", "galaxy_C3"]
            model = MaskRCNN("inference", cfg, os.path.join(tmp, "logs"), device=dev, seed=args.seed)
            say("model for batches of %d built" % max(1, batch))

            def whole():
                c = make_classifier(table_run, img_run.copy(), model, cfg)
                c.cutout_batch, c.score_thr = batch, 0.0
                assert c.classify_all() == 0
                return c
            t, runs, c = timed(whole)
            walls[batch] = t
            key = "loop" if batch == 0 else "cutout_batch_%d" % batch
            res.setdefault("run", {"mosaic": [size, size], "sources": args.run_sources, "backbone": args.backbone, "imgsize": args.imgsize,
                                   "weights": "random, seed %d" % args.seed, "detection_max_instances": args.max_instances})[key] = {
                "s": round(t, 4), "runs_s": [round(v, 4) for v in runs], "visited": int(sum(s.visited for s in c.sources)),
                "class_infos": int(sum(len(s.class_info) for s in c.sources))}
            say("whole run, cutout_batch %d: %.3f s" % (batch, t))
            del model
        res["run"]["loop_over_batched"] = round(walls[0] / walls[args.run_batch], 2)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
