"""The tester's two pixel steps, Analyzer.compute_det_mask_pars + compute_performances, host statement (mask_iou on full frames per
pair, twice) against the device path (csrc/maskeval.hip: one mask_cross_stats and one mask_plane_sums launch on bit planes, uploads
and downloads included), on seeded synthetic discs; prints one JSON object (and writes it with --out, default
profiles/tester_bench.json).

    python tools/tester_bench.py [--cases 1x1,3x3,10x10,50x50,300x100] [--sizes 256,512] [--reps 10] [--out FILE]
    python tools/tester_bench.py --profile-case 300x100,512 [--reps 5]      # the device path alone, for a kernel trace

Per case (G true objects, D detections, size x size frame), in one process on one machine: G discs of radius 2 - 12 px, D
detections of which the first min(G, D) are the true discs with the radius changed by -1 .. 1 and the rest are elsewhere.  Both
paths run on fresh Analyzers; their results are compared first (every list and array with ==, Stot and snr within the bound of a
float64 sum), and nothing is timed unless they agree.  Each path is warmed up on the case's own shape, then timed --reps times
(the host statement once where G * D >= 2500: one run takes seconds to a minute there); medians are reported.
`break_even_pairs` is the smallest G * D from which on the device path is ahead at every frame size: the source of
Analyzer.EVAL_DEVICE_MIN_PAIRS."""
import argparse
import contextlib
import io
import json
import os
import sys
import tempfile
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CLASS_NAMES = ["bkg", "spurious", "compact", "extended"]
META = {"telescope": "bench", "bkg": 1e-5, "rms": 3e-4, "bmaj": 12.0, "bmin": 9.0, "dx": -4.0, "dy": 4.0}
EPS = 2.0 ** -52


def scene(G, D, size, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:size, 0:size]

    def disc(cy, cx, r):
        return (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r
    gt_par = [(int(rng.integers(0, size)), int(rng.integers(0, size)), int(rng.integers(2, 13))) for _ in range(G)]
    det_par = [(cy, cx, max(1, r + int(rng.integers(-1, 2)))) for cy, cx, r in gt_par[:D]]
    det_par += [(int(rng.integers(0, size)), int(rng.integers(0, size)), int(rng.integers(2, 13))) for _ in range(D - len(det_par))]
    img = (rng.normal(size=(size, size)) * 3e-4).astype(np.float32)
    for cy, cx, r in gt_par:
        img[disc(cy, cx, r)] += np.float32(rng.uniform(1e-3, 1e-1))
    return {"gt": [disc(*p).astype(int) for p in gt_par], "gt_ids": rng.integers(1, len(CLASS_NAMES), size=G).tolist(),
            "det": [disc(*p) for p in det_par], "det_ids": rng.integers(1, len(CLASS_NAMES), size=D).tolist(),
            "scores": rng.uniform(0.7, 1.0, size=D).astype(np.float32).tolist(), "img": img}


def make_analyzer(sc, path, device):
    from caesar_mrcnn_amd import analyze
    from caesar_mrcnn_amd.utils import extract_bboxes
    cfg = types.SimpleNamespace(NUM_CLASSES=len(CLASS_NAMES), CLASS_NAMES=list(CLASS_NAMES))
    ds = types.SimpleNamespace(nclasses=len(CLASS_NAMES), consider_sources_near_mixed_sidelobes=True)
    an = analyze.Analyzer(None, cfg, ds, [], [])
    an.eval_device, an.eval_device_min_pairs = device, 0
    size = sc["img"].shape[0]
    an.image_path, an.image_metadata = path, dict(META, nx=size, ny=size)
    an.class_names = an.class_names_gt = list(CLASS_NAMES)
    an.masks_gt_merged, an.class_ids_gt_merged = list(sc["gt"]), list(sc["gt_ids"])
    an.sidelobes_mixed_or_near_gt_merged = [0] * len(sc["gt"])
    an.masks_final, an.class_ids_final, an.scores_final = list(sc["det"]), list(sc["det_ids"]), list(sc["scores"])
    if "boxes" not in sc:
        sc["boxes"] = ([extract_bboxes(m.astype(bool)[:, :, None])[0] for m in sc["gt"]],
                       [extract_bboxes(m[:, :, None])[0] for m in sc["det"]])
    an.bboxes_gt, an.bboxes = sc["boxes"]
    an.objs_gt = []
    return an


def run(an):
    with contextlib.redirect_stdout(io.StringIO()):
        assert an.compute_det_mask_pars() == 0
        an.compute_performances()
    return an


LISTS = ("detobj_scores", "detobj_ious", "detobj_classids", "detobj_class_names", "is_gt_obj_detected", "is_det_obj_matching_to_gt_obj",
         "is_det_obj_matching_to_gt_obj_sameclass", "matchobj_classids", "matchobj_class_names", "matchobj_ious")
ARRAYS = ("confusion_matrix", "confusion_matrix_norm", "purity", "nobjs_true", "nobjs_det", "nobjs_det_right")


def assert_same(dev, host, sc):
    for k in LISTS:
        assert getattr(dev, k) == getattr(host, k), k
    for k in ARRAYS:
        assert np.array_equal(getattr(dev, k), getattr(host, k)), k
    assert len(dev.det_obj_pars) == len(host.det_obj_pars) == len(sc["det"])
    x = np.abs(sc["img"].astype(np.float64))
    for a, b, m in zip(dev.det_obj_pars, host.det_obj_pars, sc["det"]):
        bound = a["npix"] * EPS * float(x[m].sum())
        assert abs(a["Stot"] - b["Stot"]) <= bound, (a["Stot"], b["Stot"], bound)
        assert abs(a["snr"] - b["snr"]) <= bound / (META["rms"] * np.sqrt(a["npix"])) + 4 * EPS * abs(b["snr"])
        assert {k: v for k, v in a.items() if k not in ("Stot", "snr")} == {k: v for k, v in b.items() if k not in ("Stot", "snr")}


def med(v):
    return round(float(np.median(v)), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="1x1,3x3,10x10,50x50,300x100")
    ap.add_argument("--sizes", default="256,512")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--profile-case", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tester_bench.json"))
    args = ap.parse_args()
    import logging
    logging.getLogger("mrcnn").setLevel(logging.ERROR)
    import torch
    from caesar_mrcnn_amd import fits
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda", torch.cuda.current_device())
    clock = time.perf_counter
    tmp = tempfile.mkdtemp(prefix="tester_bench_")

    def timed(sc, path, device, reps):
        times = []
        for _ in range(reps):
            an = make_analyzer(sc, path, device)
            torch.cuda.synchronize()
            t0 = clock()
            run(an)
            torch.cuda.synchronize()
            times.append(1e3 * (clock() - t0))
        return times, an

    def prepare(G, D, size):
        sc = scene(G, D, size, args.seed)
        path = os.path.join(tmp, "img_%d_%d_%d.fits" % (G, D, size))
        fits.write_fits(path, sc["img"])
        return sc, path

    if args.profile_case:
        gd, size = args.profile_case.split(",")
        G, D = (int(v) for v in gd.split("x"))
        sc, path = prepare(G, D, int(size))
        times, _ = timed(sc, path, True, args.reps)
        print(json.dumps({"true_objects": G, "detections": D, "frame": [int(size)] * 2, "device_ms": [round(t, 3) for t in times]}))
        return

    def case(G, D, size):
        sc, path = prepare(G, D, size)
        _, an_dev = timed(sc, path, True, 2)                         # warm-up on this shape: library load, allocator
        host_reps = 1 if G * D >= 2500 else args.reps
        host_ms, an_host = timed(sc, path, False, 1)                 # the host's warm-up is its first run (kept where it is the only one)
        assert_same(an_dev, an_host, sc)
        assert an_dev.eval_timing.get("mask_uploads") == 2, an_dev.eval_timing
        if host_reps > 1:
            host_ms, _ = timed(sc, path, False, host_reps)
        dev_ms, an_dev = timed(sc, path, True, args.reps)
        out = {"true_objects": G, "detections": D, "pairs": G * D, "frame": [size, size], "equal": True, "host_ms": med(host_ms),
               "host_runs": host_reps, "device_ms": med(dev_ms), "device_runs": args.reps,
               "device_min_ms": round(min(dev_ms), 3), "device_max_ms": round(max(dev_ms), 3),
               "host_over_device": round(med(host_ms) / med(dev_ms), 2),
               "device_steps_ms": {k: v for k, v in an_dev.eval_timing.items() if k.endswith("_ms")}}
        sys.stderr.write(json.dumps(out) + "\n")
        sys.stderr.flush()
        return out

    sizes = [int(v) for v in args.sizes.split(",")]
    gds = [tuple(int(v) for v in c.split("x")) for c in args.cases.split(",")]
    result = {"device": torch.cuda.get_device_name(dev), "generator": "discs of radius 2-12 px, seed %d" % args.seed,
              "timed": "compute_det_mask_pars + compute_performances, fresh Analyzer per run, uploads and downloads included",
              "cases": [case(G, D, size) for size in sizes for G, D in gds]}
    pairs = sorted(set(c["pairs"] for c in result["cases"]))
    ahead = [p for p in pairs if all(c["device_ms"] < c["host_ms"] for c in result["cases"] if c["pairs"] >= p)]
    result["break_even_pairs"] = min(ahead) if ahead else None
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
