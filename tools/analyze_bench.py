"""Analyzer.extract_det_masks, host statement against the bit-plane path (csrc/maskgraph.hip), on seeded synthetic detections;
prints one JSON object (and writes it with --out, default profiles/analyze_postprocess_bench.json).

    python tools/analyze_bench.py [--n 5,20,50,100] [--sizes 256,512] [--reps 10] [--small-n 1,2,3] [--out FILE]
    python tools/analyze_bench.py --profile-case 100,256 [--reps 5]      # the device path alone, for a kernel trace

The detections: N discs of radius 2 - 12 px with random centres, classes (three of them, one named 'spurious') and scores above
score_thr, on a size x size frame.  Per case, on the same machine in the same run:
  host     extract_det_masks_host, median of --reps runs (N = 100 at 512 x 512: one run);
  device   extract_det_masks_device with the masks already on the device, as MaskRCNN.detect leaves them, device synchronised
           before and after; and once more starting from the host array (one upload);
  stages   the device path's own split (upload + pack, merge pairs, union, selection pairs, host lists, download + unpack), from
           runs that synchronise after every stage;
  json     make_json_results on the selected masks, the stage that follows in predict().
The two paths' results are compared first; nothing is timed unless they are equal.  --small-n adds the host / device times at a
few detections on the first size: the break-even behind Analyzer.POSTPROCESS_DEVICE_MIN_MASKS."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CLASS_NAMES = ["bkg", "spurious", "compact", "extended"]


def discs(n, size, seed):
    """The detect() result of n planted discs: rois [n, 4], class_ids [n], scores [n] in [0.7, 1), masks [size, size, n] bool."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:size, 0:size]
    masks = np.zeros((size, size, n), bool)
    rois = np.zeros((n, 4), np.int32)
    for i in range(n):
        r = int(rng.integers(2, 13))
        cy, cx = int(rng.integers(0, size)), int(rng.integers(0, size))
        m = (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r
        masks[:, :, i] = m
        ys, xs = np.nonzero(m)
        rois[i] = (ys.min(), xs.min(), ys.max() + 1, xs.max() + 1)
    return {"rois": rois, "masks": masks, "class_ids": rng.integers(1, len(CLASS_NAMES), size=n).astype(np.int32),
            "scores": rng.uniform(0.7, 1.0, size=n).astype(np.float32)}


def analyzer(res):
    from caesar_mrcnn_amd import analyze
    from caesar_mrcnn_amd.config import run_py_config
    cfg = run_py_config(num_classes=len(CLASS_NAMES), imgsize=64, mode="inference")
    cfg.CLASS_NAMES = list(CLASS_NAMES)
    an = analyze.Analyzer(None, cfg)
    an.image = np.zeros(res["masks"].shape[:2] + (3,), np.uint8)
    an.image_id = "bench"
    an.masks, an.boxes, an.class_ids, an.scores = res["masks"], res["rois"], res["class_ids"], res["scores"]
    an.nobjects = an.masks.shape[-1]
    return an


def finals(an):
    return ([(np.asarray(m).dtype.str, np.asarray(m).tobytes()) for m in an.masks_final], [int(c) for c in an.class_ids_final],
            list(an.class_names_final), [float(s) for s in an.scores_final], [np.asarray(b).tolist() for b in an.bboxes], list(an.captions))


def med(v):
    return round(float(np.median(v)), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="5,20,50,100")
    ap.add_argument("--sizes", default="256,512")
    ap.add_argument("--small-n", default="1,2,3")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--profile-case", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "analyze_postprocess_bench.json"))
    args = ap.parse_args()
    import logging
    logging.getLogger("mrcnn").setLevel(logging.ERROR)
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda", torch.cuda.current_device())
    clock = time.perf_counter

    def device_run(an, resident, reps, sync_stages=False):
        an.postprocess_sync_timing = sync_stages
        times, stages = [], []
        for _ in range(reps):
            an.masks_device, an.masks_device_host = resident, an.masks
            torch.cuda.synchronize()
            t0 = clock()
            an.extract_det_masks_device()
            torch.cuda.synchronize()
            times.append(1e3 * (clock() - t0))
            stages.append(dict(an.postprocess_timing))
        return times, stages

    if args.profile_case:
        n, size = (int(v) for v in args.profile_case.split(","))
        res = discs(n, size, args.seed)
        an = analyzer(res)
        resident = torch.from_numpy(res["masks"].view(np.uint8)).to(dev)
        times, _ = device_run(an, resident, args.reps)
        print(json.dumps({"detections": n, "frame": [size, size], "device_ms": [round(t, 3) for t in times]}))
        return

    def case(n, size, reps):
        res = discs(n, size, args.seed)
        an = analyzer(res)
        resident = torch.from_numpy(res["masks"].view(np.uint8)).to(dev)
        device_run(an, resident, 2)                                  # warm-up: library load, allocator
        got = finals(an)
        host_reps = 1 if (n >= 100 and size >= 512) else reps
        host = []
        for _ in range(host_reps):
            t0 = clock()
            an.extract_det_masks_host()
            host.append(1e3 * (clock() - t0))
        assert finals(an) == got, "host and device results differ (N = %d, %d x %d)" % (n, size, size)
        t_json = []
        for _ in range(min(reps, 3)):
            t0 = clock()
            an.make_json_results()
            t_json.append(1e3 * (clock() - t0))
        dev_res, _ = device_run(an, resident, reps)
        dev_up, _ = device_run(an, None, reps)
        _, stages = device_run(an, resident, reps, sync_stages=True)
        assert finals(an) == got
        out = {"detections": n, "frame": [size, size], "selected": len(an.masks_final), "identical": True,
               "host_ms": med(host), "host_runs": host_reps, "device_ms": med(dev_res), "device_with_upload_ms": med(dev_up),
               "device_runs": reps, "host_over_device": round(med(host) / med(dev_res), 1),
               "device_stages_ms": {k: med([s[k] for s in stages]) for k in stages[0] if k.endswith("_ms")},
               "make_json_results_ms": med(t_json)}
        sys.stderr.write(json.dumps(out) + "\n")
        sys.stderr.flush()
        return out

    sizes = [int(v) for v in args.sizes.split(",")]
    result = {"device": torch.cuda.get_device_name(dev), "generator": "discs of radius 2-12 px, seed %d" % args.seed,
              "cases": [case(n, size, args.reps) for size in sizes for n in (int(v) for v in args.n.split(","))],
              "small_n": [case(n, sizes[0], args.reps) for n in (int(v) for v in args.small_n.split(",") if v)]}
    loses = [c["detections"] for c in result["small_n"] + result["cases"] if c["frame"][0] == sizes[0] and c["device_ms"] >= c["host_ms"]]
    result["break_even_detections"] = 0 if not loses else max(loses) + 1
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
