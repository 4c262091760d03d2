"""The sweep mAP over a test set (the reference's second vendored box-metric tool, tarlen5-calculate-mean-ap), metrics.sweep_metrics_host
against metrics.sweep_metrics_device (csrc/apsweep.hip: one ops.ap_sweep launch, uploads, the torch sums and downloads included);
prints one JSON object (and writes it with --out, default profiles/sweep_bench.json).

    python tools/sweep_bench.py [--images 1,2,5,20,50,100,200,2000] [--reps 3] [--tool PATH/calculate.py [--tool-only]] [--out FILE]

Test sets are the seeded ones of tools/map_bench.py: images of 256 x 256 with about 20 objects of 3 classes and about 30 detections
each, scores of two decimals -- with the corners of a box put in order where the generator's jitter crossed them (this tool raises
on such a box).  At every size the two forms are compared first (metrics.same_sweep: every number) and nothing is
timed unless they agree and no problem was handed back to the host.  Each form is warmed up once on the size's own data, then timed
--reps times with a host clock around a synchronise; medians are reported.  `tables_*_ms` is the matching step alone on the flat
problem table (sweep_tables_host against upload + ops.ap_sweep + download).  `break_even_detections` is the smallest number of
detections from which on the device form is ahead at every larger size: the source of metrics.SWEEP_DEVICE_MIN_DETECTIONS.  With
--tool (the tool's calculate.py, where a copy of the reference is at hand) the tool's own get_avg_precision_at_iou is timed at
--tool-images images (default 5: it is slow), one IoU threshold, with inert stand-ins for its plotting imports: it computes one of the sixteen curves a result
holds."""
import argparse
import copy
import importlib.util
import json
import os
import sys
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import map_bench                                            # noqa: E402


def med(v):
    return round(float(np.median(v)), 3)


class _Inert(object):
    def __init__(self, *a, **k):
        pass

    def __getattr__(self, k):
        return _Inert()

    def __call__(self, *a, **k):
        return _Inert()


def load_tool(path):
    """calculate.py as a module, its plotting imports replaced by stand-ins that do nothing."""
    for name in ("matplotlib", "matplotlib.pyplot", "pandas", "seaborn"):
        mod = types.ModuleType(name)
        mod.__getattr__ = lambda k: _Inert
        sys.modules[name] = mod
        parent, _, child = name.rpartition(".")
        if parent:
            setattr(sys.modules[parent], child, mod)
    spec = importlib.util.spec_from_file_location("_sweep_tool", path)
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def test_set(n_images, seed):
    """map_bench.test_set with the corners of every box put in order: moving the corners of a 4-pixel box by -3 .. 3 pixels can
    cross them, and this tool -- unlike the Pascal-VOC one -- raises on such a box (here: a ValueError)."""
    gt, pred = map_bench.test_set(n_images, seed)
    order = lambda r: [min(r[0], r[2]), min(r[1], r[3]), max(r[0], r[2]), max(r[1], r[3])] + list(r[4:])
    return [[order(r) for r in img] for img in gt], [[order(r) for r in img] for img in pred]


def tool_case(args, n_images, clock):
    tool = load_tool(args.tool)
    gt, pred = test_set(n_images, args.seed)
    gt_boxes = {str(i): {"boxes": [r[:4] for r in img], "class": [r[4] for r in img]} for i, img in enumerate(gt)}
    pred_boxes = {str(i): {"boxes": [r[:4] for r in img], "class": [r[4] for r in img], "scores": [r[5] for r in img]} for i, img in enumerate(pred)}
    times = []
    for _ in range(args.reps):
        g, p = copy.deepcopy(gt_boxes), copy.deepcopy(pred_boxes)
        t0 = clock()
        data = tool.get_avg_precision_at_iou(g, p, iou_thr=0.5)
        times.append(1e3 * (clock() - t0))
    return {"images": n_images, "detections": sum(map(len, pred)), "iou_threshold": 0.5, "avg_prec": round(float(data["avg_prec"]), 6),
            "tool_one_threshold_ms": med(times), "runs": args.reps,
            "measured": "with --tool-only, on a host without a GPU: not the machine of `cases`" if args.tool_only else "on the machine of `cases`"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", default="1,2,5,20,50,100,200,2000")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--tool", default="")
    ap.add_argument("--tool-images", type=int, default=5)
    ap.add_argument("--tool-only", action="store_true", help="time the tool alone (no GPU needed) and add it to the JSON of --out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sweep_bench.json"))
    args = ap.parse_args()
    import torch
    from caesar_mrcnn_amd import metrics, ops
    clock = time.perf_counter
    if args.tool_only:
        result = json.load(open(args.out)) if args.out and os.path.exists(args.out) else {}
        result["tool"] = tool_case(args, args.tool_images, clock)
        line = json.dumps(result)
        print(line)
        if args.out:
            with open(args.out, "w") as f:
                f.write(line + "\n")
        return
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda", torch.cuda.current_device())
    thr_all = metrics._sweep_thresholds(metrics.SWEEP_IOU_THRESHOLDS, metrics.SWEEP_CLASS_THRESHOLDS)[2]

    def timed(f, reps):
        f()                                                              # warm-up on this data
        times = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = clock()
            f()
            torch.cuda.synchronize()
            times.append(1e3 * (clock() - t0))
        return times

    def device_tables(pr):
        t = lambda a: torch.from_numpy(a).to(dev)
        tp, status = ops.ap_sweep(t(pr.det_box), pr.det_off, t(pr.gt_box), pr.gt_off, t(thr_all))
        return tp.cpu().numpy(), status.cpu().numpy()

    def case(n_images):
        gt, pred = test_set(n_images, args.seed)
        back = []
        host, device = metrics.sweep_metrics_host(gt, pred), metrics.sweep_metrics_device(gt, pred, device=dev, handed_back=back)
        assert metrics.same_sweep(host, device), "the two forms differ at %d images" % n_images
        assert back == [], "problems handed back to the host at %d images: %s" % (n_images, back[:8])
        pr = metrics.SweepProblems(gt, pred)
        tp, status = device_tables(pr)
        assert not status.any() and np.array_equal(tp, metrics.sweep_tables_host(pr, thr_all)[0])
        host_ms = timed(lambda: metrics.sweep_metrics_host(gt, pred), args.reps)
        dev_ms = timed(lambda: metrics.sweep_metrics_device(gt, pred, device=dev), args.reps)
        th_ms = timed(lambda: metrics.sweep_tables_host(pr, thr_all), args.reps)
        td_ms = timed(lambda: device_tables(pr), args.reps)
        out = {"images": n_images, "detections": sum(map(len, pred)), "ground_truths": sum(map(len, gt)), "problems": pr.N, "equal": True,
               "mAP": round(float(host["mAP"]), 6), "points_0.5": int(host["results"][0]["precisions"].size),
               "host_ms": med(host_ms), "device_ms": med(dev_ms), "host_over_device": round(med(host_ms) / med(dev_ms), 2),
               "tables_host_ms": med(th_ms), "tables_device_ms": med(td_ms), "runs": args.reps}
        sys.stderr.write(json.dumps(out) + "\n")
        sys.stderr.flush()
        return out

    sizes = [int(n) for n in args.images.split(",")]
    result = {"device": torch.cuda.get_device_name(dev), "thresholds": [float(t) for t in thr_all],
              "generator": "tools/map_bench.py test_set: 256 x 256 images, about 20 objects and 30 detections of 3 classes each, seed %d" % args.seed,
              "timed": "sweep_metrics_host / sweep_metrics_device from the row lists to the result, host clock around a synchronise, median",
              "cases": [case(n) for n in sizes]}
    by_size = sorted(c["detections"] for c in result["cases"])
    ahead = [d for d in by_size if all(c["device_ms"] < c["host_ms"] for c in result["cases"] if c["detections"] >= d)]
    result["break_even_detections"] = min(ahead) if ahead else None
    result["device_min_detections_in_use"] = metrics.SWEEP_DEVICE_MIN_DETECTIONS
    if args.tool:
        result["tool"] = tool_case(args, args.tool_images, clock)
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
