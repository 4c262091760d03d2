"""The Pascal-VOC box metrics over a test set, metrics.voc_metrics_host against metrics.voc_metrics_device (csrc/apmatch.hip: one
ops.voc_match launch, uploads, sorts and downloads included), and utils.compute_ap of one image with the mask overlaps formed on
the host against metrics.mask_ap on the device tensor of the masks (csrc/maskeval.hip); prints one JSON object (and writes it with
--out, default profiles/map_bench.json).

    python tools/map_bench.py [--images 5,20,50,100,200,2000,20000] [--reps 3] [--mask-case 100x300,512] [--out FILE]

Test sets are seeded: images of 256 x 256 with about 20 objects of 3 classes and about 30 detections each -- two thirds of the
objects detected with their corners moved by -3 .. 3 pixels, the rest of the detections elsewhere; scores have two decimals, so equal
scores are frequent.  At every size the two forms are compared first (metrics.same_metrics: every number, NaN equal to NaN) and
nothing is timed unless they agree.  Each form is warmed up once on the size's own data, then timed --reps times with a host clock
around a synchronise; medians are reported.  `match_*_ms` is the matching step alone on the flat tables (voc_match_host against
upload + ops.voc_match + download).  `break_even_detections` is the smallest number of detections from which on the device form is
ahead at every larger size: the source of metrics.DEVICE_MIN_DETECTIONS.  The mask case: D detections x G objects, discs on a
size x size frame, all four results of compute_ap compared with == first."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LABELS = ["compact", "extended", "galaxy"]


def test_set(n_images, seed, size=256):
    rng = np.random.default_rng(seed)
    gt_data, pred_data = [], []
    for _ in range(n_images):
        gt, pred = [], []
        for _ in range(int(rng.poisson(20))):
            y, x = (int(v) for v in rng.integers(0, size - 8, 2))
            h, w = (int(v) for v in rng.integers(4, 40, 2))
            gt.append([y, x, min(y + h, size), min(x + w, size), LABELS[int(rng.integers(0, 3))]])
        for row in gt:
            if rng.random() < 2.0 / 3.0:
                box = [max(0, min(size, c + int(rng.integers(-3, 4)))) for c in row[:4]]
                label = row[4] if rng.random() < 0.9 else LABELS[int(rng.integers(0, 3))]
                pred.append(box + [label, round(float(rng.uniform(0.5, 1.0)), 2)])
        for _ in range(int(rng.poisson(17))):
            y, x = (int(v) for v in rng.integers(0, size - 8, 2))
            h, w = (int(v) for v in rng.integers(4, 40, 2))
            pred.append([y, x, min(y + h, size), min(x + w, size), LABELS[int(rng.integers(0, 3))], round(float(rng.uniform(0.5, 1.0)), 2)])
        order = rng.permutation(len(pred))
        gt_data.append(gt)
        pred_data.append([pred[k] for k in order])
    return gt_data, pred_data


def discs(n, size, rng, centres=None):
    yy, xx = np.mgrid[0:size, 0:size]
    centres = centres or [(int(rng.integers(0, size)), int(rng.integers(0, size)), int(rng.integers(2, 13))) for _ in range(n)]
    return np.stack([(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r for cy, cx, r in centres], axis=-1), centres


def med(v):
    return round(float(np.median(v)), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", default="5,20,50,100,200,2000,20000")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--mask-case", default="100x300,512")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_bench.json"))
    args = ap.parse_args()
    import torch
    from caesar_mrcnn_amd import metrics, ops, utils
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda", torch.cuda.current_device())
    clock = time.perf_counter
    thr = (0.5, 0.6)

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

    def device_match(flat):
        t = lambda a: torch.from_numpy(a).to(dev)
        got = ops.voc_match(t(flat.det_box), t(flat.det_cls), t(flat.det_score), flat.det_off, t(flat.gt_box), t(flat.gt_cls), flat.gt_off,
                            t(np.asarray(thr, np.float64)))
        return [g.cpu().numpy() for g in got]

    def case(n_images):
        gt, pred = test_set(n_images, args.seed)
        host, device = metrics.voc_metrics_host(gt, pred, thr), metrics.voc_metrics_device(gt, pred, thr, device=dev)
        assert metrics.same_metrics(host, device), "the two forms differ at %d images" % n_images
        flat = metrics.Flat(gt, pred)
        for a, b in zip(device_match(flat), metrics.voc_match_host(flat, thr)):
            assert np.array_equal(a, b)
        host_ms = timed(lambda: metrics.voc_metrics_host(gt, pred, thr), args.reps)
        dev_ms = timed(lambda: metrics.voc_metrics_device(gt, pred, thr, device=dev), args.reps)
        mh_ms = timed(lambda: metrics.voc_match_host(flat, thr), args.reps)
        md_ms = timed(lambda: device_match(flat), args.reps)
        out = {"images": n_images, "detections": flat.D, "ground_truths": flat.G, "equal": True, "mAP_0.5": round(float(host["results"][0]["mAP"]), 6),
               "host_ms": med(host_ms), "device_ms": med(dev_ms), "host_over_device": round(med(host_ms) / med(dev_ms), 2),
               "match_host_ms": med(mh_ms), "match_device_ms": med(md_ms), "runs": args.reps}
        sys.stderr.write(json.dumps(out) + "\n")
        sys.stderr.flush()
        return out

    def mask_case(D, G, size):
        rng = np.random.default_rng(args.seed)
        gt_mask, centres = discs(G, size, rng)
        det_c = [(cy, cx, max(1, r + int(rng.integers(-1, 2)))) for cy, cx, r in centres[:D]]
        pred_mask, _ = discs(D, size, rng, det_c + [(int(rng.integers(0, size)), int(rng.integers(0, size)), 5) for _ in range(D - len(det_c))])
        gt_box, box = utils.extract_bboxes(gt_mask), utils.extract_bboxes(pred_mask)
        gt_cls, cls = rng.integers(1, 4, G).astype(np.int32), rng.integers(1, 4, D).astype(np.int32)
        score = rng.uniform(0.5, 1.0, D).astype(np.float32)
        r = {"rois": box, "class_ids": cls, "scores": score, "masks": pred_mask}
        masks_dev = torch.from_numpy(pred_mask.view(np.uint8)).to(dev)
        host = lambda: utils.compute_ap(gt_box, gt_cls, gt_mask, box, cls, score, pred_mask, 0.6)
        device = lambda: metrics.mask_ap(gt_box, gt_cls, gt_mask, r, masks_dev, 0.6)
        for a, b in zip(host(), device()):
            assert np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True), "mask AP differs"
        host_ms, dev_ms = timed(host, args.reps), timed(device, args.reps)
        return {"detections": D, "true_objects": G, "frame": [size, size], "equal": True, "AP": round(float(host()[0]), 6),
                "host_ms": med(host_ms), "device_ms": med(dev_ms), "host_over_device": round(med(host_ms) / med(dev_ms), 2), "runs": args.reps}

    result = {"device": torch.cuda.get_device_name(dev), "thresholds": list(thr),
              "generator": "256 x 256 images, about 20 objects and 30 detections of 3 classes each, seed %d" % args.seed,
              "timed": "voc_metrics_host / voc_metrics_device from the row lists to the result, host clock around a synchronise, median",
              "cases": [case(int(n)) for n in args.images.split(",")]}
    sizes = sorted(c["detections"] for c in result["cases"])
    ahead = [d for d in sizes if all(c["device_ms"] < c["host_ms"] for c in result["cases"] if c["detections"] >= d)]
    result["break_even_detections"] = min(ahead) if ahead else None
    result["device_min_detections_in_use"] = metrics.DEVICE_MIN_DETECTIONS
    if args.mask_case:
        dg, size = args.mask_case.split(",")
        D, G = (int(v) for v in dg.split("x"))
        result["mask_ap"] = mask_case(D, G, int(size))
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
