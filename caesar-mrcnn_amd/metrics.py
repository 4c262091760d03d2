"""Box and mask average precision over a test set: what the reference's ``ModelTester.compute_mAP`` (mrcnn/analyze.py:408-575)
prepares for, and what its vendored Pascal-VOC tool (Object-Detection-Metrics: pascalvoc.py, lib/Evaluator.py) computes from it.

``gt_data`` / ``pred_data`` are the lists ``Analyzer.inspect_results`` fills: per image a list of rows
``[c0, c1, c2, c3, label]`` resp. ``[c0, c1, c2, c3, label, score]`` (corner boxes; swapping the two axes of every box changes no
IoU, so the (y1, x1, y2, x2) rows here give what the tool gives on the exported files read with ``-gtformat xyrb -detformat xyrb``).

  voc_metrics_host    Evaluator.GetPascalVOCMetrics (every-point interpolation) and the mAP rule of pascalvoc.py:352-378, restated:
                      same float64 operations in the same order.
  voc_metrics_device  the same numbers; the matching -- best ground truth per detection and the "seen" flag, the part that
                      grows with detections x ground truths -- is one ops.voc_match launch (csrc/apmatch.hip) over the whole set,
                      the per-class order and the cumulative counts are torch calls, the integration is the host's.
  voc_metrics         picks one of the two from the size of the problem.
  write_metric_files  the input files of the three external tools, as compute_mAP writes them.
  mask_overlaps_device / mask_ap   the [P, G] mask IoUs of one image from bit planes (one ops.mask_cross_stats launch) and
                      utils.compute_ap on them.

A result is ``{"classes": [labels, sorted], "thresholds": [...], "results": [per threshold {"threshold", "mAP", "classes":
{label: {"precision", "recall", "AP", "total positives", "total TP", "total FP", "TP", "FP", "acc TP", "acc FP"}}}]}`` -- the
tool's keys, plus the flags and cumulative counts in the class's descending-score order.
"""
import json
import os
import sys

import numpy as np

from . import utils
from .analyze import model_device, model_has_gpu

# voc_metrics takes the device form from this many detections on: the measured break-even (tools/map_bench.py,
# profiles/map_bench.json `break_even_detections`: the smallest measured test set from which on the device form was ahead; below
# it the uploads, the launch and the downloads cost more than the host's per-image NumPy calls)
DEVICE_MIN_DETECTIONS = 614
# mask counts are exact in float32 below this many pixels: the device overlaps equal compute_overlaps_masks bit for bit
EXACT_PIXELS = 1 << 24


class Flat(object):
    """A test set as flat tables: det_box [D, 4] / gt_box [G, 4] float64, det_cls / gt_cls int32 (index into `classes`), det_score
    [D] float64, det_off / gt_off [I + 1] int64 (image i owns rows off[i] .. off[i + 1]); rows keep the lists' order."""

    def __init__(self, gt_data, pred_data):
        if len(gt_data) != len(pred_data):
            raise ValueError("gt_data and pred_data hold %d and %d images" % (len(gt_data), len(pred_data)))
        gt_rows = [r for img in gt_data for r in img]
        det_rows = [r for img in pred_data for r in img]
        self.classes = sorted(set(r[4] for r in gt_rows) | set(r[4] for r in det_rows))
        index = {c: k for k, c in enumerate(self.classes)}
        self.gt_box = np.array([r[:4] for r in gt_rows], dtype=np.float64).reshape(-1, 4)
        self.det_box = np.array([r[:4] for r in det_rows], dtype=np.float64).reshape(-1, 4)
        self.gt_cls = np.array([index[r[4]] for r in gt_rows], dtype=np.int32)
        self.det_cls = np.array([index[r[4]] for r in det_rows], dtype=np.int32)
        self.det_score = np.array([r[5] for r in det_rows], dtype=np.float64)
        self.gt_off = np.concatenate([[0], np.cumsum([len(img) for img in gt_data], dtype=np.int64)]).astype(np.int64)
        self.det_off = np.concatenate([[0], np.cumsum([len(img) for img in pred_data], dtype=np.int64)]).astype(np.int64)
        self.I, self.D, self.G = len(gt_data), len(det_rows), len(gt_rows)


def _thresholds(iou_thresholds):
    thr = np.array([float(t) for t in iou_thresholds], dtype=np.float64).reshape(-1)
    if thr.size == 0 or not bool(np.all(thr > 0)):
        raise ValueError("IoU thresholds must be > 0 (at 0 the tool reads a ground-truth index it never set)")
    return thr


def box_iou_matrix(a, b):
    """Evaluator.iou (:382-426) of every box of a [n, 4] against every box of b [m, 4], float64, operation for operation."""
    a0, a1, a2, a3 = (a[:, k][:, None] for k in range(4))
    b0, b1, b2, b3 = (b[:, k][None, :] for k in range(4))
    apart = (a0 > b2) | (b0 > a2) | (a3 < b1) | (a1 > b3)
    inter = (np.minimum(a2, b2) - np.maximum(a0, b0) + 1) * (np.minimum(a3, b3) - np.maximum(a1, b1) + 1)
    union = (a2 - a0 + 1) * (a3 - a1 + 1) + (b2 - b0 + 1) * (b3 - b1 + 1) - inter
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(apart, 0.0, inter / union)


def voc_match_host(flat, thr):
    """The host statement of ops.voc_match (Evaluator.py:99-122): (best_gt [D] int32, best_iou [D] float64, tp [T, D] uint8)."""
    thr = _thresholds(thr)
    best_gt = np.full(flat.D, -1, np.int32)
    best_iou = np.zeros(flat.D, np.float64)
    for i in range(flat.I):
        d0, d1, g0, g1 = flat.det_off[i], flat.det_off[i + 1], flat.gt_off[i], flat.gt_off[i + 1]
        if d1 == d0 or g1 == g0:
            continue
        iou = box_iou_matrix(flat.det_box[d0:d1], flat.gt_box[g0:g1])
        iou = np.where(flat.det_cls[d0:d1, None] == flat.gt_cls[None, g0:g1], iou, 0.0)
        arg = np.argmax(iou, axis=1)                                   # the first of equal maxima, as `iou > iouMax` keeps it
        top = iou[np.arange(d1 - d0), arg]
        found = top > sys.float_info.min                               # iouMax starts there: an IoU of 0 is no ground truth
        best_gt[d0:d1] = np.where(found, g0 + arg, -1)
        best_iou[d0:d1] = np.where(found, top, 0.0)
    # the tool's walk, per class in stable descending-score order; a ground truth belongs to one class, so one walk over all
    # detections in that order visits every class's detections in the class's order
    order = np.argsort(-flat.det_score, kind="stable")
    tp = np.zeros((thr.size, flat.D), np.uint8)
    for t, th in enumerate(thr):
        seen = np.zeros(flat.G, bool)
        for d in order:
            g = best_gt[d]
            if g >= 0 and best_iou[d] >= th and not seen[g]:
                tp[t, d] = 1
                seen[g] = True
    return best_gt, best_iou, tp


def average_precision(rec, prec):
    """Evaluator.CalculateAveragePrecision (:291-311): the area under the precision envelope, the terms added one after the other."""
    mrec = np.concatenate([[0.0], rec, [1.0]])
    mpre = np.concatenate([[0.0], prec, [0.0]])
    mpre = np.maximum.accumulate(mpre[::-1])[::-1]
    ii = np.flatnonzero(mrec[1:] != mrec[:-1]) + 1
    terms = (mrec[ii] - mrec[ii - 1]) * mpre[ii]
    return np.add.accumulate(terms)[-1] if terms.size else np.float64(0.0)


def _curves(flat, thr, groups, tp_sorted, acc_tp):
    """The result from the per-class order: groups[c] = (start, stop) into the class-grouped descending-score order, tp_sorted /
    acc_tp [T, D] the flags and their per-class running sums in that order."""
    npos = np.bincount(flat.gt_cls, minlength=len(flat.classes))
    out = {"classes": list(flat.classes), "thresholds": [float(t) for t in thr], "results": []}
    for t, th in enumerate(thr):
        per_class, acc_ap, valid = {}, 0, 0
        for c, label in enumerate(flat.classes):
            s, e = groups[c]
            TP = tp_sorted[t, s:e].astype(np.float64)
            FP = 1.0 - TP
            acc_TP = acc_tp[t, s:e].astype(np.float64)
            acc_FP = np.arange(1, e - s + 1, dtype=np.float64) - acc_TP
            with np.errstate(divide="ignore", invalid="ignore"):
                rec = acc_TP / int(npos[c])
                prec = np.divide(acc_TP, acc_FP + acc_TP)
            ap = average_precision(rec, prec)
            per_class[label] = {"precision": prec, "recall": rec, "AP": ap, "total positives": int(npos[c]),
                                "total TP": np.sum(TP), "total FP": np.sum(FP), "TP": TP, "FP": FP, "acc TP": acc_TP, "acc FP": acc_FP}
            if npos[c] > 0:                                            # pascalvoc.py:363-365
                valid += 1
                acc_ap = acc_ap + ap
        out["results"].append({"threshold": float(th), "classes": per_class, "mAP": acc_ap / valid if valid else float("nan")})
    return out


def _groups(cls_sorted, n_classes):
    counts = np.bincount(cls_sorted, minlength=n_classes)
    stops = np.cumsum(counts)
    return [(int(stops[c] - counts[c]), int(stops[c])) for c in range(n_classes)]


def _restart_per_class(acc, groups):
    """Running sums over the whole class-grouped order [T, D] -> running sums that start again with every class."""
    out = acc.copy()
    for s, e in groups:
        if s > 0 and e > s:
            out[:, s:e] = acc[:, s:e] - acc[:, s - 1:s]
    return out


def voc_metrics_host(gt_data, pred_data, iou_thresholds=(0.5,)):
    flat = Flat(gt_data, pred_data)
    thr = _thresholds(iou_thresholds)
    _, _, tp = voc_match_host(flat, thr)
    order = np.argsort(-flat.det_score, kind="stable")
    order = order[np.argsort(flat.det_cls[order], kind="stable")]
    groups = _groups(flat.det_cls[order], len(flat.classes))
    tp_sorted = tp[:, order]
    return _curves(flat, thr, groups, tp_sorted, _restart_per_class(np.cumsum(tp_sorted, axis=1, dtype=np.int64), groups))


def voc_metrics_device(gt_data, pred_data, iou_thresholds=(0.5,), device=None):
    import torch
    from . import ops
    flat = Flat(gt_data, pred_data)
    thr = _thresholds(iou_thresholds)
    dev = model_device(None) if device is None else device
    if flat.D == 0 or flat.I == 0:
        empty = np.zeros((thr.size, 0), np.int64)
        return _curves(flat, thr, _groups(flat.det_cls, len(flat.classes)), empty.astype(np.uint8), empty)
    det_cls = torch.from_numpy(flat.det_cls).to(dev)
    det_score = torch.from_numpy(flat.det_score).to(dev)
    _, _, tp = ops.voc_match(torch.from_numpy(flat.det_box).to(dev), det_cls, det_score, flat.det_off,
                             torch.from_numpy(flat.gt_box).to(dev), torch.from_numpy(flat.gt_cls).to(dev), flat.gt_off,
                             torch.from_numpy(thr).to(dev))
    order = torch.sort(det_score, descending=True, stable=True).indices
    cls_sorted, by_class = torch.sort(det_cls[order], stable=True)
    order = order[by_class]
    tp_sorted = tp[:, order]
    acc = torch.cumsum(tp_sorted, dim=1, dtype=torch.int64)
    groups = _groups(cls_sorted.cpu().numpy(), len(flat.classes))
    return _curves(flat, thr, groups, tp_sorted.cpu().numpy(), _restart_per_class(acc.cpu().numpy(), groups))


def voc_metrics(gt_data, pred_data, iou_thresholds=(0.5,)):
    """The device form from DEVICE_MIN_DETECTIONS detections on, where a GPU is present; else the host form.  Same numbers."""
    n_det = sum(len(img) for img in pred_data)
    if n_det >= DEVICE_MIN_DETECTIONS and model_has_gpu(None):
        return voc_metrics_device(gt_data, pred_data, iou_thresholds)
    return voc_metrics_host(gt_data, pred_data, iou_thresholds)


def same_metrics(a, b):
    """True when two results hold the same numbers, NaN equal to NaN."""
    if a["classes"] != b["classes"] or a["thresholds"] != b["thresholds"]:
        return False
    for ra, rb in zip(a["results"], b["results"]):
        if not np.array_equal(np.float64(ra["mAP"]), np.float64(rb["mAP"]), equal_nan=True):
            return False
        for label in a["classes"]:
            ca, cb = ra["classes"][label], rb["classes"][label]
            if sorted(ca) != sorted(cb):
                return False
            for k in ca:
                x, y = np.asarray(ca[k], dtype=np.float64), np.asarray(cb[k], dtype=np.float64)
                if x.shape != y.shape or not np.array_equal(x, y, equal_nan=True):
                    return False
    return True


# ---- the external tools' input files (mrcnn/analyze.py:458-575) -------------------------------------------------
def write_metric_files(gt_data, pred_data, image_names, outdir):
    """Under `outdir`: Object-Detection-Metrics/{groundtruths,detections}/<i>.txt (``label c0 c1 c2 c3`` resp. ``label score c0 c1
    c2 c3`` per row), tarlen5-calculate-mean-ap/{ground_truth_boxes,predicted_boxes}.json (per image index ``boxes``, ``class``
    and ``scores``) and metric-computation/{ground_truth_boxes,predicted_boxes}.json (per image name ``labels``, ``boxes`` as
    [x1, y1, x2, y2] and ``scores``).  Returns the paths written."""
    written = []

    def folder(*parts):
        path = os.path.join(outdir, *parts)
        os.makedirs(path, exist_ok=True)
        return path

    def dump(obj, *parts):
        path = os.path.join(folder(*parts[:-1]), parts[-1])
        with open(path, "w") as fp:
            json.dump(obj, fp)
        written.append(path)

    gt_dir, det_dir = folder("Object-Detection-Metrics", "groundtruths"), folder("Object-Detection-Metrics", "detections")
    for i, (gt_image, pred_image) in enumerate(zip(gt_data, pred_data)):
        for path, rows, lead in ((os.path.join(gt_dir, "%d.txt" % i), gt_image, 1), (os.path.join(det_dir, "%d.txt" % i), pred_image, 2)):
            with open(path, "w") as fp:
                for row in rows:
                    head = row[4] if lead == 1 else row[4] + " " + str(row[5])
                    fp.write(head + " " + " ".join(str(v) for v in row[0:4]) + "\n")
            written.append(path)
    gt_dict, pred_dict = {}, {}
    for i, (gt_image, pred_image) in enumerate(zip(gt_data, pred_data)):
        gt_dict[str(i)] = {"boxes": [row[0:4] for row in gt_image], "class": [row[4] for row in gt_image]}
        pred_dict[str(i)] = {"boxes": [row[0:4] for row in pred_image], "class": [row[4] for row in pred_image],
                             "scores": [row[5] for row in pred_image]}
    dump(gt_dict, "tarlen5-calculate-mean-ap", "ground_truth_boxes.json")
    dump(pred_dict, "tarlen5-calculate-mean-ap", "predicted_boxes.json")
    gt_dict, pred_dict = {}, {}
    for i, (gt_image, pred_image) in enumerate(zip(gt_data, pred_data)):
        name = image_names[i].split(os.sep)[-1]
        gt_dict[name] = {"labels": [row[4] for row in gt_image], "boxes": [[row[1], row[0], row[3], row[2]] for row in gt_image]}
        pred_dict[name] = {"labels": [row[4] for row in pred_image], "boxes": [[row[1], row[0], row[3], row[2]] for row in pred_image],
                           "scores": [row[5] for row in pred_image]}
    dump(gt_dict, "metric-computation", "ground_truth_boxes.json")
    dump(pred_dict, "metric-computation", "predicted_boxes.json")
    return written


# ---- mask AP with the overlaps from the device ---------------------------------------------------------------------
def mask_overlaps_device(pred_masks_device, gt_masks, device=None):
    """utils.compute_overlaps_masks(pred, gt) -> [P, G] float32 from bit planes: `pred_masks_device` the [H, W, P] uint8 / bool
    device tensor of the last detect (MaskRCNN.last_masks_device; None without detections), `gt_masks` [H, W, G] on the host,
    uploaded once.  Two ops.mask_planes_pack and one ops.mask_cross_stats launch; the division is the host's, in float32 as
    compute_overlaps_masks forms it: equal bit for bit while H * W < 2^24 (the caller's check)."""
    import torch
    from . import ops
    P = 0 if pred_masks_device is None else int(pred_masks_device.shape[-1])
    G = int(gt_masks.shape[-1])
    if P == 0 or G == 0:
        return np.zeros((P, G))
    dev = pred_masks_device.device if device is None else device
    a = ops.mask_planes_pack(pred_masks_device.contiguous())
    gt = np.ascontiguousarray(np.asarray(gt_masks) > .5)
    b = ops.mask_planes_pack(torch.from_numpy(gt.view(np.uint8)).to(dev))
    inter = ops.mask_cross_stats(a, b).cpu().numpy().astype(np.float32)
    count_a, count_b = a.count.cpu().numpy().astype(np.float32), b.count.cpu().numpy().astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        return inter / (count_a[:, None] + count_b[None, :] - inter)


def mask_ap(gt_boxes, gt_class_ids, gt_masks, result, masks_device=None, iou_threshold=0.5):
    """utils.compute_ap of one image's detect result; with `masks_device` (the device tensor behind result["masks"]) the overlaps
    come from mask_overlaps_device, rows taken in the score order compute_matches walks."""
    overlaps = None
    H, W = gt_masks.shape[:2]
    if masks_device is not None and H * W < EXACT_PIXELS and tuple(masks_device.shape) == tuple(result["masks"].shape):
        n_gt = int(np.any(gt_boxes != 0, axis=1).sum())
        n_pred = int(np.any(result["rois"] != 0, axis=1).sum())
        order = np.argsort(result["scores"][:n_pred])[::-1]
        overlaps = mask_overlaps_device(masks_device, gt_masks[..., :n_gt])[order]
    return utils.compute_ap(gt_boxes, gt_class_ids, gt_masks, result["rois"], result["class_ids"], result["scores"], result["masks"],
                            iou_threshold, overlaps=overlaps)
