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
  sweep_metrics_host / _device / sweep_metrics   what the second vendored tool (tarlen5-calculate-mean-ap/calculate.py) computes: the
                      precision / recall curve over every score threshold and the mAP over IoU 0.50 ... 0.95; the matching of
                      every image at every score threshold is one ops.ap_sweep launch (csrc/apsweep.hip).  See below.
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


# ---- the sweep mAP of the second vendored tool (tarlen5-calculate-mean-ap/calculate.py) -------------------------------
# The tool walks every distinct model score s of the set, keeps the detections with score > s and matches each image again.  Within
# an image sorted ascending by score the kept set is a suffix, so an image has only P + 1 outcomes per IoU threshold: the suffix
# table tp[t][k] (detections k .. P - 1 kept).  Every point of the precision / recall curve is then a sum of table entries.
#   sweep_tables_host    the tables, problem by problem, in NumPy: the statement of ops.ap_sweep (csrc/apsweep.hip)
#   sweep_metrics_host   the tool's numbers from them; sweep_metrics_device the same with the tables from one launch and the sums as
#                        torch integer calls on the device; sweep_metrics picks one of the two
# A result is {"classes", "thresholds", "class_thresholds", "results": [per threshold, class-blind: {"threshold", "avg_prec",
# "precisions", "recalls", "model_thrs"}], "mAP": 100 * mean of the avg_prec rounded to four decimals, "per_class": {label: [per
# class threshold the same five]}}.

# sweep_metrics takes the device form from this many detections on: the measured break-even (tools/sweep_bench.py,
# profiles/sweep_bench.json `break_even_detections`: the smallest measured test set from which on the device form was ahead -- 2
# images, 63 detections, 1.33 ms against 1.12 ms; at 1 image, 27 detections, the host form won, 0.96 ms against 1.06 ms).  None
# would send everything to the host form.
SWEEP_DEVICE_MIN_DETECTIONS = 63
SWEEP_IOU_THRESHOLDS = tuple(float(t) for t in np.linspace(0.5, 0.95, 10))        # __main__ :458
SWEEP_CLASS_THRESHOLDS = (0.5, 0.6)                                               # np.linspace(0.5, 0.6, 2), :586


class SweepProblems(object):
    """The flat problem table of ops.ap_sweep.  A problem is one (image, class filter) pair: the I images with every row first
    (group 0), then the I images with the rows of class 0 only (group 1), of class 1 (group 2), ... -- as split_boxes_by_class
    keeps every image, with possibly empty lists.  det_box [D, 4] / gt_box [G, 4] float64, det_score [D] float64, det_off / gt_off
    [N + 1] int64; a problem's detections are in the order np.argsort(scores) gives them (ascending, as the tool sorts them), its
    ground truths in row order.  group [N] int32.  A malformed box (c0 > c2 or c1 > c3: the tool raises on it) or a number that is
    not finite is a ValueError."""

    def __init__(self, gt_data, pred_data):
        flat = Flat(gt_data, pred_data)
        for what, box in (("ground-truth", flat.gt_box), ("detection", flat.det_box)):
            if not bool(np.all(np.isfinite(box))):
                raise ValueError("a %s box holds a number that is not finite" % what)
            bad = np.flatnonzero((box[:, 0] > box[:, 2]) | (box[:, 1] > box[:, 3]))
            if bad.size:
                raise ValueError("%s box is malformed: %r" % (what, box[bad[0]].tolist()))
        if not bool(np.all(np.isfinite(flat.det_score))):
            raise ValueError("a detection score is not finite")
        self.classes, self.I = flat.classes, flat.I
        n_groups = 1 + len(flat.classes)
        det_rows, gt_rows, det_n, gt_n = [], [], [], []
        for grp in range(n_groups):
            for i in range(flat.I):
                d = np.arange(flat.det_off[i], flat.det_off[i + 1])
                g = np.arange(flat.gt_off[i], flat.gt_off[i + 1])
                if grp:
                    d, g = d[flat.det_cls[d] == grp - 1], g[flat.gt_cls[g] == grp - 1]
                d = d[np.argsort(flat.det_score[d])]
                det_rows.append(d)
                gt_rows.append(g)
                det_n.append(d.size)
                gt_n.append(g.size)
        det_rows = np.concatenate(det_rows) if det_rows else np.zeros(0, np.int64)
        gt_rows = np.concatenate(gt_rows) if gt_rows else np.zeros(0, np.int64)
        self.det_box = np.ascontiguousarray(flat.det_box[det_rows]).reshape(-1, 4)
        self.gt_box = np.ascontiguousarray(flat.gt_box[gt_rows]).reshape(-1, 4)
        self.det_score = flat.det_score[det_rows]
        self.det_off = np.concatenate([[0], np.cumsum(det_n, dtype=np.int64)]).astype(np.int64)
        self.gt_off = np.concatenate([[0], np.cumsum(gt_n, dtype=np.int64)]).astype(np.int64)
        self.group = np.repeat(np.arange(n_groups, dtype=np.int32), flat.I)
        self.N, self.D, self.G, self.n_groups = n_groups * flat.I, int(self.det_off[-1]), int(self.gt_off[-1]), n_groups

    def select(self, keep):
        """The table of the problems keep[p] is set for, in order (no groups: a table for ops.ap_sweep / sweep_tables_host)."""
        keep = np.asarray(keep, bool)
        out = object.__new__(SweepProblems)
        dn, gn = np.diff(self.det_off), np.diff(self.gt_off)
        out.det_box = np.ascontiguousarray(self.det_box[np.repeat(keep, dn)])
        out.gt_box = np.ascontiguousarray(self.gt_box[np.repeat(keep, gn)])
        out.det_score = self.det_score[np.repeat(keep, dn)]
        out.det_off = np.concatenate([[0], np.cumsum(dn[keep])]).astype(np.int64)
        out.gt_off = np.concatenate([[0], np.cumsum(gn[keep])]).astype(np.int64)
        out.N, out.D, out.G = int(keep.sum()), int(out.det_off[-1]), int(out.gt_off[-1])
        return out


def sweep_iou_matrix(pred, gt):
    """calc_iou_individual (:40-77) of every box of pred [P, 4] against every box of gt [G, 4], float64, operation for operation."""
    p0, p1, p2, p3 = (pred[:, k][:, None] for k in range(4))
    t0, t1, t2, t3 = (gt[:, k][None, :] for k in range(4))
    apart = (t2 < p0) | (p2 < t0) | (t3 < p1) | (p3 < t1)
    inter = (np.minimum(t2, p2) - np.maximum(t0, p0) + 1) * (np.minimum(t3, p3) - np.maximum(t1, p1) + 1)
    area_t = (t2 - t0 + 1) * (t3 - t1 + 1)
    area_p = (p2 - p0 + 1) * (p3 - p1 + 1)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(apart, 0.0, inter / (area_t + area_p - inter))


def sweep_table_entries(problems, T):
    """(start [N], rows [N]) int64: problem p's table is tp[start[p] : start[p] + T * rows[p]], T rows of rows[p] = P + 1."""
    return T * (problems.det_off[:-1] + np.arange(problems.N, dtype=np.int64)), np.diff(problems.det_off) + 1


def sweep_tables_host(flat_problem, thresholds, only=None):
    """The host statement of ops.ap_sweep: (tp [T * (D + N)] int32, status [N] int32, all 0).  Per problem and threshold t,
    tp[t][k] = the matches of get_single_image_results (:80-139) on detections k .. P - 1: the pairs with iou > thr[t] in
    detection-major order, walked by np.argsort(ious, kind="stable")[::-1] (the tool's order where no two IoUs of the problem are
    bit-equal; where some are, the tool's own order is NumPy's unstable sort's), a pair matched when both its sides are free.
    The walk runs once per problem, for every (t, k) at the same time.  `only`: the problems to compute (the others stay 0)."""
    thr = _thresholds(thresholds)
    T, pr = thr.size, flat_problem
    start, rows = sweep_table_entries(pr, T)
    tp = np.zeros(T * (pr.D + pr.N), np.int32)
    tmin = thr.min()
    for p in (range(pr.N) if only is None else only):
        d0, d1, g0, g1 = pr.det_off[p], pr.det_off[p + 1], pr.gt_off[p], pr.gt_off[p + 1]
        P, G = int(d1 - d0), int(g1 - g0)
        if P == 0 or G == 0:
            continue
        iou = sweep_iou_matrix(pr.det_box[d0:d1], pr.gt_box[g0:g1])
        dd, gg = np.nonzero(iou > tmin)                                  # row-major: detection-major, ground-truth-minor
        vals = iou[dd, gg]
        ks = np.arange(P + 1)
        det_taken = np.zeros((T, P + 1, P), bool)
        gt_taken = np.zeros((T, P + 1, G), bool)
        count = np.zeros((T, P + 1), np.int32)
        for c in np.argsort(vals, kind="stable")[::-1]:
            d, g = dd[c], gg[c]
            match = (vals[c] > thr)[:, None] & (ks <= d)[None, :] & ~det_taken[:, :, d] & ~gt_taken[:, :, g]
            det_taken[:, :, d] |= match
            gt_taken[:, :, g] |= match
            count += match
        tp[start[p]:start[p] + T * rows[p]] = count.reshape(-1)
    return tp, np.zeros(pr.N, np.int32)


def _sweep_bins(pr):
    """The model-score bins: per group the sorted distinct scores of its detections.  (scores [B] float64 -- the groups' bins one
    after the other --, bin_off [n_groups + 1], row_bin [D]: the bin of every detection row)."""
    group_of_row = np.repeat(pr.group, np.diff(pr.det_off))
    scores, bin_off, row_bin = [], [0], np.zeros(pr.D, np.int64)
    for grp in range(pr.n_groups):
        rows = np.flatnonzero(group_of_row == grp)
        uniq, inv = np.unique(pr.det_score[rows], return_inverse=True)
        row_bin[rows] = bin_off[-1] + inv.reshape(-1)
        scores.append(uniq)
        bin_off.append(bin_off[-1] + uniq.size)
    return np.concatenate(scores) if scores else np.zeros(0), np.array(bin_off, np.int64), row_bin


def _sweep_gather_index(pr, T):
    """Where the sums read the tables: entry [T, D] of tp[t][q] for every detection row (q its place in its problem), first [T, N] of
    tp[t][0] for every problem."""
    start, rows = sweep_table_entries(pr, T)
    dn = np.diff(pr.det_off)
    q = np.arange(pr.D, dtype=np.int64) - np.repeat(pr.det_off[:-1], dn)
    t = np.arange(T, dtype=np.int64)[:, None]
    return np.repeat(start, dn)[None, :] + t * np.repeat(rows, dn)[None, :] + q[None, :], start[None, :] + t * rows[None, :]


def _sweep_true_positives_host(pr, T, tp, bin_off, row_bin):
    """TP [T, B] int64: per threshold and score bin j the matches summed over the group's images when the detections with a score
    <= the bin's are dropped -- tp_i[t][k_i] with k_i = searchsorted(scores_i, s, "right"), as the sum of tp_i[t][0] and the
    steps tp_i[t][q + 1] - tp_i[t][q] of the dropped rows.  Integers throughout."""
    entry, first = _sweep_gather_index(pr, T)
    B = int(bin_off[-1])
    tp = tp.astype(np.int64)
    step = tp[entry + 1] - tp[entry]
    acc = np.zeros((T, B), np.int64)
    for t in range(T):
        np.add.at(acc[t], row_bin, step[t])
    acc = np.cumsum(acc, axis=1)
    base = np.zeros((T, pr.n_groups), np.int64)
    for t in range(T):
        np.add.at(base[t], pr.group, tp[first[t]])
    return _sweep_restart_per_group(acc, base, bin_off)


def _sweep_restart_per_group(acc, base, bin_off):
    out = acc.copy()
    for grp in range(base.shape[1]):
        s, e = int(bin_off[grp]), int(bin_off[grp + 1])
        if e > s:
            out[:, s:e] = acc[:, s:e] - (acc[:, s - 1:s] if s > 0 else 0) + base[:, grp:grp + 1]
    return out


def _sweep_point_curve(tp, kept, n_gt, model_thrs):
    """calc_precision_recall (:142-171) per model threshold and the eleven-point rule of get_avg_precision_at_iou (:262-272)."""
    fp, fn = kept - tp, n_gt - tp
    with np.errstate(divide="ignore", invalid="ignore"):
        precisions = np.where(tp + fp == 0, 0.0, tp / (tp + fp))
        recalls = np.where(tp + fn == 0, 0.0, tp / (tp + fn))
    prec_at_rec = []
    for level in np.linspace(0.0, 1.0, 11):
        sel = recalls >= level
        prec_at_rec.append(precisions[sel].max() if bool(sel.any()) else 0.0)
    return {"avg_prec": np.mean(prec_at_rec), "precisions": precisions, "recalls": recalls, "model_thrs": [float(s) for s in model_thrs]}


def _sweep_result(pr, iou_thr, cls_thr, thr_all, TP, scores, bin_off, row_bin):
    """The result from TP [len(thr_all), B]: everything else -- kept detections per bin, ground truths per group, the divisions and
    the eleven-point rule -- is the host's."""
    B = int(bin_off[-1])
    dropped = np.cumsum(np.bincount(row_bin, minlength=B).astype(np.int64))
    group_of_row = np.repeat(pr.group, np.diff(pr.det_off))
    n_det = np.bincount(group_of_row, minlength=pr.n_groups).astype(np.int64)
    n_gt = np.bincount(np.repeat(pr.group, np.diff(pr.gt_off)), minlength=pr.n_groups).astype(np.int64)

    def curve(grp, th):
        t = int(np.flatnonzero(thr_all == th)[0])
        s, e = int(bin_off[grp]), int(bin_off[grp + 1])
        last = max(e - 1, s)                                             # the model thresholds are S[:-1]
        kept = n_det[grp] - (dropped[s:last] - (dropped[s - 1] if s > 0 else 0))
        out = _sweep_point_curve(TP[t, s:last], kept, n_gt[grp], scores[s:last])
        out["threshold"] = float(th)
        return out

    res = {"classes": list(pr.classes), "thresholds": [float(t) for t in iou_thr], "class_thresholds": [float(t) for t in cls_thr],
           "results": [curve(0, th) for th in iou_thr]}
    rounded = [float("{:.4f}".format(r["avg_prec"])) for r in res["results"]]
    res["mAP"] = 100 * np.mean(rounded)
    res["per_class"] = {label: [curve(1 + c, th) for th in cls_thr] for c, label in enumerate(pr.classes)}
    return res


def _sweep_thresholds(iou_thresholds, class_thresholds):
    iou_thr, cls_thr = _thresholds(iou_thresholds), _thresholds(class_thresholds)
    return iou_thr, cls_thr, np.unique(np.concatenate([iou_thr, cls_thr]))


def sweep_metrics_host(gt_data, pred_data, iou_thresholds=SWEEP_IOU_THRESHOLDS, class_thresholds=SWEEP_CLASS_THRESHOLDS):
    """What calculate.py computes from the two JSON files write_metric_files writes: get_avg_precision_at_iou class-blind at every
    IoU threshold, its mAP, and per class (the sorted labels present; the tool hard-codes run.py's three) at the class thresholds."""
    iou_thr, cls_thr, thr_all = _sweep_thresholds(iou_thresholds, class_thresholds)
    pr = SweepProblems(gt_data, pred_data)
    scores, bin_off, row_bin = _sweep_bins(pr)
    tp, _ = sweep_tables_host(pr, thr_all)
    TP = _sweep_true_positives_host(pr, thr_all.size, tp, bin_off, row_bin)
    return _sweep_result(pr, iou_thr, cls_thr, thr_all, TP, scores, bin_off, row_bin)


def sweep_tables_device(pr, thr, dev, handed_back=None):
    """tp [T * (D + N)] int32 on `dev` for the whole table, T <= the kernel's threshold cap: one ops.ap_sweep launch over the
    problems within the row caps; the others, and the ones the kernel reports an overflowing candidate list for, come from
    sweep_tables_host and are written into the device table.  `handed_back`: a list that receives those problems' indices."""
    import torch
    from . import ops
    caps = ops.ap_sweep_caps()
    T = thr.size
    fits = (np.diff(pr.det_off) <= caps["det"]) & (np.diff(pr.gt_off) <= caps["gt"])
    start, rows = sweep_table_entries(pr, T)
    host = np.flatnonzero(~fits)
    if bool(fits.all()):
        tp, status = ops.ap_sweep(torch.from_numpy(pr.det_box).to(dev), pr.det_off, torch.from_numpy(pr.gt_box).to(dev), pr.gt_off,
                                  torch.from_numpy(thr).to(dev))
        host = np.flatnonzero(status.cpu().numpy() != ops.AP_SWEEP_OK)
    else:
        tp = torch.zeros((T * (pr.D + pr.N),), dtype=torch.int32, device=dev)
        if bool(fits.any()):
            sub = pr.select(fits)
            sub_tp, status = ops.ap_sweep(torch.from_numpy(sub.det_box).to(dev), sub.det_off, torch.from_numpy(sub.gt_box).to(dev),
                                          sub.gt_off, torch.from_numpy(thr).to(dev))
            sent = np.flatnonzero(fits)
            # the sent problems' entries, in order, are the sub-table's entries
            where = np.concatenate([np.arange(start[p], start[p] + T * rows[p]) for p in sent])
            tp[torch.from_numpy(where).to(dev)] = sub_tp
            host = np.sort(np.concatenate([host, sent[status.cpu().numpy() != ops.AP_SWEEP_OK]]))
    if host.size:
        host_tp, _ = sweep_tables_host(pr, thr, only=[int(p) for p in host])
        where = np.concatenate([np.arange(start[p], start[p] + T * rows[p]) for p in host])
        tp[torch.from_numpy(where).to(dev)] = torch.from_numpy(host_tp[where]).to(dev)
    if handed_back is not None:
        handed_back.extend(int(p) for p in host)
    return tp


def sweep_metrics_device(gt_data, pred_data, iou_thresholds=SWEEP_IOU_THRESHOLDS, class_thresholds=SWEEP_CLASS_THRESHOLDS, device=None,
                         handed_back=None):
    """sweep_metrics_host with the suffix tables from one ops.ap_sweep launch over every problem of the set (csrc/apsweep.hip) and
    the curve sums -- steps gathered from the tables, added per score bin, running sums -- as torch integer calls on the device;
    the divisions and the eleven-point rule are the host's.  More thresholds than the kernel takes go in several launches."""
    import torch
    from . import ops
    iou_thr, cls_thr, thr_all = _sweep_thresholds(iou_thresholds, class_thresholds)
    pr = SweepProblems(gt_data, pred_data)
    scores, bin_off, row_bin = _sweep_bins(pr)
    dev = model_device(None) if device is None else device
    B, cap = int(bin_off[-1]), ops.ap_sweep_caps()["thr"]
    parts = []
    if pr.N > 0 and pr.D > 0:
        row_bin_t, group_t = torch.from_numpy(row_bin).to(dev), torch.from_numpy(pr.group.astype(np.int64)).to(dev)
        for t0 in range(0, thr_all.size, cap):
            thr = np.ascontiguousarray(thr_all[t0:t0 + cap])
            T = thr.size
            tp = sweep_tables_device(pr, thr, dev, handed_back if t0 == 0 else None).to(torch.int64)
            entry, first = (torch.from_numpy(a).to(dev) for a in _sweep_gather_index(pr, T))
            step = tp[entry + 1] - tp[entry]
            acc = torch.zeros((T, B), dtype=torch.int64, device=dev).index_add_(1, row_bin_t, step)
            base = torch.zeros((T, pr.n_groups), dtype=torch.int64, device=dev).index_add_(1, group_t, tp[first])
            parts.append(_sweep_restart_per_group(torch.cumsum(acc, dim=1).cpu().numpy(), base.cpu().numpy(), bin_off))
    TP = np.concatenate(parts, axis=0) if parts else np.zeros((thr_all.size, B), np.int64)
    return _sweep_result(pr, iou_thr, cls_thr, thr_all, TP, scores, bin_off, row_bin)


def sweep_metrics(gt_data, pred_data, iou_thresholds=SWEEP_IOU_THRESHOLDS, class_thresholds=SWEEP_CLASS_THRESHOLDS):
    """The device form from SWEEP_DEVICE_MIN_DETECTIONS detections on (None: never), where a GPU is present; else the host form.
    Same numbers."""
    n_det = sum(len(img) for img in pred_data)
    if SWEEP_DEVICE_MIN_DETECTIONS is not None and n_det >= SWEEP_DEVICE_MIN_DETECTIONS and model_has_gpu(None):
        return sweep_metrics_device(gt_data, pred_data, iou_thresholds, class_thresholds)
    return sweep_metrics_host(gt_data, pred_data, iou_thresholds, class_thresholds)


def same_sweep(a, b):
    """True when two sweep results hold the same numbers, bit for bit."""
    if any(a[k] != b[k] for k in ("classes", "thresholds", "class_thresholds")) or sorted(a["per_class"]) != sorted(b["per_class"]):
        return False
    if not np.array_equal(np.float64(a["mAP"]), np.float64(b["mAP"]), equal_nan=True):
        return False
    pairs = list(zip(a["results"], b["results"]))
    for label in a["classes"]:
        pairs += list(zip(a["per_class"][label], b["per_class"][label]))
    for ra, rb in pairs:
        if sorted(ra) != sorted(rb):
            return False
        for k in ra:
            x, y = np.asarray(ra[k], dtype=np.float64), np.asarray(rb[k], dtype=np.float64)
            if x.shape != y.shape or not np.array_equal(x, y, equal_nan=True):
                return False
    return True


def format_sweep(result, classes=None):
    """The lines calculate.py's __main__ prints (:437-478, :612-623; not the two timing lines), formatted as it formats them: per
    class `<Label> avg precision` at the first class threshold, `avg precision` class-blind at the first IoU threshold, then
    `map:` / `avg precs:` / `iou_thrs:` over the IoU thresholds and over classes x class thresholds -- every AP rounded to four
    decimals before the mean.  `classes`: the labels and their order (the tool's are source, sidelobe, galaxy); default the
    result's.  A label the data does not hold has no score threshold, hence AP 0, as in the tool."""
    labels = list(result["classes"] if classes is None else classes)
    cls_thr = result["class_thresholds"]

    def ap(label, k):
        return result["per_class"][label][k]["avg_prec"] if label in result["per_class"] else 0.0
    lines = ["{} avg precision: {:.4f}".format(label.capitalize(), ap(label, 0)) for label in labels]
    lines.append("avg precision: {:.4f}".format(result["results"][0]["avg_prec"]))
    blocks = [([r["avg_prec"] for r in result["results"]], result["thresholds"]),
              ([ap(label, k) for label in labels for k in range(len(cls_thr))], [t for _ in labels for t in cls_thr])]
    for avg_precs, iou_thrs in blocks:
        if not avg_precs:                                                # no label at all: the tool always has its three
            continue
        avg_precs =[float("{:.4f}".format(v)) for v in avg_precs]
        iou_thrs = [float("{:.4f}".format(t)) for t in iou_thrs]
        lines.append("map: {:.2f}".format(100 * np.mean(avg_precs)))
        lines.append("avg precs:  " + str(avg_precs))
        lines.append("iou_thrs:   " + str(iou_thrs))
    return lines


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
