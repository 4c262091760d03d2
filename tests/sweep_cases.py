"""Test sets for the sweep mAP (caesar-mrcnn_amd/metrics.py: sweep_metrics_*, csrc/apsweep.hip), the flat record a result is
compared through, and a brute-force statement of the tool's loop.  tests/golden/make_sweep_fixtures.py records the reference's
side -- tarlen5-calculate-mean-ap/calculate.py run on these rows -- into tests/golden/sweep.npz.

Rows are ``[c0, c1, c2, c3, label]`` / ``[c0, c1, c2, c3, label, score]`` with inclusive corners, as the tool counts them: a box
(0, 0, 9, 9) holds 10 x 10 pixels."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sweep.npz")
LABELS = ("source", "sidelobe", "galaxy")                  # the tool's hard-coded three, in the order its __main__ takes them
IOU_THRESHOLDS = tuple(float(t) for t in np.linspace(0.5, 0.95, 10))
CLASS_THRESHOLDS = (0.5, 0.6)
FIELDS = ("avg_prec", "precisions", "recalls", "model_thrs")
MAIN_SETS = ("seeded_small", "hand_mixed")                 # the sets the tool's __main__ is run on as well

B10 = [0, 0, 9, 9]                       # 10 x 10


def inside(n):
    """10 x n inside B10: IoU n / 10 exactly ... with n = 5: 0.5, not above the threshold 0.5."""
    return [0, 0, 9, n - 1]


def _shift(box, dy, dx=0):
    return [box[0] + dy, box[1] + dx, box[2] + dy, box[3] + dx]


def seeded(n_images, max_det, max_gt, seed, score_places, grid=None, frame=200.0):
    """Images with 0 .. max_gt true boxes and 0 .. max_det detections of the three classes.  About two thirds of the true boxes are
    detected with their corners moved; the other detections lie anywhere.  grid None: corners are floats drawn from a continuum, so
    no two IoUs of an image are bit-equal (checked by the generator of the fixture); grid g: corners on multiples of g and many
    detections ARE a true box, so equal IoUs are frequent.  Scores are rounded to `score_places` decimals (None: not rounded)."""
    rng = np.random.default_rng(seed)

    def score():
        s = float(rng.uniform(0.3, 1.0))
        return s if score_places is None else round(s, score_places)

    def anywhere():
        if grid:
            y, x = (float(v) * grid for v in rng.integers(0, 6, 2))
            h, w = (float(v) * grid for v in rng.integers(1, 4, 2))
            return [y, x, y + h - 1, x + w - 1]
        y, x = (float(v) for v in rng.uniform(0, frame - 50, 2))
        h, w = (float(v) for v in rng.uniform(5, 45, 2))
        return [y, x, y + h, x + w]
    gt_data, pred_data = [], []
    for i in range(n_images):
        n_gt = 0 if i % 5 == 3 else int(rng.integers(0, max_gt + 1))
        n_det = 0 if i % 5 == 4 else int(rng.integers(0, max_det + 1))
        gt = [anywhere() + [LABELS[int(rng.integers(0, 3))]] for _ in range(n_gt)]
        pred = []
        for row in gt:
            if len(pred) < n_det and rng.random() < 2.0 / 3.0:
                if grid:
                    box = list(row[:4]) if rng.random() < 0.6 else [row[0], row[1], row[2], row[3] + grid]
                else:
                    lo = [row[0] + float(rng.uniform(-3, 3)), row[1] + float(rng.uniform(-3, 3))]
                    box = lo + [max(lo[0] + 1, row[2] + float(rng.uniform(-3, 3))), max(lo[1] + 1, row[3] + float(rng.uniform(-3, 3)))]
                label = row[4] if rng.random() < 0.85 else LABELS[int(rng.integers(0, 3))]
                pred.append(box + [label, score()])
        while len(pred) < n_det:
            pred.append(anywhere() + [LABELS[int(rng.integers(0, 3))], score()])
        gt_data.append(gt)
        pred_data.append([pred[k] for k in rng.permutation(len(pred))])
    return gt_data, pred_data


def sets():
    """name -> (gt_data, pred_data, tied): `tied` sets hold bit-equal IoUs within an image, where the tool's order is NumPy's
    unstable sort's -- this machine's order; the others are pinned."""
    s, l, g = LABELS
    far = [40, 40, 49, 49]
    out = {
        # up to 40 detections x 25 true boxes, scores of two decimals: equal scores within and across images
        "seeded_small": seeded(12, 40, 25, 11, 2) + (False,),
        # up to 70 x 40, scores from a continuum
        "seeded_wide": seeded(5, 70, 40, 12, None) + (False,),
        # one detection per class and image position, exact IoUs: 0.5 (10 x 5 in 10 x 10) is NOT above the threshold 0.5; 0.6 is
        # above 0.5 and 0.55, not above 0.6; boxes that share one pixel row (IoU 10 / 160); boxes one pixel apart
        "hand_mixed": ([[B10 + [s], _shift(B10, 20) + [l], _shift(B10, 40) + [g], _shift(B10, 60) + [s]],
                        [B10 + [g], far + [s]], [], [B10 + [l]]],
                       [[inside(5) + [s, 0.9], _shift(inside(6), 20) + [l, 0.8], _shift(inside(8), 40) + [g, 0.7],
                         [69, 0, 75, 9, s, 0.6], [30, 50, 35, 55, g, 0.5]],
                        [inside(9) + [g, 0.95], [50, 40, 59, 49, s, 0.85], _shift(B10, 0, 30) + [l, 0.4]],
                        [B10 + [s, 0.75]], []], False),
        # an IoU of exactly n / 20 for every one of the ten thresholds: 10 x (n / 2) ... built from 20 x 20 boxes
        "hand_twentieths": ([[_shift([0, 0, 19, 19], 0, 30 * k) + [s] for k in range(10)]],
                            [[_shift([0, 0, 19, 9 + k], 0, 30 * k) + [s, 0.5 + 0.04 * k] for k in range(10)]], False),
        # one distinct score in the whole set: no model threshold, AP 0
        "one_score": ([[B10 + [s]], [B10 + [g]]], [[B10 + [s, 0.5]], [B10 + [g, 0.5], far + [g, 0.5]]], False),
        "no_detections": ([[B10 + [s]], [far + [l], B10 + [g]]], [[], []], False),
        "no_ground_truths": ([[], []], [[B10 + [s, 0.9], far + [l, 0.8]], [B10 + [g, 0.7]]], False),
        # equal scores within and across images, every detection a hit or a clear miss
        "equal_scores": ([[B10 + [s], far + [s]], [B10 + [s]], [B10 + [s]]],
                         [[inside(8) + [s, 0.5], far + [s, 0.5], _shift(far, 20) + [s, 0.7]], [inside(9) + [s, 0.5]],
                          [_shift(far, 20) + [s, 0.7], B10 + [s, 0.9]]], False),
        # tied IoUs whose order changes the match count: the first detection lies between two true boxes (IoU 90 / 110 with
        # either), the second one reaches only the second true box (80 / 120).  The later pair first gives the first detection
        # the second true box and leaves the second detection without one: one match where the other order finds two
        "tied_pairs": ([[[0, 0, 9, 9, s], [0, 2, 9, 11, s]]],
                       [[[0, 1, 9, 10, s, 0.6], [0, 4, 9, 13, s, 0.8], far + [s, 0.9], [0, 1, 9, 10, s, 0.3]]], True),
        "tied_grid": seeded(8, 30, 20, 13, 1, grid=8) + (True,),
    }
    return out


# x1 > x2 in a detection: the tool raises as soon as it looks at the box (with two distinct scores it does)
MALFORMED = ([[B10 + ["source"]]], [[[5, 0, 4, 9, "source", 0.9], B10 + ["source", 0.5]]])


def has_tied_ious(gt_data, pred_data, iou_matrix):
    """True when some image holds two bit-equal IoUs > 0 (whatever the class: the class-blind problem holds every pair)."""
    for gt, pred in zip(gt_data, pred_data):
        if gt and pred:
            v = iou_matrix(np.array([r[:4] for r in pred], np.float64), np.array([r[:4] for r in gt], np.float64)).reshape(-1)
            v = v[v > 0]
            if np.unique(v).size < v.size:
                return True
    return False


# ---- the flat record of a result ------------------------------------------------------------------------------------
def record(result):
    """A sweep result (metrics.py's layout) as {key: float64 array}."""
    out = {"mAP": np.array([result["mAP"]], np.float64)}
    for k, res in enumerate(result["results"]):
        for f in FIELDS:
            out["t%d/%s" % (k, f)] = np.asarray(res[f], np.float64).reshape(-1)
    for label in result["classes"]:
        for k, res in enumerate(result["per_class"][label]):
            for f in FIELDS:
                out["%s/t%d/%s" % (label, k, f)] = np.asarray(res[f], np.float64).reshape(-1)
    return out


def store(prefix, gt_data, pred_data, tied, classes, rec, main_lines, out):
    out[prefix + "/input"] = np.array(json.dumps({"gt": gt_data, "pred": pred_data, "tied": bool(tied), "classes": classes,
                                                  "main": main_lines}))
    keys = sorted(rec)
    out[prefix + "/keys"] = np.array(json.dumps(keys))
    out[prefix + "/sizes"] = np.array([rec[k].size for k in keys], np.int64)
    out[prefix + "/nums"] = np.concatenate([rec[k] for k in keys]) if keys else np.zeros(0)


def load(golden, prefix):
    """(gt_data, pred_data, tied, classes, record, main_lines) of a stored set."""
    head = json.loads(str(golden[prefix + "/input"]))
    keys, sizes, nums = json.loads(str(golden[prefix + "/keys"])), golden[prefix + "/sizes"], golden[prefix + "/nums"]
    rec, at = {}, 0
    for k, n in zip(keys, sizes):
        rec[k] = nums[at:at + int(n)]
        at += int(n)
    assert at == nums.size
    return head["gt"], head["pred"], head["tied"], head["classes"], rec, head["main"]


def differences(got, want):
    """The keys at which two records differ (`==` on every float64, NaN equal to NaN)."""
    if sorted(got) != sorted(want):
        return sorted(set(got) ^ set(want))
    bad = []
    for k in sorted(want):
        a, b = np.asarray(got[k], np.float64), np.asarray(want[k], np.float64)
        if a.shape != b.shape or not bool(np.all((a == b) | (np.isnan(a) & np.isnan(b)))):
            bad.append(k)
    return bad


def golden_sets(golden):
    return sorted(set(k.split("/")[0] for k in golden.files if k.endswith("/input")))


# ---- the tool's loop, by brute force ---------------------------------------------------------------------------------
def iou_one(p, t):
    """One predicted box against one true box, the tool's operations on Python floats."""
    if t[2] < p[0] or p[2] < t[0] or t[3] < p[1] or p[3] < t[1]:
        return 0.0
    inter = (min(t[2], p[2]) - max(t[0], p[0]) + 1) * (min(t[3], p[3]) - max(t[1], p[1]) + 1)
    return inter / ((t[2] - t[0] + 1) * (t[3] - t[1] + 1) + (p[2] - p[0] + 1) * (p[3] - p[1] + 1) - inter)


def image_matches(gt_boxes, kept_boxes, iou_thr):
    """tp of one image: the pairs above the threshold in detection-major order, taken by np.argsort(kind="stable")[::-1], a pair
    matched when both sides are free."""
    pairs, ious = [], []
    for d, p in enumerate(kept_boxes):
        for g, t in enumerate(gt_boxes):
            v = iou_one(p, t)
            if v > iou_thr:
                pairs.append((d, g))
                ious.append(v)
    used_d, used_g = set(), set()
    for c in np.argsort(np.array(ious, np.float64), kind="stable")[::-1]:
        d, g = pairs[c]
        if d not in used_d and g not in used_g:
            used_d.add(d)
            used_g.add(g)
    return len(used_d)


def brute_curve(gt_images, pred_images, iou_thr):
    """get_avg_precision_at_iou by brute force: gt_images a list of box lists, pred_images a list of (boxes, scores); every image
    is matched again at every distinct score of the set."""
    sorted_images = []
    for boxes, scores in pred_images:
        order = np.argsort(np.array(scores, np.float64)) if len(scores) else []
        sorted_images.append(([boxes[k] for k in order], [scores[k] for k in order]))
    distinct = sorted(set(s for _, scores in sorted_images for s in scores))
    precisions, recalls = [], []
    for s in distinct[:-1]:
        tp = fp = fn = 0
        for gt, (boxes, scores) in zip(gt_images, sorted_images):
            kept = [b for b, v in zip(boxes, scores) if v > s]
            m = image_matches(gt, kept, iou_thr) if kept and gt else 0
            tp, fp, fn = tp + m, fp + len(kept) - m, fn + len(gt) - m
        precisions.append(tp / (tp + fp) if tp + fp else 0.0)
        recalls.append(tp / (tp + fn) if tp + fn else 0.0)
    precisions, recalls = np.array(precisions, np.float64), np.array(recalls, np.float64)
    levels = [precisions[recalls >= level].max() if bool((recalls >= level).any()) else 0.0 for level in np.linspace(0.0, 1.0, 11)]
    return {"avg_prec": np.mean(levels), "precisions": precisions, "recalls": recalls, "model_thrs": distinct[:-1]}


def brute_result(gt_data, pred_data, iou_thresholds=IOU_THRESHOLDS, class_thresholds=CLASS_THRESHOLDS):
    """The whole result in metrics.py's layout from brute_curve."""
    classes = sorted(set(r[4] for img in gt_data for r in img) | set(r[4] for img in pred_data for r in img))

    def split(label):
        keep = lambda r: label is None or r[4] == label
        return ([[r[:4] for r in img if keep(r)] for img in gt_data],
                [([r[:4] for r in img if keep(r)], [r[5] for r in img if keep(r)]) for img in pred_data])

    def curve(label, th):
        out = brute_curve(*split(label), iou_thr=th)
        out["threshold"] = float(th)
        return out
    res = {"classes": classes, "thresholds": [float(t) for t in iou_thresholds], "class_thresholds": [float(t) for t in class_thresholds],
           "results": [curve(None, th) for th in iou_thresholds]}
    res["mAP"] = 100 * np.mean([float("{:.4f}".format(r["avg_prec"])) for r in res["results"]])
    res["per_class"] = {label: [curve(label, th) for th in class_thresholds] for label in classes}
    return res


def brute_tables(problems, thresholds):
    """The suffix tables of a metrics.SweepProblems table, every suffix matched on its own."""
    thr = [float(t) for t in thresholds]
    T = len(thr)
    tp = np.zeros(T * (problems.D + problems.N), np.int32)
    for p in range(problems.N):
        d0, d1, g0, g1 = (int(v) for v in (problems.det_off[p], problems.det_off[p + 1], problems.gt_off[p], problems.gt_off[p + 1]))
        P = d1 - d0
        det, gt = problems.det_box[d0:d1].tolist(), problems.gt_box[g0:g1].tolist()
        for t in range(T):
            for k in range(P):
                tp[T * (d0 + p) + t * (P + 1) + k] = image_matches(gt, det[k:], thr[t]) if gt else 0
    return tp
