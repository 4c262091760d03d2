"""Hand-built test sets for the Pascal-VOC box metrics and the mask AP (caesar-mrcnn_amd/metrics.py, ModelTester.compute_mAP): the
cases, the flat record a result is compared through, and the stand-ins that drive ``compute_mAP`` of the reference and of this
package alike.  tests/golden/make_map_fixtures.py records the reference's side into tests/golden/map.npz.

Rows are ``[c0, c1, c2, c3, label]`` / ``[c0, c1, c2, c3, label, score]`` with inclusive corners, as the tool counts them: a box
(0, 0, 9, 9) holds 10 x 10 pixels."""
import json
import os

import numpy as np

import tester_cases as tcases

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "map.npz")
THRESHOLDS = (0.5, 0.6)
SAMPLE_FORMATS = ("xyrb", "xywh")
FIELDS = ("precision", "recall", "AP", "total positives", "total TP", "total FP", "TP", "FP", "acc TP", "acc FP")

B10 = [0, 0, 9, 9]                       # 10 x 10
B10x5 = [0, 0, 9, 4]                     # 10 x 5 inside it: IoU 50 / 100 = 0.5 exactly
B10x6 = [0, 0, 9, 5]                     # 10 x 6 inside it: IoU 60 / 100 = 0.6 exactly
FAR = [40, 40, 49, 49]


def _shift(box, d):
    return [box[0] + d, box[1] + d, box[2] + d, box[3] + d]


def hand_cases():
    """name -> (gt_data, pred_data)."""
    g, s = "galaxy", "source"
    cases = {
        # an image without ground truth next to one with: the lone detections are false positives
        "no_gt_image": ([[], [B10 + [g]]], [[B10 + [g, 0.9]], [B10 + [g, 0.8]]]),
        # an image without detections
        "no_det_image": ([[B10 + [g]], [B10 + [g]]], [[], [B10 + [g, 0.7]]]),
        # two detections on one ground truth: the higher score takes it, whichever row comes first
        "twin_scores": ([[B10 + [g]]], [[B10x6 + [g, 0.6], B10 + [g, 0.9]]]),
        # ... at equal scores the earlier row does
        "twin_equal": ([[B10 + [g]]], [[B10x6 + [g, 0.8], B10 + [g, 0.8]]]),
        # equal scores across images: the class order is the row order (stable sort), seen in precision / recall
        "equal_across": ([[B10 + [g]], [B10 + [g]], [B10 + [g]]],
                         [[FAR + [g, 0.5]], [B10 + [g, 0.5]], [FAR + [g, 0.5], B10 + [g, 0.5]]]),
        # two ground truths at equal IoU: the first one is chosen by both detections, the second one stays unmatched
        "twin_gts": ([[B10 + [g], B10 + [g]]], [[B10 + [g, 0.9], B10 + [g, 0.8]]]),
        # IoU exactly 0.5 and exactly 0.6: `>=` at both thresholds
        "iou_exact": ([[B10 + [g]], [B10 + [g]]], [[B10x5 + [g, 0.9]], [B10x6 + [g, 0.8]]]),
        # boxes that share one corner pixel only: not disjoint, IoU 1 / 148
        "edge_pixel": ([[B10 + [g]]], [[[9, 9, 15, 15] + [g, 0.9]]]),
        # ... and boxes one pixel apart: disjoint, IoU 0, no ground truth at all
        "apart": ([[B10 + [g]]], [[[10, 0, 15, 9] + [g, 0.9]]]),
        # a class only among the detections (AP NaN, left out of mAP) and a class only among the ground truths (AP 0, counted)
        "det_only_class": ([[B10 + [g]]], [[B10 + [g, 0.9], FAR + [s, 0.8]]]),
        "gt_only_class": ([[B10 + [g], FAR + [s]]], [[B10 + [g, 0.9]]]),
        # the detection's best box is of another class: it does not count
        "other_class": ([[B10 + [s], B10x6 + [g]]], [[B10 + [g, 0.9]]]),
    }
    # three classes with hits and misses each: the running sums start again with every class
    t = "triple"
    cases["three_classes"] = (
        [[B10 + [g], FAR + [s], _shift(B10, 20) + [t]], [B10 + [g], B10 + [s], B10 + [t], FAR + [t]]],
        [[B10 + [g, 0.9], FAR + [g, 0.8], FAR + [s, 0.7], B10 + [s, 0.6], _shift(B10x6, 20) + [t, 0.5], B10 + [t, 0.45]],
         [B10x5 + [g, 0.85], B10 + [s, 0.3], B10 + [s, 0.2], FAR + [t, 0.9], B10 + [t, 0.1], B10x6 + [t, 0.05]]])
    # all of them as one test set, every image shifted so that nothing else changes
    gt_all, pred_all = [], []
    for k, name in enumerate(sorted(cases)):
        gt, pred = cases[name]
        for gi, pi in zip(gt, pred):
            gt_all.append([_shift(r[:4], k) + r[4:] for r in gi])
            pred_all.append([_shift(r[:4], k) + r[4:] for r in pi])
    cases["all"] = (gt_all, pred_all)
    return cases


# ---- the flat record of a result ------------------------------------------------------------------------------------
def record(result):
    """A metrics result (metrics.py's layout) as {key: float64 array}."""
    out = {}
    for k, res in enumerate(result["results"]):
        out["t%d/mAP" % k] = np.array([res["mAP"]], np.float64)
        for label in result["classes"]:
            for f in FIELDS:
                out["t%d/%s/%s" % (k, label, f)] = np.asarray(res["classes"][label][f], np.float64).reshape(-1)
    return out


def store(prefix, gt_data, pred_data, classes, thresholds, rec, out):
    out[prefix + "/input"] = np.array(json.dumps({"gt": gt_data, "pred": pred_data, "classes": classes, "thresholds": list(thresholds)}))
    keys = sorted(rec)
    out[prefix + "/keys"] = np.array(json.dumps(keys))
    out[prefix + "/sizes"] = np.array([rec[k].size for k in keys], np.int64)
    out[prefix + "/nums"] = np.concatenate([rec[k] for k in keys]) if keys else np.zeros(0)


def load(golden, prefix):
    """(gt_data, pred_data, classes, thresholds, record) of a stored case."""
    head = json.loads(str(golden[prefix + "/input"]))
    keys, sizes, nums = json.loads(str(golden[prefix + "/keys"])), golden[prefix + "/sizes"], golden[prefix + "/nums"]
    rec, at = {}, 0
    for k, n in zip(keys, sizes):
        rec[k] = nums[at:at + int(n)]
        at += int(n)
    assert at == nums.size
    return head["gt"], head["pred"], head["classes"], head["thresholds"], rec


def assert_record(got, want, what):
    """`==` on every float64, NaN where the tool gives NaN."""
    assert sorted(got) == sorted(want), (what, sorted(set(got) ^ set(want)))
    for k in sorted(want):
        a, b = np.asarray(got[k], np.float64), np.asarray(want[k], np.float64)
        assert a.shape == b.shape, (what, k, a.shape, b.shape)
        assert bool(np.all((a == b) | (np.isnan(a) & np.isnan(b)))), "%s %s:\nwant %r\ngot  %r" % (what, k, b, a)


def golden_cases(golden):
    return sorted(set(k.split("/")[0] for k in golden.files if k.startswith(("hand_", "sample_"))))


# ---- compute_ap_range on the tester's scenes -------------------------------------------------------------------------
def ap_inputs(sc, extract_bboxes):
    """The seven arrays utils.compute_ap takes, from a scene of tests/tester_cases.py."""
    shape = sc["shape"]
    gt = [tcases.rects(shape, *r) for r, _, _ in sc["gt"]]
    det = [tcases.rects(shape, *r) for r, _, _ in sc["dets"]]
    gt_mask = np.stack(gt, axis=-1) if gt else np.zeros(shape + (0,), bool)
    pred_mask = np.stack(det, axis=-1) if det else np.zeros(shape + (0,), bool)
    return (extract_bboxes(gt_mask), np.array([c for _, c, _ in sc["gt"]], np.int32), gt_mask,
            extract_bboxes(pred_mask), np.array([c for _, c, _ in sc["dets"]], np.int32),
            np.array([s for _, _, s in sc["dets"]], np.float32), pred_mask)


def ap_scenes():
    """The scenes with at least one true object (without one the reference divides 0 by 0 and warns)."""
    return [sc for sc in tcases.scenarios() if any(r for r, _, _ in sc["gt"])]


# ---- compute_mAP with stand-ins ---------------------------------------------------------------------------------------
MAP_IMAGES = ("unmatched", "thr_exact")            # scenes of tester_cases.py, one per image
MAP_PATHS = ("data/set1/img_unmatched.fits", "img_thr_exact.fits")
MAP_GT = [[[4, 5, 10, 12, "compact"], [20, 40, 30, 65, "extended"]], [[2, 0, 3, 8, "compact"], [10, 28, 11, 36, "compact"]]]
MAP_PRED = [[[4, 5, 10, 12, "compact", 0.99], [32, 0, 40, 9, "spurious", 0.7099999785423279]],
            [[2, 2, 3, 10, "compact", 0.949999988079071], [10, 31, 11, 38, "compact", 0.8500000238418579]]]


class MapDataset(tcases.StubDataset):
    def __init__(self):
        tcases.StubDataset.__init__(self)
        for path in MAP_PATHS:
            self.add(None, None, [], [], path=path)


def map_image_gt(extract_bboxes):
    """Stand-in for load_image_gt: (dataset, config, image_id, use_mini_mask=False) -> image, meta, class ids, boxes, masks."""
    def load_image_gt(dataset, config, image_id, augment=False, augmentation=None, use_mini_mask=False):
        assert use_mini_mask is False
        sc = tcases.scenario(MAP_IMAGES[image_id])
        gt_box, gt_cls, gt_mask = ap_inputs(sc, extract_bboxes)[:3]
        return np.full(sc["shape"] + (3,), image_id, np.uint8), np.zeros(12 + len(tcases.CLASS_NAMES)), gt_cls, gt_box, gt_mask
    return load_image_gt


class MapModel(object):
    """detect() answers with the scene whose index the stand-in image carries."""

    def __init__(self, extract_bboxes):
        self.extract_bboxes, self.calls = extract_bboxes, 0

    def detect(self, images, verbose=0):
        self.calls += 1
        sc = tcases.scenario(MAP_IMAGES[int(images[0][0, 0, 0])])
        _, _, _, box, cls, score, mask = ap_inputs(sc, self.extract_bboxes)
        return [{"rois": box, "class_ids": cls, "scores": score, "masks": mask}]


def tree_bytes(root):
    """{relative path: bytes} of every file under root."""
    out = {}
    for base, _, files in os.walk(root):
        for f in files:
            p = os.path.join(base, f)
            out[os.path.relpath(p, root).replace(os.sep, "/")] = open(p, "rb").read()
    return out
