"""Hand-built scenes for the tester (Analyzer.extract_gt_masks / compute_performances / get_data and ModelTester): the scenarios, a
driver that works on the reference's classes and on this package's alike (tests/golden/make_tester_fixtures.py records the
former into tests/golden/tester.npz), and the comparison of a run against that record.  Frames are 33 x 33 and 40 x 65."""
import contextlib
import io
import json
import os
import types

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tester.npz")

CLASS_NAMES = ['bkg', 'spurious', 'compact', 'extended', 'extended-multisland', 'flagged', 'galaxy']
META = {"telescope": "askap", "bkg": 1.25e-05, "rms": 0.0003, "bmaj": 12.0, "bmin": 9.0, "dx": -4.0, "dy": 4.0, "nx": 65, "ny": 40}
S33, S65 = (33, 33), (40, 65)


def rects(shape, *rs, dtype=bool):
    m = np.zeros(shape, dtype)
    for y1, y2, x1, x2 in rs:
        m[y1:y2, x1:x2] = 1
    return m


def _sc(name, shape, gt, dets, **kw):
    d = dict(name=name, shape=shape, gt=gt, dets=dets, iou_thr=0.6, consider=True, split=False, objs=False, int_dets=False)
    d.update(kw)
    return d


def scenarios():
    """gt: (rectangles, class id, sidelobe flag); dets: (rectangles, class id, score)."""
    A = [(4, 10, 5, 12)]
    return [
        # two identical detections on one true object: the later one wins, in both directions
        _sc("twin_dets", S33, [(A, 2, 0)], [(A, 2, 0.9), (A, 3, 0.8)]),
        _sc("twin_gts", S33, [(A, 2, 0), (A, 3, 0)], [(A, 2, 0.9)]),
        # IoU exactly at the threshold (6 of 10 pixels) and one pixel below it (5 of 10)
        _sc("thr_exact", S65, [([(2, 3, 0, 8)], 2, 0), ([(10, 11, 28, 36)], 2, 0)],
            [([(2, 3, 2, 10)], 2, 0.95), ([(10, 11, 31, 38)], 2, 0.85)]),
        _sc("class_mismatch", S33, [(A, 2, 0)], [(A, 1, 0.75)]),
        _sc("unmatched", S65, [(A, 2, 0), ([(20, 30, 40, 65)], 3, 0)], [(A, 2, 0.99), ([(32, 40, 0, 9)], 1, 0.71)]),
        _sc("no_dets", S33, [(A, 2, 0)], []),
        _sc("no_gts", S33, [], [(A, 2, 0.9)]),
        _sc("nothing", S33, [], []),
        # an empty mask, hence an invalid (all zero) box, on either side
        _sc("empty_gt", S33, [([], 2, 0), (A, 2, 0)], [(A, 2, 0.9)]),
        _sc("empty_det", S33, [(A, 2, 0)], [([], 2, 0.9), (A, 2, 0.8), ([], 3, 0.7)]),
        # iou_thr = 0: a detection that shares no pixel with the true object still matches it, with an IoU of 0
        _sc("thr_zero", S33, [(A, 2, 0)], [(A, 2, 0.9), ([(20, 25, 20, 25)], 3, 0.8)], iou_thr=0.0),
        # sources near or mixed with sidelobes left out of the true-object loop (not of the detection loop); no object info
        _sc("sidelobe_off", S65, [(A, 2, 0), ([(20, 30, 40, 65)], 3, 1), ([(34, 38, 2, 9)], 2, 0)],
            [(A, 2, 0.9), ([(20, 30, 40, 65)], 3, 0.8), ([(34, 38, 2, 8)], 2, 0.7)], consider=False),
        # merged-like integer detection masks
        _sc("int_dets", S65, [(A, 2, 0)], [([(4, 10, 5, 11)], 2, 0.9)], int_dets=True),
        # split_gtmasks: a compact source of two components (component 1 is taken twice), two touching pieces of one class, two
        # touching pieces of different classes, an `extended` and a `galaxy` mask of two components each left whole
        _sc("split_gt", S65, [([(2, 5, 2, 6), (2, 5, 30, 35)], 2, 0), ([(10, 14, 10, 20)], 1, 0), ([(14, 18, 12, 34)], 1, 1),
                              ([(18, 20, 30, 40)], 2, 0), ([(25, 28, 2, 6), (25, 28, 50, 60)], 3, 0),
                              ([(32, 36, 2, 6), (32, 36, 50, 65)], 6, 1)],
            [([(2, 5, 2, 6)], 2, 0.9), ([(10, 18, 10, 34)], 1, 0.8), ([(25, 28, 2, 6), (25, 28, 50, 60)], 3, 0.75)], split=True),
        # with object info and planted detection parameters: the rows of the two tables
        _sc("table_a", S65, [(A, 2, 0), ([(20, 30, 40, 65)], 3, 0), ([(34, 38, 2, 9)], 5, 1)],
            [(A, 2, 0.97), ([(20, 30, 40, 64)], 1, 0.88), ([(0, 3, 60, 65)], 2, 0.72)], objs=True),
        _sc("table_b", S33, [(A, 3, 0)], [(A, 3, 0.91), (A, 3, 0.74)], objs=True),
        # the sidelobe switch off WITH object info: the reference's single counter runs over lists of different lengths
        _sc("table_off", S65, [(A, 2, 1), ([(20, 30, 40, 65)], 3, 0), ([(34, 38, 2, 9)], 2, 0)],
            [([(20, 30, 40, 65)], 3, 0.9)], objs=True, consider=False),
    ]


TESTER_RUNS = {"tables": ["table_a", "table_b", "no_dets"], "tables_off": ["table_off", "table_b"]}


def scenario(name):
    return [s for s in scenarios() if s["name"] == name][0]


def cfg():
    return types.SimpleNamespace(NUM_CLASSES=len(CLASS_NAMES), CLASS_NAMES=list(CLASS_NAMES))


class StubDataset(object):
    """What Analyzer.get_data and ModelTester ask of a dataset, for one hand-built image."""

    def __init__(self, consider=True):
        self.nclasses = len(CLASS_NAMES)
        self.class_names = list(CLASS_NAMES)
        self.consider_sources_near_mixed_sidelobes = consider
        self.image_info = []
        self.image_ids = []
        self.images, self.gt_masks = [], []

    def add(self, image, masks, class_ids, flags, objs=None, metadata=None, path="img.fits"):
        info = {"id": "uuid-%d" % len(self.image_info), "path": path, "class_ids": list(class_ids), "sidelobes_mixed_or_near": list(flags)}
        if objs is not None:
            info["objs"] = objs
        if metadata is not None:
            info["metadata"] = metadata
        self.image_info.append(info)
        self.image_ids = list(range(len(self.image_info)))
        self.images.append(image)
        self.gt_masks.append(masks)

    def load_image(self, image_id):
        return self.images[image_id]

    def image_uuid(self, image_id):
        return self.image_info[image_id]["id"]

    def image_metadata(self, image_id):
        return self.image_info[image_id].get("metadata", {})

    def load_gt_masks(self, image_id, binary=True):
        m = self.gt_masks[image_id]
        return m.astype(bool) if binary else m.astype(int)

    def load_gt_obj_info(self, image_id):
        return self.image_info[image_id].get("objs", [])


class StubModel(object):
    def __init__(self, result):
        self.result = result

    def detect(self, images, verbose=0):
        return [self.result]


def gt_objs(sc):
    """Object info as a JSON file holds it, one dict per true object."""
    return [{"name": "S%d" % (k + 1), "class": CLASS_NAMES[c], "sidelobe-mixed": int(f), "nislands": 1 + k % 2, "border": int(k == 1),
             "snr": 12.5 + 3 * k, "maxsize_beam": 2.5 + k, "minsize_beam": 1.25 + 0.5 * k} for k, (_, c, f) in enumerate(sc["gt"])]


def det_pars(sc):
    """What compute_det_mask_pars would leave: planted, so that the fixture pins the tables and not OpenCV / skimage.  The second
    detection's smaller side is 0 (a straight run of pixels): aspectRatio -999."""
    return [{"name": "Sdet%d" % (k + 1), "class": CLASS_NAMES[c], "border": int(k == 2), "snr": 30.0 / (k + 1), "npix": 10 + k,
             "maxsize_beam": 1.5 + k, "minsize_beam": 0.0 if k == 1 else 0.75 + 0.25 * k, "nislands": 1, "Stot": 0.5 * (k + 1)}
            for k, (_, c, _) in enumerate(sc["dets"])]


def drive(an, sc, extract_bboxes):
    """Sets the hand-built scene on an Analyzer (the reference's or this package's) and runs extract_gt_masks and
    compute_performances on it; what the steps in between would have left is set directly."""
    shape = sc["shape"]
    an.image_path = "img_%s.fits" % sc["name"]
    an.image_metadata = dict(META)
    an.dataset.consider_sources_near_mixed_sidelobes = sc["consider"]
    an.class_names = an.class_names_gt = list(CLASS_NAMES)
    gt = [rects(shape, *r, dtype=int) for r, _, _ in sc["gt"]]
    an.masks_gt = np.stack(gt, axis=-1) if gt else np.zeros(shape + (0,), int)
    an.class_ids_gt = [c for _, c, _ in sc["gt"]]
    an.labels_gt = [CLASS_NAMES[c] for c in an.class_ids_gt]
    an.sidelobes_mixed_or_near_gt = [f for _, _, f in sc["gt"]]
    an.split_gtmasks = sc["split"]
    an.extract_gt_masks()
    an.masks_final = [rects(shape, *r, dtype=int if sc["int_dets"] else bool) for r, _, _ in sc["dets"]]
    an.class_ids_final = [c for _, c, _ in sc["dets"]]
    an.class_names_final = [CLASS_NAMES[c] for c in an.class_ids_final]
    an.scores_final = [np.float32(s) for _, _, s in sc["dets"]]
    an.bboxes = [extract_bboxes(m.astype(bool)[:, :, None])[0] for m in an.masks_final]
    an.objs_gt = gt_objs(sc) if sc["objs"] else []
    an.iou_thr = sc["iou_thr"]
    an.compute_performances()
    an.det_obj_pars = det_pars(sc)
    return an


LISTS = (("class_ids_gt_merged", np.int64), ("sidelobes_mixed_or_near_gt_merged", np.int64), ("detobj_scores", np.float64),
         ("detobj_ious", np.float64), ("detobj_classids", np.int64), ("is_gt_obj_detected", np.int64),
         ("is_det_obj_matching_to_gt_obj", np.int64), ("is_det_obj_matching_to_gt_obj_sameclass", np.int64),
         ("matchobj_classids", np.int64), ("matchobj_ious", np.float64))
NAME_LISTS = ("captions_gt", "detobj_class_names", "matchobj_class_names")
ARRAYS = ("confusion_matrix", "confusion_matrix_norm", "purity", "nobjs_true", "nobjs_det", "nobjs_det_right")


def analyzer_record(an, shape):
    """Every list and array the two steps leave, as arrays."""
    out = {}
    for key, dtype in LISTS:
        out[key] = np.array(getattr(an, key), dtype=dtype).reshape(-1)
    for key in NAME_LISTS:
        out[key] = np.array([str(v) for v in getattr(an, key)], dtype="U32")
    for key in ARRAYS:
        out[key] = np.array(getattr(an, key), dtype=np.float64)
    out["bboxes_gt"] = np.array(an.bboxes_gt, dtype=np.int64).reshape(-1, 4)
    masks = [np.asarray(m) for m in an.masks_gt_merged]
    out["masks_gt_merged"] = np.stack(masks).astype(np.uint8) if masks else np.zeros((0,) + shape, np.uint8)
    out["detobj_gtinfo_names"] = np.array([o["name"] for o in an.detobj_gtinfo], dtype="U32")
    return out


def run_tester(tester, make_analyzer, names, extract_bboxes, tmpdir):
    """update_performances on the driven scenarios `names`, then compute_performances and save: the record."""
    tester.outfilename_completeness = os.path.join(tmpdir, "completeness.csv")
    tester.outfilename_reliability = os.path.join(tmpdir, "reliability.csv")
    tester.score_thr, tester.iou_thr = 0.7, 0.6
    quiet = io.StringIO()
    for name in names:
        sc = scenario(name)
        with contextlib.redirect_stdout(quiet):
            an = drive(make_analyzer(sc), sc, extract_bboxes)
            tester.update_performances(an)
    printed = io.StringIO()
    with contextlib.redirect_stdout(printed):
        tester.compute_performances()
    with contextlib.redirect_stdout(quiet):
        tester.save()
    out = {"printed": np.frombuffer(printed.getvalue().encode(), np.uint8)}
    for key, fn in (("completeness_csv", tester.outfilename_completeness), ("reliability_csv", tester.outfilename_reliability)):
        out[key] = np.frombuffer(open(fn, "rb").read() if os.path.exists(fn) else b"", np.uint8)
    for key in ("classification_matrix", "classification_matrix_norm", "purity", "nobjs_true", "nobjs_det", "nobjs_det_right"):
        out[key] = np.array(getattr(tester, key), dtype=np.float64)
    out["detobj_scores"] = np.array(tester.detobj_scores, dtype=np.float64)
    out["detobj_ious"] = np.array(tester.detobj_ious, dtype=np.float64)
    out["stats"] = np.array([tester.detobj_scoreMean, tester.detobj_scoreStdDev, tester.detobj_iouMean, tester.detobj_iouStdDev], np.float64)
    return out


# ---- get_data: class-id remapping (analyze.py:760-776) -----------------------------------------------------------
REMAP_CASES = {"remap": {1: 2, 2: 1, 3: 3}, "remap_missing": {1: 2, 2: 1}, "remap_off": None, "remap_empty": {}}


def get_data_scene():
    shape = S33
    image = np.zeros(shape + (3,), np.uint8)
    gt = np.stack([rects(shape, (4, 10, 5, 12), dtype=int), rects(shape, (20, 25, 20, 30), dtype=int)], axis=-1)
    det = np.stack([rects(shape, (4, 10, 5, 12)), rects(shape, (20, 25, 20, 30)), rects(shape, (0, 2, 0, 2))], axis=-1)
    result = {"masks": det, "rois": np.array([[4, 5, 10, 12], [20, 20, 25, 30], [0, 0, 2, 2]], np.int32),
              "class_ids": np.array([1, 2, 3], np.int32), "scores": np.array([0.9, 0.8, 0.75], np.float32)}
    ds = StubDataset()
    ds.add(image, gt, [2, 3], [0, 1], objs=[{"name": "S1"}, {"name": "S2"}], metadata=dict(META), path="img_remap.fits")
    return ds, StubModel(result)


def run_get_data(an, case):
    an.image_id = 0
    an.image_path = "img_remap.fits"
    classid_map = REMAP_CASES[case]
    an.remap_classids = classid_map is not None
    an.classid_map = classid_map or {}
    status = an.get_data()
    out = {"status": np.array(status), "class_ids": np.array([int(c) for c in an.class_ids], np.int64)}
    if status == 0:
        out["labels_gt"] = np.array(an.labels_gt, dtype="U32")
        out["captions_gt"] = np.array(an.captions_gt, dtype="U32")
        out["class_ids_gt"] = np.array(an.class_ids_gt, np.int64)
        out["sidelobes"] = np.array(an.sidelobes_mixed_or_near_gt, np.int64)
        out["nobjects"] = np.array(an.nobjects)
        out["masks_gt_dtype_kind"] = np.array(an.masks_gt.dtype.kind)
        out["n_objs_gt"] = np.array(len(an.objs_gt))
    return out


def flatten(prefix, rec, out):
    """A record as three kinds of entries: `head` (JSON: per key its kind and shape, the strings themselves), `nums` (every
    numeric array, flattened, as float64 -- the integers here are small, so nothing is rounded) and the byte arrays as they are."""
    head, nums = {}, []
    for k in sorted(rec):
        v = np.asarray(rec[k])
        if v.dtype.kind in "US":
            head[k] = {"kind": "U", "shape": list(v.shape), "values": [str(x) for x in v.ravel().tolist()]}
        elif v.dtype == np.uint8:
            head[k] = {"kind": "bytes"}
            out["%s/%s" % (prefix, k)] = v
        else:
            head[k] = {"kind": v.dtype.kind, "shape": list(v.shape)}
            nums.append(v.astype(np.float64).ravel())
    out[prefix + "/head"] = np.array(json.dumps(head, sort_keys=True))
    out[prefix + "/nums"] = np.concatenate(nums) if nums else np.zeros(0)


def unflatten(golden, prefix):
    head, nums, at, rec = json.loads(str(golden[prefix + "/head"])), golden[prefix + "/nums"], 0, {}
    for k in sorted(head):
        h = head[k]
        if h["kind"] == "U":
            rec[k] = np.array(h["values"], dtype="U32").reshape(h["shape"])
        elif h["kind"] == "bytes":
            rec[k] = golden["%s/%s" % (prefix, k)]
        else:
            n = int(np.prod(h["shape"], dtype=np.int64))
            rec[k] = nums[at:at + n].astype({"i": np.int64, "f": np.float64}[h["kind"]]).reshape(h["shape"])
            at += n
    assert at == nums.size
    return rec


def assert_record(got, golden, prefix):
    """Every array of `got` equals the fixture's, value for value (== on every element; same shape and kind)."""
    rec = unflatten(golden, prefix)
    assert sorted(rec) == sorted(got), (prefix, sorted(rec), sorted(got))
    for k in sorted(rec):
        want, have = rec[k], np.asarray(got[k])
        assert want.shape == have.shape and want.dtype.kind == have.dtype.kind, (prefix, k, want.shape, have.shape, want.dtype, have.dtype)
        assert bool(np.all(want == have)), "%s/%s:\nwant %r\ngot  %r" % (prefix, k, want, have)
