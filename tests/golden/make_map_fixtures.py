#!/usr/bin/env python3
"""Generates tests/golden/map.npz by running the REFERENCE's own code and recording inputs and outputs only -- no reference
source text:

  * ``Evaluator.GetPascalVOCMetrics`` of the vendored Object-Detection-Metrics tool (every-point interpolation, with the mAP rule
    of its pascalvoc.py restated around it: the script itself parses the command line and plots on import) on the 11 + 11 sample
    files the tool ships, read as ``xyrb`` and as ``xywh``, and on the hand-built cases of tests/map_cases.py, at thresholds 0.5
    and 0.6.  The flags and running sums are not part of the tool's answer: they are caught where the tool hands them to
    ``numpy.cumsum`` (FP first, then TP).
  * ``ModelTester.compute_mAP`` (mrcnn/analyze.py) with ``model.detect``, ``modellib.load_image_gt`` and ``modellib.mold_image``
    replaced by the stand-ins of tests/map_cases.py: its ``mAP`` and the bytes of every file it writes.
  * ``utils.compute_ap_range`` (mrcnn/utils.py) on the scenes of tests/tester_cases.py.

Runs only where the reference is present; the .npz is committed and pins caesar-mrcnn_amd/metrics.py, utils.compute_ap_range and
ModelTester.compute_mAP (tests/test_map_cpu.py, tests/test_map_gpu.py).  ``cv2`` is a stand-in: the tool only draws with it."""
import contextlib
import glob
import io
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_reference_fixtures as base            # noqa: E402
import make_sfinder_fixtures as sbase             # noqa: E402
import map_cases as cases                         # noqa: E402
import tester_cases as tcases                     # noqa: E402

TOOL = os.path.join(base.REF, "Object-Detection-Metrics")


class _NumpySpy(object):
    """numpy, with the arguments of cumsum kept."""

    def __init__(self):
        self.seen = []

    def __getattr__(self, name):
        return getattr(np, name)

    def cumsum(self, a, *args, **kw):
        self.seen.append(np.array(a, np.float64))
        return np.cumsum(a, *args, **kw)


def tool_record(tool, gt_data, pred_data, thresholds):
    """The tool's answer on the rows, in the layout of map_cases.record: every image's ground truths first, then every image's
    detections, as getBoundingBoxes reads its two folders."""
    boxes = tool["BoundingBoxes"]()
    for i, rows in enumerate(gt_data):
        for r in rows:
            boxes.addBoundingBox(tool["BoundingBox"](str(i), r[4], r[0], r[1], r[2], r[3], tool["CoordinatesType"].Absolute, None,
                                                     tool["BBType"].GroundTruth, format=tool["BBFormat"].XYX2Y2))
    for i, rows in enumerate(pred_data):
        for r in rows:
            boxes.addBoundingBox(tool["BoundingBox"](str(i), r[4], r[0], r[1], r[2], r[3], tool["CoordinatesType"].Absolute, None,
                                                     tool["BBType"].Detected, r[5], format=tool["BBFormat"].XYX2Y2))
    rec, classes = {}, None
    for k, thr in enumerate(thresholds):
        spy = tool["module"].np = _NumpySpy()
        with np.errstate(divide="ignore", invalid="ignore"):
            res = tool["Evaluator"]().GetPascalVOCMetrics(boxes, IOUThreshold=thr, method=tool["Method"].EveryPointInterpolation)
        tool["module"].np = np
        assert len(spy.seen) == 2 * len(res)
        classes = [r["class"] for r in res]
        acc_ap, valid = 0, 0
        for n, r in enumerate(res):
            FP, TP = spy.seen[2 * n], spy.seen[2 * n + 1]
            vals = {"precision": r["precision"], "recall": r["recall"], "AP": r["AP"], "total positives": r["total positives"],
                    "total TP": r["total TP"], "total FP": r["total FP"], "TP": TP, "FP": FP, "acc TP": np.cumsum(TP), "acc FP": np.cumsum(FP)}
            for f in cases.FIELDS:
                rec["t%d/%s/%s" % (k, r["class"], f)] = np.asarray(vals[f], np.float64).reshape(-1)
            if r["total positives"] > 0:
                valid += 1
                acc_ap = acc_ap + r["AP"]
        rec["t%d/mAP" % k] = np.array([acc_ap / valid if valid else np.nan], np.float64)
    return classes, rec


def sample_rows(tool, fmt):
    """The tool's sample files as rows of corners, through the tool's own BoundingBox (``xywh``: right = left + width)."""
    names = sorted(set(os.path.basename(f)[:-4] for sub in ("groundtruths", "detections") for f in glob.glob(os.path.join(TOOL, sub, "*.txt"))))
    bbformat = {"xyrb": tool["BBFormat"].XYX2Y2, "xywh": tool["BBFormat"].XYWH}[fmt]
    gt_data, pred_data = [], []
    for name in names:
        for sub, rows_of in (("groundtruths", gt_data), ("detections", pred_data)):
            rows, path = [], os.path.join(TOOL, sub, name + ".txt")
            for line in (open(path).read().splitlines() if os.path.exists(path) else []):
                if line.replace(" ", "") == "":
                    continue
                p = line.split(" ")
                nums = [float(v) for v in p[1:]]
                is_gt = sub == "groundtruths"
                bb = tool["BoundingBox"](name, p[0], *nums[(0 if is_gt else 1):], tool["CoordinatesType"].Absolute, None,
                                         tool["BBType"].GroundTruth if is_gt else tool["BBType"].Detected, None if is_gt else nums[0],
                                         format=bbformat)
                corners = [float(v) for v in bb.getAbsoluteBoundingBox(tool["BBFormat"].XYX2Y2)]
                rows.append(corners + [p[0]] + ([] if is_gt else [nums[0]]))
            rows_of.append(rows)
    return gt_data, pred_data


def main():
    sbase.install_stubs()
    sys.path.insert(0, base.REF)
    sys.path.insert(0, os.path.join(TOOL, "lib"))
    import Evaluator as ev_module
    import BoundingBox as bb_module
    import BoundingBoxes as bbs_module
    import utils as tool_utils
    del sys.path[0]
    del sys.modules["utils"]
    tool = {"module": ev_module, "Evaluator": ev_module.Evaluator, "BoundingBox": bb_module.BoundingBox,
            "BoundingBoxes": bbs_module.BoundingBoxes, "BBFormat": tool_utils.BBFormat, "BBType": tool_utils.BBType,
            "CoordinatesType": tool_utils.CoordinatesType, "Method": tool_utils.MethodAveragePrecision}
    out = {}
    for fmt in cases.SAMPLE_FORMATS:
        gt_data, pred_data = sample_rows(tool, fmt)
        classes, rec = tool_record(tool, gt_data, pred_data, cases.THRESHOLDS)
        cases.store("sample_" + fmt, gt_data, pred_data, classes, cases.THRESHOLDS, rec, out)
        print("sample %s: %d images, %d objects, %d detections; at 0.5: %s" % (
            fmt, len(gt_data), sum(map(len, gt_data)), sum(map(len, pred_data)),
            ", ".join("%s AP %.4f (%d, %d, %d)" % (c, rec["t0/%s/AP" % c][0], rec["t0/%s/total positives" % c][0], rec["t0/%s/total TP" % c][0],
                                                   rec["t0/%s/total FP" % c][0]) for c in classes)))
    for name, (gt_data, pred_data) in sorted(cases.hand_cases().items()):
        classes, rec = tool_record(tool, gt_data, pred_data, cases.THRESHOLDS)
        cases.store("hand_" + name, gt_data, pred_data, classes, cases.THRESHOLDS, rec, out)
        print("hand %-15s classes %s: AP@0.5 %s, mAP %s" % (name, classes, [float(rec["t0/%s/AP" % c][0]) for c in classes],
                                                            [float(rec["t%d/mAP" % k][0]) for k in range(len(cases.THRESHOLDS))]))

    # compute_ap_range and compute_mAP of the reference
    from mrcnn import analyze as ref
    U = ref.utils
    names, values = [], []
    for sc in cases.ap_scenes():
        with np.errstate(divide="ignore", invalid="ignore"):
            values.append(U.compute_ap_range(*cases.ap_inputs(sc, U.extract_bboxes), verbose=0))
        names.append(sc["name"])
    out["ap_range/names"] = np.array(names, dtype="U32")
    out["ap_range/values"] = np.array(values, np.float64)
    print("compute_ap_range:", dict(zip(names, ["%.4f" % v for v in values])))

    ref.modellib.load_image_gt = cases.map_image_gt(U.extract_bboxes)
    ref.modellib.mold_image = lambda image, config: image
    tester = ref.ModelTester(cases.MapModel(U.extract_bboxes), tcases.cfg(), cases.MapDataset())
    tester.iou_thr = 0.6
    printed = io.StringIO()
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        try:
            with contextlib.redirect_stdout(printed):
                tester.compute_mAP(gt_data=cases.MAP_GT, pred_data=cases.MAP_PRED)
        finally:
            os.chdir(cwd)
        files = cases.tree_bytes(tmp)
    out["compute_map/mAP"] = np.array([tester.mAP], np.float64)
    out["compute_map/printed"] = np.frombuffer(printed.getvalue().encode(), np.uint8)
    out["compute_map/files"] = np.array(sorted(files), dtype="U128")
    for k, name in enumerate(sorted(files)):
        out["compute_map/file%d" % k] = np.frombuffer(files[name], np.uint8)
    print("compute_mAP: mAP %.6f, %d files, %d bytes" % (tester.mAP, len(files), sum(len(v) for v in files.values())))
    np.savez_compressed(cases.GOLDEN, **out)
    print("wrote %s (%d bytes)" % (cases.GOLDEN, os.path.getsize(cases.GOLDEN)))


if __name__ == "__main__":
    main()
