#!/usr/bin/env python3
"""Generates tests/golden/sweep.npz by running the REFERENCE's own code and recording inputs and outputs only -- no reference
source text: the vendored tarlen5-calculate-mean-ap/calculate.py on the sets of tests/sweep_cases.py, read from the two JSON files
``metrics.write_metric_files`` writes for them.

  * ``get_avg_precision_at_iou`` class-blind at the ten IoU thresholds 0.50 ... 0.95 (``avg_prec``, ``precisions``, ``recalls``,
    ``model_thrs``), on a fresh copy of the files' content each time;
  * the same after ``split_boxes_by_class`` for every label the set holds, at 0.5 and 0.6;
  * for the sets of ``sweep_cases.MAIN_SETS`` the lines the tool's ``__main__`` prints, run as a script in a directory that holds
    the two files, without its two timing lines and the empty lines;
  * that the tool raises on the malformed box of ``sweep_cases.MALFORMED``.

The tool imports matplotlib, pandas and seaborn and opens plot windows: inert stand-ins take their place.  Sets marked ``tied``
hold bit-equal IoUs within an image; there the tool's order of equal IoUs is NumPy's unstable sort's: the record is this machine's.
Every other set is checked to hold none.  Runs only where the reference is present; the .npz is committed and pins
``metrics.sweep_metrics_host`` (tests/test_sweep_cpu.py, tests/test_sweep_gpu.py)."""
import contextlib
import copy
import importlib.util
import io
import json
import os
import runpy
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import make_reference_fixtures as base            # noqa: E402
import sweep_cases as cases                       # noqa: E402

TOOL = os.path.join(base.REF, "tarlen5-calculate-mean-ap", "calculate.py")


def tool_inputs(metrics, gt_data, pred_data):
    """The content of the tool's two input files as write_metric_files writes them."""
    with tempfile.TemporaryDirectory() as tmp:
        metrics.write_metric_files(gt_data, pred_data, ["%d.fits" % i for i in range(len(gt_data))], tmp)
        folder = os.path.join(tmp, "tarlen5-calculate-mean-ap")
        return (json.load(open(os.path.join(folder, "ground_truth_boxes.json"))), json.load(open(os.path.join(folder, "predicted_boxes.json"))),
                open(os.path.join(folder, "ground_truth_boxes.json")).read(), open(os.path.join(folder, "predicted_boxes.json")).read())


def tool_record(tool, gt_boxes, pred_boxes, classes):
    rec = {}

    def put(prefix, data):
        for f in cases.FIELDS:
            rec[prefix + f] = np.asarray(data[f], np.float64).reshape(-1)
    avg = []
    for k, thr in enumerate(np.linspace(0.5, 0.95, 10)):
        data = tool.get_avg_precision_at_iou(copy.deepcopy(gt_boxes), copy.deepcopy(pred_boxes), iou_thr=thr)
        put("t%d/" % k, data)
        avg.append(float("{:.4f}".format(data["avg_prec"])))
    rec["mAP"] = np.array([100 * np.mean(avg)], np.float64)
    for label in classes:
        for k, thr in enumerate(np.linspace(0.5, 0.6, 2)):
            gt_c, pred_c = tool.split_boxes_by_class(copy.deepcopy(gt_boxes), copy.deepcopy(pred_boxes), label)
            put("%s/t%d/" % (label, k), tool.get_avg_precision_at_iou(gt_c, pred_c, iou_thr=thr))
    return rec


def tool_main_lines(gt_text, pred_text):
    printed = io.StringIO()
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        for name, text in (("ground_truth_boxes.json", gt_text), ("predicted_boxes.json", pred_text)):
            with open(os.path.join(tmp, name), "w") as fp:
                fp.write(text)
        os.chdir(tmp)
        try:
            with contextlib.redirect_stdout(printed):
                runpy.run_path(TOOL, run_name="__main__")
        finally:
            os.chdir(cwd)
    return [l for l in printed.getvalue().splitlines() if l.strip() and " secs" not in l]


def main():
    for name in ("matplotlib", "matplotlib.pyplot", "pandas", "seaborn"):
        base._stub(name)
    spec = importlib.util.spec_from_file_location("_sweep_tool", TOOL)
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    from caesar_mrcnn_amd import metrics
    out = {}
    for name, (gt_data, pred_data, tied) in sorted(cases.sets().items()):
        assert cases.has_tied_ious(gt_data, pred_data, metrics.sweep_iou_matrix) == tied, "%s: tied IoUs %s" % (name, not tied)
        gt_boxes, pred_boxes, gt_text, pred_text = tool_inputs(metrics, gt_data, pred_data)
        classes = sorted(set(r[4] for img in gt_data for r in img) | set(r[4] for img in pred_data for r in img))
        rec = tool_record(tool, gt_boxes, pred_boxes, classes)
        lines = tool_main_lines(gt_text, pred_text) if name in cases.MAIN_SETS else None
        cases.store(name, gt_data, pred_data, tied, classes, rec, lines, out)
        print("%-16s %2d images, %3d objects, %3d detections%s: mAP %.2f, AP@0.5 %.4f, %d points%s" % (
            name, len(gt_data), sum(map(len, gt_data)), sum(map(len, pred_data)), " (tied: this machine's order)" if tied else "",
            rec["mAP"][0], rec["t0/avg_prec"][0], rec["t0/precisions"].size, "; __main__: %d lines" % len(lines) if lines else ""))
    gt_boxes, pred_boxes, _, _ = tool_inputs(metrics, *cases.MALFORMED)
    try:
        tool.get_avg_precision_at_iou(gt_boxes, pred_boxes, iou_thr=0.5)
        raised = False
    except AssertionError:
        raised = True
    out["malformed/raises"] = np.array([raised])
    print("malformed box: the tool raises: %s" % raised)
    np.savez_compressed(cases.GOLDEN, **out)
    print("wrote %s (%d bytes)" % (cases.GOLDEN, os.path.getsize(cases.GOLDEN)))


if __name__ == "__main__":
    main()
