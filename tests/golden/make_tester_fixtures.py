#!/usr/bin/env python3
"""Generates tests/golden/tester.npz by running the REFERENCE's ``Analyzer.extract_gt_masks``, ``Analyzer.compute_performances``,
``Analyzer.get_data`` and ``ModelTester.update_performances / compute_performances / save`` (mrcnn/analyze.py under
/root/reference) on the hand-built scenes of tests/tester_cases.py, and recording inputs and outputs only -- no reference source
text.  Runs only where the reference is present; the .npz is committed and pins caesar-mrcnn_amd/analyze.py
(tests/test_tester_cpu.py, tests/test_tester_gpu.py).

The reference module's third-party imports are absent here, so stand-ins are registered first (install_stubs of
make_sfinder_fixtures.py).  ``sklearn.metrics.jaccard_score`` is the real one.  One stand-in IS called on this path:
``skimage.measure.label`` (through extract_mask_connected_components, connectivity=1), pointed at this package's
``analyze.label_components``.  ``compute_det_mask_pars`` (OpenCV contours, skimage regionprops) is not run: the scenes plant the
``det_obj_pars`` it would leave.  So the fixture pins the matching rules, the counters, the fillers, the table keys, the CSV bytes
and the printed blocks -- not OpenCV or skimage.
"""
import contextlib
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
import tester_cases as cases                      # noqa: E402


def main():
    sbase.install_stubs()
    sys.path.insert(0, base.REF)
    from sklearn.metrics import jaccard_score
    from mrcnn import analyze as ref
    from caesar_mrcnn_amd import analyze
    assert ref.jaccard_score is jaccard_score, "the real jaccard_score is what the fixture pins"

    def label(mask, background=0, return_num=True, connectivity=1):
        assert background == 0 and return_num and connectivity == 1
        return analyze.label_components(mask)
    ref.skimage.measure.label = label
    extract_bboxes = ref.utils.extract_bboxes

    def make_analyzer(sc):
        return ref.Analyzer(None, cases.cfg(), cases.StubDataset(sc["consider"]), [], [])

    out = {}
    quiet = io.StringIO()
    for sc in cases.scenarios():
        with contextlib.redirect_stdout(quiet):
            an = cases.drive(make_analyzer(sc), sc, extract_bboxes)
        rec = cases.analyzer_record(an, sc["shape"])
        cases.flatten(sc["name"], rec, out)
        print("%-14s gt %d -> %d, dets %d: detected %s, matching %s, ious %s" % (
            sc["name"], len(sc["gt"]), len(an.masks_gt_merged), len(sc["dets"]), an.is_gt_obj_detected,
            an.is_det_obj_matching_to_gt_obj, ["%.3f" % v for v in an.detobj_ious]))
    for run, names in cases.TESTER_RUNS.items():
        with tempfile.TemporaryDirectory() as tmp:
            tester = ref.ModelTester(None, cases.cfg(), cases.StubDataset())
            rec = cases.run_tester(tester, make_analyzer, names, extract_bboxes, tmp)
        cases.flatten("tester_" + run, rec, out)
        print("%s: completeness.csv %d bytes, reliability.csv %d bytes" % (run, rec["completeness_csv"].size, rec["reliability_csv"].size))
    for case in cases.REMAP_CASES:
        ds, model = cases.get_data_scene()
        an = ref.Analyzer(model, cases.cfg(), ds, [], [])
        with contextlib.redirect_stdout(quiet):
            rec = cases.run_get_data(an, case)
        cases.flatten("get_data_" + case, rec, out)
        print("%-14s status %d, class ids %s" % (case, int(rec["status"]), rec["class_ids"].tolist()))
    np.savez_compressed(cases.GOLDEN, **out)
    print("wrote %s (%d bytes)" % (cases.GOLDEN, os.path.getsize(cases.GOLDEN)))


if __name__ == "__main__":
    main()
