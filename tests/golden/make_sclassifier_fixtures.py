#!/usr/bin/env python3
"""Generates tests/golden/sclassifier.npz by running the REFERENCE's ``SClassifier.classify_source`` (mrcnn/classifier.py of the
reference checkout, make_reference_fixtures.REF) on the hand-built scenarios of tests/sclassifier_cases.py, and recording inputs and outputs only -- no reference
source text.  Runs only where the reference is present; the .npz is committed and pins caesar-mrcnn_amd/classifier.py
(tests/test_sclassifier_cpu.py).

The reference module's third-party imports are absent here, so stand-ins are registered first (install_stubs of
make_sfinder_fixtures.py).  Two names of the reference are replaced: ``mrcnn.classifier.Analyzer`` by the stand-in of
sclassifier_cases.py, which answers every cut-out with the detections planted for it and logs the image and the boxes it was
given; and ``mrcnn.utils.stretch_img`` (astropy's ZScaleInterval) by this package's ``fits.stretch_img``.  So the fixture pins
the windows, the member scan, the visited bookkeeping, the matching and crop_img's in-place NaN fill -- not astropy.

Recorded per scenario: the status of every classify_source call, the visited flags after each, the local boxes every
Analyzer.predict call received, the class_info entries (class_id, class_name, snames) and the mosaic as the run left it.  The
cut-out image is not recorded: the reference's crop_img hands gray2rgb the 2-D crop, which takes its first three ROWS as the
channels and returns a [width, 3] array; fits.crop_img of this package repeats the plane three times instead (as read_fits does).
"""
import contextlib
import io
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_reference_fixtures as base            # noqa: E402
import make_sfinder_fixtures as sbase             # noqa: E402
import sclassifier_cases as cases                 # noqa: E402


def main():
    sbase.install_stubs()
    sys.path.insert(0, base.REF)
    from mrcnn import classifier as ref
    from caesar_mrcnn_amd import fits
    ref.utils.stretch_img = fits.stretch_img
    out = {}
    quiet = io.StringIO()
    for sc in cases.scenarios():
        log = []
        ref.Analyzer = cases.analyzer_class(sc["planted"], log)
        clf = cases.setup(ref.SClassifier(None, cases.Cfg()), sc, ref.SData)
        with contextlib.redirect_stdout(quiet), warnings.catch_warnings():
            warnings.simplefilter("ignore")
            statuses, visited = cases.drive(clf)
        assert all(c.score == 0 for s in clf.sources for c in s.class_info), "the reference leaves SClassInfo.score at 0"
        for k, v in cases.record(clf, log, statuses, visited).items():
            out["%s/%s" % (sc["name"], k)] = v
        print("%-10s %2d sources, %2d calls, statuses %s, %d cut-outs, %d class infos, visited %s" % (
            sc["name"], len(clf.sources), len(statuses), statuses, len(log), len(cases.class_infos(clf)),
            "".join("x" if s.visited else "." for s in clf.sources)))
    np.savez_compressed(cases.GOLDEN, **out)
    print("wrote %s (%d bytes)" % (cases.GOLDEN, os.path.getsize(cases.GOLDEN)))


if __name__ == "__main__":
    main()
