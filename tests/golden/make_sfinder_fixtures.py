#!/usr/bin/env python3
"""Generates tests/golden/sfinder_merge.npz by running the REFERENCE's ``SFinder`` (mrcnn/sfinder.py under /root/reference:
create_tile_tasks, find_sources_at_edge, merge_edge_sources) on the hand-built tile results of tests/sfinder_cases.py and
recording inputs and outputs only -- no reference source text.  Runs only where the reference is present; the .npz is
committed and pins caesar-mrcnn_amd/sfinder.py (tests/test_sfinder_cpu.py, tests/test_sfinder_gpu.py).

The reference module's third-party imports are absent here, so inert stand-ins are registered first (install_stubs of
make_reference_fixtures.py plus the few more sfinder.py and analyze.py pull in); none of them is called on this path.  One
function IS called and has no stand-in: skimage's ``find_contours``.  The reference module's name is pointed at this package's
``analyze.find_contours`` (itself pinned against contourpy in tests/test_analyze_cpu.py), so the ``vertexes`` in the fixture pin
the 10-pixel offset arithmetic and the plumbing around the contour finder, not skimage itself.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_reference_fixtures as base        # noqa: E402
import sfinder_cases as cases                 # noqa: E402


def install_stubs():
    base.install_stubs()
    base._stub("numpyencoder", NumpyEncoder=json.JSONEncoder)
    # (an installed matplotlib asks a registered IPython for its version and its shell: answer "recent" and "none")
    base._stub("IPython", version_info=(8, 30, 0), get_ipython=lambda: None)
    for name in ("regions", "astropy.coordinates", "astropy.wcs.utils", "IPython.display", "skimage.draw", "imutils",
                 "matplotlib", "matplotlib.pyplot", "matplotlib.patches", "matplotlib.lines", "sklearn", "sklearn.metrics",
                 "networkx", "scipy", "scipy.ndimage"):
        if name not in sys.modules:
            try:
                __import__(name)
            except Exception:
                base._stub(name)


def main():
    install_stubs()
    sys.path.insert(0, base.REF)
    from mrcnn import sfinder as ref
    from mrcnn.config import Config
    from caesar_mrcnn_amd import analyze
    ref.find_contours = analyze.find_contours

    class Cfg(Config):
        NAME = "fixture"
        NUM_CLASSES = len(cases.CLASS_NAMES)
        IMG_PATH = "mosaic.fits"
        MPI = None
        MAX_NTASKS_PER_WORKER = 100

    ref_cfg = Cfg()
    cfg = cases.make_config()
    out = {}
    for sc in cases.grid_scenarios() + cases.merge_scenarios():
        sf = ref.SFinder(None, ref_cfg)
        grid, sources = cases.drive(sf, sc, cfg)
        cases.encode(sc["name"], sc, grid, sources, out)
        print("%-16s %2d tiles, %2d detections -> %2d sources, %d merged" % (
            sc["name"], sum(len(t) for t in grid), len(sc["dets"]), len(sources), sum(bool(s["merged"]) for s in sources)))
    np.savez_compressed(cases.GOLDEN, **out)
    print("wrote %s (%d bytes)" % (cases.GOLDEN, os.path.getsize(cases.GOLDEN)))


if __name__ == "__main__":
    main()
