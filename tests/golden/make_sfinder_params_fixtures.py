#!/usr/bin/env python3
"""Generates tests/golden/sfinder_params.npz by running the REFERENCE's ``SFinder.compute_source_params`` and the beam part of
``SFinder.set_img_size_params`` (mrcnn/sfinder.py under /root/reference) on the hand-built sources of
tests/sfinder_params_cases.py over a small seeded image, and recording inputs and outputs only -- no reference source text.
Runs only where the reference is present; the .npz is committed and pins caesar-mrcnn_amd/sfinder.py
(tests/test_sfinder_params_cpu.py, tests/test_sfinder_params_gpu.py).

The reference module's third-party imports are absent here, so stand-ins are registered first (install_stubs of
make_sfinder_fixtures.py).  Four of them ARE called on this path and are written here:

  cv.moments            its defining sums in NumPy: m00 = sum I, m10 = sum x I, m01 = sum y I (I = 1 where the image is non-zero
                        for a binary image), in float64;
  sigma_clipped_stats   returns a sentinel: the fixture does not pin the clipping (tests pin it on constructed inputs);
  utils.read_fits /     this package's reader (caesar-mrcnn_amd/fits.py, pinned elsewhere);
  utils.get_fits_header
  WCS                   a recorder with a fixed affine answer (sfinder_params_cases.RecorderWCS).

So the fixture pins the offset and cut-out arithmetic, the NaN fill, the float32 reductions, the centroid arithmetic, the keys
and where the WCS answers go -- not the astropy / OpenCV numerics.
"""
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_reference_fixtures as base            # noqa: E402
import make_sfinder_fixtures as sbase             # noqa: E402
import sfinder_params_cases as cases              # noqa: E402


def moments(image, binary=False):
    a = np.asarray(image)
    a = (a != 0).astype(np.float64) if binary else a.astype(np.float64)
    ys, xs = np.arange(a.shape[0], dtype=np.float64)[:, None], np.arange(a.shape[1], dtype=np.float64)[None, :]
    return {"m00": float(a.sum()), "m10": float((a * xs).sum()), "m01": float((a * ys).sum())}


def main():
    sbase.install_stubs()
    sys.path.insert(0, base.REF)
    from mrcnn import sfinder as ref
    from mrcnn.config import Config
    from caesar_mrcnn_amd import fits
    ref.cv = types.SimpleNamespace(moments=moments)
    ref.sigma_clipped_stats = lambda data: cases.SENTINEL
    ref.utils = types.SimpleNamespace(read_fits=fits.read_fits, get_fits_header=fits.get_fits_header)
    ref.WCS = cases.RecorderWCS

    img, srcs = cases.make_image(), cases.make_sources()
    results, beams = {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        for hname, cards in cases.headers().items():
            path = os.path.join(tmp, hname + ".fits")
            cases.write_image(path, img, cards)

            class Cfg(Config):
                NAME = "fixture"
                NUM_CLASSES = 4
                IMG_PATH = path
                IMG_XMIN = IMG_XMAX = IMG_YMIN = IMG_YMAX = -1
                SPLIT_IMG_IN_TILES = False
                MPI = None

            sf = ref.SFinder(None, Cfg())
            assert sf.set_img_size_params() == 0 and (sf.nx, sf.ny) == (cases.NX, cases.NY)
            beams[hname] = float(sf.beamArea)
            results[hname] = []
            with np.errstate(all="ignore"):
                for s in srcs:
                    r = sf.compute_source_params(dict(s))
                    results[hname].append(r)
                    print("%-8s %-12s nPix %4d  S %-12.6g X0 %-8.4f Y0 %-8.4f X0w %-8.4f Y0w %-8.4f flux %.6g" % (
                        hname, s["name"], r["nPix"], r["S"], r["X0"], r["Y0"], r["X0w"], r["Y0w"], r["flux"]))
    np.savez_compressed(cases.GOLDEN, **cases.encode(img, srcs, results, beams))
    print("wrote %s (%d bytes)" % (cases.GOLDEN, os.path.getsize(cases.GOLDEN)))


if __name__ == "__main__":
    main()
