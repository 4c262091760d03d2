#!/usr/bin/env python3
"""Generates tests/golden/draw.npz by running the REFERENCE's ``visualize.apply_mask`` (mrcnn/visualize.py under /root/reference)
the way ``Analyzer.draw_results`` does (mrcnn/analyze.py:2061, :2109): a uint32 image, the masks applied one after the other with
alpha 0.3, each in the colour of its class.  Inputs and outputs are recorded only -- no reference source text.  Runs only where
the reference is present; the .npz is committed and pins caesar-mrcnn_amd/draw.py (``apply_mask``, ``shade_table``:
tests/test_draw_cpu.py) and the shading of csrc/draw.hip (tests/test_draw_gpu.py).

``visualize.py`` imports skimage, matplotlib and IPython at module level; none of them is called by ``apply_mask``, so inert
stand-ins are registered where they are absent (install_stubs of make_sfinder_fixtures.py).

The scene: a seeded 37 x 70 x 3 image (uint8 values as uint32, the extremes 0 and 255 planted), five overlapping 0 / 1 masks, and
every colour of the reference's colour map (analyze.py:683-690), (1, 0.647, 0) included; black occurs twice there and once here.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_reference_fixtures as base            # noqa: E402
import make_sfinder_fixtures as sbase             # noqa: E402

GOLDEN = os.path.join(HERE, "draw.npz")
SHAPE = (37, 70)
ALPHA = 0.3
COLOURS = [(0, 0, 0), (1, 0, 0), (0, 0, 1), (1, 1, 0), (1, 0.647, 0)]         # bkg / flagged, spurious, compact, extended, extended-multisland


def scene():
    rng = np.random.default_rng(20261019)
    image = rng.integers(0, 256, SHAPE + (3,)).astype(np.uint32)
    image[0, 0], image[0, 1] = 0, 255
    H, W = SHAPE
    yy, xx = np.mgrid[0:H, 0:W]
    masks = np.zeros((5, H, W), np.uint8)
    masks[0] = (yy - 12) ** 2 + (xx - 20) ** 2 <= 100                       # a disc across the word border x = 31 | 32 ...
    masks[1] = (yy >= 5) & (yy < 30) & (xx >= 15) & (xx < 50)               # ... under a rectangle ...
    masks[2] = (yy - 25) ** 2 + (xx - 58) ** 2 <= 196                       # ... under a disc across x = 63 | 64 that leaves the frame
    masks[3] = rng.random(SHAPE) < 0.4                                      # scattered pixels over everything
    masks[4] = 1                                                            # the whole frame, the corners (0, 0) and (0, 1) with it
    return image, masks


def main():
    sbase.install_stubs()
    sys.path.insert(0, base.REF)
    from mrcnn import visualize
    image, masks = scene()
    colours = np.array(COLOURS, np.float64)
    steps = np.zeros((len(masks),) + image.shape, np.uint32)
    work = image.copy()
    for k in range(len(masks)):
        work = visualize.apply_mask(work, masks[k], tuple(COLOURS[k]), alpha=ALPHA)
        assert work.dtype == np.uint32
        steps[k] = work
        print("mask %d: %5d pixels set, %5d values changed, max %d" % (k, int(masks[k].sum()), int((steps[k] != (steps[k - 1] if k else image)).sum()),
                                                                       int(work.max())))
    np.savez_compressed(GOLDEN, image=image, masks=masks, colours=colours, alpha=np.float64(ALPHA), steps=steps)
    print("wrote %s (%d bytes)" % (GOLDEN, os.path.getsize(GOLDEN)))


if __name__ == "__main__":
    main()
