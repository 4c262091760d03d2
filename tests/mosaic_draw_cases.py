"""Planes, pixel lists and the small catalogue of the mosaic-picture tests.  Not a test module: imported by
test_mosaic_draw_cpu.py and test_mosaic_draw_gpu.py, so that the GPU entries are held to the very inputs the host statements
were checked on."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def noise_plane(ny, nx, seed, blobs=6):
    """Unit noise with a few Gaussian blobs (a wide zscale range, bytes all over 0 .. 255)."""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:ny, 0:nx]
    img = rng.normal(0.0, 1.0, (ny, nx)).astype(np.float32)
    for _ in range(blobs):
        cy, cx, s = rng.uniform(0, ny), rng.uniform(0, nx), rng.uniform(1.5, 5.0)
        img += np.float32(rng.uniform(10.0, 60.0)) * np.exp(-0.5 * (((yy - cy) / s) ** 2 + ((xx - cx) / s) ** 2)).astype(np.float32)
    return img


def plane_97x61():
    """97 x 61 (5917 pixels: six chunks of 1024, the last one partial): scattered NaNs, a NaN strip and one -inf.  The -inf is
    the plane's minimum, so the NaNs are filled with it and count as not finite too."""
    img = noise_plane(97, 61, 11)
    rng = np.random.RandomState(12)
    img[rng.randint(0, 97, 40), rng.randint(0, 61, 40)] = np.nan
    img[30:33, 5:50] = np.nan
    img[70, 20] = -np.inf
    return img


def plane_nan_chunks():
    """97 x 61 with the NaNs concentrated in the chunks 1 and 3 (finite minimum: NaNs are filled and stay samples) and two
    infinities in chunk 4: the rank of a sample among the finite pixels differs from its position behind them."""
    img = noise_plane(97, 61, 21)
    flat = img.reshape(-1)
    flat[1024 + 100:1024 + 900] = np.nan
    flat[3 * 1024 + 5:3 * 1024 + 1000:3] = np.nan
    flat[4 * 1024 + 17] = np.inf
    flat[4 * 1024 + 600] = -np.inf
    return img


def plane_nan_chunks_infinite_fill():
    """The same with no finite minimum taken away: chunk 0 starts with a -inf, so every NaN becomes -inf and is skipped."""
    img = plane_nan_chunks()
    img[0, 3] = -np.inf
    return img


def plane_one_finite():
    img = np.full((9, 13), np.nan, np.float32)
    img[4, 7] = 2.5
    return img


def plane_2049x2048():
    """4098 chunks: the smallest shape past the one-workgroup chunk table (4096 chunks) -- five super-chunks of the new scan, the
    last one of two chunks.  NaN runs of different lengths, among them whole chunks and the border between super-chunks 0 and 1
    (chunks 1023 | 1024), so that the sample ranks slide against the positions from the first super-chunk on."""
    rng = np.random.RandomState(31)
    ny, nx = 2049, 2048
    img = rng.normal(0.0, 1.0, (ny, nx)).astype(np.float32)
    for _ in range(12):
        cy, cx, s = rng.uniform(0, ny), rng.uniform(0, nx), rng.uniform(4.0, 30.0)
        y0, y1, x0, x1 = int(max(cy - 4 * s, 0)), int(min(cy + 4 * s, ny)), int(max(cx - 4 * s, 0)), int(min(cx + 4 * s, nx))
        gy, gx = np.mgrid[y0:y1, x0:x1]
        img[y0:y1, x0:x1] += np.float32(rng.uniform(20.0, 90.0)) * np.exp(-0.5 * (((gy - cy) / s) ** 2 + ((gx - cx) / s) ** 2)).astype(np.float32)
    flat = img.reshape(-1)
    flat[5000:5300] = np.nan                                 # inside chunk 4
    flat[1022 * 1024 + 500:1026 * 1024 + 10] = np.nan        # across the super-chunk border, two whole chunks among them
    flat[3000 * 1024:3002 * 1024] = np.nan                   # two whole chunks of super-chunk 2
    flat[4097 * 1024 + 1:4097 * 1024 + 700:2] = np.nan       # the last chunk
    img[1500:1510, 100:1900] = np.nan
    return img


# ---- pixel lists ([y, x], mosaic coordinates) ------------------------------------------------------------------------------------
def source_cases(k, h, w):
    """Pixel lists for a frame [h, w] shrunk by k: a source spanning several blocks (and a word edge when the frame is wide
    enough), a single pixel, an empty source, a pixel on the last partial block, a source with pixels outside the frame (dropped:
    past k h / k w and at negative coordinates)."""
    H, W = k * h, k * w
    span = [[y, x] for y in range(max(0, H // 2 - 2 * k), min(H, H // 2 + 2 * k + 1)) for x in range(max(0, W // 3), min(W, W // 3 + 3 * k + 2))
            if (x + y) % 3]
    wide = [[min(H - 1, 1), x] for x in range(0, W, max(1, k // 2 + 1))]                  # one row across every word of the frame
    single = [[H // 3, (2 * W) // 3]]
    last = [[H - 1, W - 1]]
    outside = [[H // 2, W - 1], [H // 2, W], [H // 2, W + 3 * k], [H, 0], [H + 7, 2], [-1, 0], [-k, -k], [0, -1], [0, 0]]
    return [span, wide, single, [], last, outside]


def blobs_384x320(n=40, seed=5):
    """n seeded blobs (filled ellipses with holes punched by a modulus) on a 384 x 320 mosaic; some touch the border."""
    rng = np.random.RandomState(seed)
    out = []
    for _ in range(n):
        cy, cx = rng.randint(0, 384), rng.randint(0, 320)
        ry, rx = rng.randint(1, 14), rng.randint(1, 20)
        pts = [[y, x] for y in range(max(0, cy - ry), min(384, cy + ry + 1)) for x in range(max(0, cx - rx), min(320, cx + rx + 1))
               if ((y - cy) / float(ry)) ** 2 + ((x - cx) / float(rx)) ** 2 <= 1.0 and (3 * x + 5 * y) % 7]
        out.append(pts or [[cy, cx]])
    return out


def planes_by_loop(pixel_lists, k, h, w):
    """The definition, pixel by pixel."""
    planes = np.zeros((len(pixel_lists), h, w), bool)
    for i, pixels in enumerate(pixel_lists):
        for y, x in pixels:
            if 0 <= y < k * h and 0 <= x < k * w:
                planes[i, y // k, x // k] = True
    return planes


def unpack_words(words, w):
    """int32 / uint32 [n, h, wpr] plane words -> (bool [n, h, w], the padding bits bool [n, h, 32 wpr - w])."""
    u = np.ascontiguousarray(words).view(np.uint32).astype("<u4")
    n, h, wpr = u.shape
    bits = np.unpackbits(u.view(np.uint8).reshape(n, h, wpr * 4), axis=2, bitorder="little").astype(bool)
    return bits[:, :, :w], bits[:, :, w:]


# ---- a catalogue of three sources, one of them merged ---------------------------------------------------------------------------
CATALOGUE_PLANE_SHAPE = (50, 70)


def catalogue():
    """Three sources on a 50 x 70 mosaic as SFinder.sources holds them.  S2 is merged: its x2 / y2 are the INCLUSIVE pixel
    maxima, the others' are the exclusive box corners -- the picture must use neither, but the boxes of the planes."""
    a = [[y, x] for y in range(4, 9) for x in range(10, 21)]                     # rows 4 .. 8, columns 10 .. 20
    b = [[y, x] for y in range(20, 31) for x in range(33, 38)] + [[25, 38], [25, 39]]     # rows 20 .. 30, columns 33 .. 39
    c = [[47, 66]]
    return [
        {"name": "S1", "class_name": "compact", "class_id": 3, "score": 0.912, "merged": False, "edge": False, "pixels": a,
         "x1": 10, "x2": 21, "y1": 4, "y2": 9, "vertexes": []},
        {"name": "S2", "class_name": "extended", "class_id": 4, "score": 0.5, "merged": True, "edge": True, "pixels": b,
         "x1": 33, "x2": 39, "y1": 20, "y2": 30, "vertexes": []},
        {"name": "S3", "class_name": "no-such-class", "class_id": 9, "score": 0.998, "merged": False, "edge": False, "pixels": c,
         "x1": 66, "x2": 67, "y1": 47, "y2": 48, "vertexes": []},
    ]


def sfinder_for(path, plane, sources, model=None):
    """An SFinder over the FITS file `path` (written here from `plane`) whose catalogue is `sources`: what a run leaves behind,
    without the run."""
    import sfinder_tiles_cases as tiles
    from caesar_mrcnn_amd import fits
    from caesar_mrcnn_amd.sfinder import SFinder
    fits.write_fits(path, plane)
    cfg = tiles.config(path)
    sf = SFinder(model or tiles.ThresholdModel(cfg), cfg)
    sf.image_id = os.path.splitext(os.path.basename(path))[0]
    sf.sources = {"sources": sources}
    return sf
