"""Seeded scenes for the detection overlay (caesar-mrcnn_amd/draw.py, csrc/draw.hip), shared by
tests/test_draw_cpu.py and tests/test_draw_gpu.py.  A scene is the dict of draw.render_host.  Frames are at most 64 x 70 and the
canvases at most 962 pixels wide; the host statement of a scene is computed once (``expected``) and handed out read-only."""
import functools
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "draw.npz")
CLASS_NAMES = ["bkg", "spurious", "compact", "extended", "extended-multisland", "flagged", "unheard-of"]


def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def golden_scene(scale=2):
    """The fixture's image and masks as a shaded scene (boxes from the masks, score captions)."""
    g = golden()
    masks = [m for m in g["masks"]]
    colours = [tuple(float(v) for v in c) for c in g["colours"]]
    boxes = [bbox(m) for m in masks]
    return {"image": g["image"].astype(np.uint8), "scale": scale, "shaded": True, "masks": masks, "colours": colours, "boxes": boxes,
            "gt_boxes": [], "gt_colours": [], "texts": score_texts(boxes, [0.5 + 0.1 * k for k in range(len(masks))])}


def bbox(mask):
    ys, xs = np.nonzero(mask)
    return [int(ys.min()), int(xs.min()), int(ys.max()) + 1, int(xs.max()) + 1] if ys.size else [0, 0, 0, 0]


def score_texts(boxes, scores):
    from caesar_mrcnn_amd import draw
    return [("{:.2f}".format(s), b[1] + (b[3] - b[1]) // 2 - 4, b[0] - 1, draw.CAPTION_COLOUR) for b, s in zip(boxes, scores)]


def label_texts(boxes, labels, scores, colours):
    from caesar_mrcnn_amd import draw
    return [("{} {:.2f}".format(l, s), b[1], b[0] + 8, draw.colour8(c)) for b, l, s, c in zip(boxes, labels, scores, colours)]


def _shape_mask(rng, H, W, layout, k):
    yy, xx = np.mgrid[0:H, 0:W]
    if layout == "corner":                                         # everything piled into the top-left corner, nothing elsewhere
        cy, cx, r = int(rng.integers(0, max(H // 4, 1))), int(rng.integers(0, max(W // 4, 1))), int(rng.integers(1, 7))
    else:
        cy, cx, r = int(rng.integers(0, H)), int(rng.integers(0, W)), int(rng.integers(1, 9))
    kind = k % 4
    if kind == 0:
        m = (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r
    elif kind == 1:
        m = (abs(yy - cy) <= r) & (abs(xx - cx) <= 2 * r)
    elif kind == 2:                                                # a ring: a hole inside the contour
        d = (yy - cy) ** 2 + (xx - cx) ** 2
        m = (d <= r * r) & (d >= (r // 2) ** 2)
    else:
        m = ((abs(yy - cy) <= r) & (abs(xx - cx) <= r)) & (rng.random((H, W)) < 0.6)
    return m.astype(np.uint8)


def make_scene(H, W, n, scale, shaded=False, labels=False, gt=0, gt_classes=True, layout="spread", specials=False, seed=0):
    """n masks (discs, bars, rings, speckle) with their own boxes; with `specials`, some of them are replaced by a mask that
    touches all four frame edges, a full frame, a single pixel, an EMPTY mask (box all zero) and valid masks whose boxes are
    zero-area, inverted or reach beyond the frame; captions then get clipped at all four canvas edges."""
    from caesar_mrcnn_amd import draw
    rng = np.random.default_rng(1000 * seed + 7 * n + H + W)
    image = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
    masks = [_shape_mask(rng, H, W, layout, k) for k in range(n)]
    if specials and n >= 1:
        frame = np.zeros((H, W), np.uint8)
        frame[0, :] = frame[-1, :] = 1
        frame[:, 0] = frame[:, -1] = 1
        masks[0] = frame                                           # touches every edge; its caption is cut at the top and the left
    if specials and n >= 8:
        masks[1] = np.ones((H, W), np.uint8)
        masks[2] = np.zeros((H, W), np.uint8)                      # empty
        masks[3] = np.zeros((H, W), np.uint8)
        masks[3][H // 2, W // 2] = 1                               # one pixel
        masks[4] = np.zeros((H, W), np.uint8)
        masks[4][H - 1, W - 1] = 1                                 # the last pixel: captions cut at the right and at the bottom
    boxes = [bbox(m) for m in masks]
    if specials and n >= 8:
        y1, x1, y2, x2 = boxes[5]
        boxes[5] = [y1, x1, y1, x2]                                # zero area
        boxes[6] = [boxes[6][2], boxes[6][3], boxes[6][0], boxes[6][1]]           # inverted
        boxes[7] = [-3, -5, H + 3, W + 6]                          # beyond the frame and the margin
    class_ids = [int(rng.integers(0, len(CLASS_NAMES))) for _ in range(n)]
    names = [CLASS_NAMES[c] for c in class_ids]
    colours = [draw.CLASS_COLOR_MAP.get(name, draw.UNKNOWN_COLOUR) for name in names]
    scores = [float(rng.uniform(0.7, 1.0)) for _ in range(n)]
    gt_boxes, gt_colours = [], []
    for k in range(gt):
        y1, x1 = int(rng.integers(-2, H)), int(rng.integers(-2, W))
        gt_boxes.append([y1, x1, y1 + int(rng.integers(0, H // 2 + 2)), x1 + int(rng.integers(0, W // 2 + 2))])
        name = CLASS_NAMES[int(rng.integers(0, len(CLASS_NAMES)))] if gt_classes else "bkg"
        gt_colours.append(draw.CLASS_COLOR_MAP.get(name, draw.UNKNOWN_COLOUR))
    texts = label_texts(boxes, names, scores, colours) if labels else score_texts(boxes, scores)
    if specials:
        texts.append(("Edge_Case-9.5?", W - 3, H + 4, (10, 20, 30)))                  # upper case, '?' -> a filled cell; right / bottom cut
        texts.append(("left", -9, 5, (200, 0, 100)))                                  # starts left of the canvas
    return {"image": image, "scale": scale, "shaded": shaded, "masks": masks, "colours": colours, "boxes": boxes, "gt_boxes": gt_boxes,
            "gt_colours": gt_colours, "texts": texts}


# id -> make_scene arguments.  Canvas widths: 74, 148, 370, 962 (37 x 70), 68, 136, 340 (64 x 64), 37, 74, 185 (1 x 33): multiples of
# 4 take the kernel's 96-bit stores, the others its byte stores; none is a multiple of the 128-pixel tile.
FRAME_CASES = {
    "37x70_s1_n1": dict(H=37, W=70, n=1, scale=1),
    "37x70_s2_n40_shaded_labels_gt": dict(H=37, W=70, n=40, scale=2, shaded=True, labels=True, gt=5, specials=True),
    "37x70_s5_n100_corner_shaded": dict(H=37, W=70, n=100, scale=5, shaded=True, layout="corner", gt=3, gt_classes=False),
    "37x70_s13_n40_default_scale": dict(H=37, W=70, n=40, scale=13, specials=True, gt=2),
    "64x64_s1_n100": dict(H=64, W=64, n=100, scale=1, specials=True, labels=True),
    "64x64_s2_n1_edges_shaded": dict(H=64, W=64, n=1, scale=2, shaded=True, specials=True, gt=1),
    "64x64_s5_n40_gt_bkg": dict(H=64, W=64, n=40, scale=5, gt=6, gt_classes=False, specials=True, shaded=True),
    "64x64_s5_n100_corner": dict(H=64, W=64, n=100, scale=5, layout="corner", labels=True),
    "1x33_s1_n1": dict(H=1, W=33, n=1, scale=1, specials=True, shaded=True),
    "1x33_s2_n40": dict(H=1, W=33, n=40, scale=2, specials=True, gt=2),
    "1x33_s5_n100_shaded": dict(H=1, W=33, n=100, scale=5, shaded=True, labels=True, gt=1, gt_classes=False),
    "37x70_s2_no_masks_gt_only": dict(H=37, W=70, n=0, scale=2, gt=4),
}


@functools.lru_cache(maxsize=None)
def frame_case(name):
    return make_scene(seed=sorted(FRAME_CASES).index(name), **FRAME_CASES[name])


@functools.lru_cache(maxsize=None)
def expected(name):
    """draw.render_host of the case, computed once; read-only."""
    from caesar_mrcnn_amd import draw
    out = draw.render_host(golden_scene() if name == "golden" else frame_case(name))
    out.setflags(write=False)
    return out


class StubModel(object):
    """MaskRCNN.detect's result, planted (tests/test_analyze_cpu.py does the same)."""

    def __init__(self, result):
        self.result = result

    def detect(self, images, verbose=0):
        return [self.result]


def png_pixels(data):
    """Decode an 8-bit RGB, non-interlaced PNG with zlib and struct only -> (uint8 [h, w, 3], the chunk names in order)."""
    import struct
    import zlib
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    at, names, idat, head = 8, [], b"", None
    while at < len(data):
        n, tag = struct.unpack(">I4s", data[at:at + 8])
        body = data[at + 8:at + 8 + n]
        assert struct.unpack(">I", data[at + 8 + n:at + 12 + n])[0] == zlib.crc32(tag + body) & 0xFFFFFFFF, tag
        names.append(tag)
        if tag == b"IHDR":
            head = struct.unpack(">IIBBBBB", body)
        if tag == b"IDAT":
            idat += body
        at += 12 + n
    w, h, depth, colour_type, compression, filt, interlace = head
    assert (depth, colour_type, compression, filt, interlace) == (8, 2, 0, 0, 0)
    raw = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(h, 1 + 3 * w)
    assert not raw[:, 0].any()                                    # filter type 0 on every row
    return raw[:, 1:].reshape(h, w, 3).copy(), names


def table_cases():
    """[(name, H, W, scale, n_planes, tables, status)]: 0, -1 (malformed) or -4 (past a cap).  Shared with tests/test_draw_gpu.py,
    where the C entry must answer the same and launch nothing."""
    from caesar_mrcnn_amd import draw
    sc = make_scene(6, 7, 3, 2, shaded=True, gt=2, seed=3)
    good = draw.device_tables(sc)

    def mod(**fields):
        t = {k: (v.copy() if v is not None else None) for k, v in good.items()}
        for key, value in fields.items():
            table, i, name = key.split("__")
            t[table][name][int(i)] = value
        return t
    out = [("good", 6, 7, 2, 3, good, 0), ("no planes but detections name them", 6, 7, 2, 0, good, -1),
           ("empty frame", 0, 7, 2, 3, good, -1), ("scale 0", 6, 7, 0, 3, good, -1), ("negative planes", 6, 7, 2, -1, good, -1),
           ("unknown kind", 6, 7, 2, 3, mod(items__0__kind=2), -1), ("colour past the palette", 6, 7, 2, 3, mod(items__4__colour=len(good["palette"])), -1),
           ("negative colour", 6, 7, 2, 3, mod(items__1__colour=-1), -1), ("plane past the planes", 6, 7, 2, 3, mod(items__2__plane=3), -1),
           ("plane -2", 6, 7, 2, 3, mod(items__2__plane=-2), -1), ("gt box with a plane", 6, 7, 2, 3, mod(items__0__plane=0), -1),
           ("detection without a plane", 6, 7, 2, 3, mod(items__2__plane=-1), 0),
           ("text past the glyphs", 6, 7, 2, 3, mod(texts__2__count=good["texts"]["count"][2] + 1), -1),
           ("negative first", 6, 7, 2, 3, mod(texts__0__first=-1), -1), ("negative count", 6, 7, 2, 3, mod(texts__0__count=-1), -1),
           ("text colour", 6, 7, 2, 3, mod(texts__1__colour=99), -1),
           ("frame side cap", 16385, 1, 1, 3, good, -4), ("frame side at cap", 16384, 1, 1, 3, good, 0),
           ("scale cap", 6, 7, 65, 3, good, -4), ("scale at cap", 6, 7, 64, 3, good, 0),
           ("canvas side cap", 1021, 1, 64, 3, good, -4), ("canvas side at cap", 1020, 1, 64, 3, good, 0),
           ("canvas bytes cap", 16384, 16384, 2, 3, good, -4),
           ("coordinate cap", 6, 7, 2, 3, mod(items__3__x2=2 ** 20 + 1), -4), ("coordinate at cap", 6, 7, 2, 3, mod(items__3__x2=-2 ** 20), 0),
           ("anchor cap", 6, 7, 2, 3, mod(texts__0__ya=-2 ** 20 - 1), -4)]
    bad_glyph = mod()
    bad_glyph["glyphs"][1] = 1 << 35
    out.append(("glyph bit 35", 6, 7, 2, 3, bad_glyph, -1))
    many = mod()
    many["items"] = np.tile(good["items"][:1], 4097)
    out.append(("items cap", 6, 7, 2, 3, many, -4))
    many = mod()
    many["items"] = np.tile(good["items"][:1], 4096)
    out.append(("items at cap", 6, 7, 2, 3, many, 0))
    long_text = mod()
    long_text["glyphs"] = np.zeros(300, np.uint64)
    long_text["texts"] = good["texts"][:1].copy()
    long_text["texts"]["first"], long_text["texts"]["count"] = 0, 257
    out.append(("text length cap", 6, 7, 2, 3, long_text, -4))
    colours = mod()
    colours["palette"] = np.zeros((257, 4), np.uint8)
    colours["shade"] = np.zeros((257, 3, 256), np.uint8)
    out.append(("colour cap", 6, 7, 2, 3, colours, -4))
    return out
