"""The detection overlay of Analyzer.draw_results as an integer raster: the frame, nearest-neighbour scaled onto
a white canvas with a margin of two frame pixels, under the shaded masks, the dashed ground-truth boxes, the detections' boxes
and mask contours and the captions in a 5 x 7 bitmap font.  The reference draws this with matplotlib (mrcnn/analyze.py:2039-2135);
its anti-aliased figure cannot be matched byte for byte, so the picture is DEFINED here: ``render_host`` is the NumPy statement
of that text, ``csrc/draw.hip`` (``ops.draw_overlay``) renders the same bytes on the GPU from ``device_tables`` of the same scene.
The one arithmetic piece the reference states in NumPy, visualize.apply_mask, is ``apply_mask`` here and pinned by
tests/golden/draw.npz.  No PIL, no matplotlib: ``write_png`` needs zlib and struct only.

A scene is a dict:
  image [H, W, 3]; scale s >= 1; shaded bool;
  masks [n] of [H, W] 0 / 1 arrays, colours [n] of (r, g, b) floats in 0 .. 1, boxes [n] of (y1, x1, y2, x2);
  gt_boxes [g] of (y1, x1, y2, x2), gt_colours [g] of (r, g, b) floats;
  texts [(string, xa, ya, (r8, g8, b8))]: the anchor is the bottom-left corner of the text block, in frame pixels.
"""
import struct
import zlib

import numpy as np

MARGIN = 2                               # frame pixels around the frame (the reference's axis limits -2 .. size + 2)
SHADE_ALPHA = 0.3                        # draw_shaded_masks: apply_mask(..., alpha=0.3)
BOX_ALPHA_NUM = (179, 76)                # alpha 0.7 in integers: out = (179 * colour + 76 * below + 127) // 255
CAPTION_COLOUR = (0, 206, 209)           # darkturquoise
UNKNOWN_COLOUR = (0, 1, 0)
CLASS_COLOR_MAP = {'bkg': (0, 0, 0), 'spurious': (1, 0, 0), 'compact': (0, 0, 1), 'extended': (1, 1, 0),
                   'extended-multisland': (1, 0.647, 0), 'flagged': (0, 0, 0),
                   'sidelobe': (1, 0, 0), 'source': (0, 0, 1), 'galaxy': (1, 1, 0)}
PNG_LEVEL = 1                            # zlib level of write_png (tools/draw_bench.py records what 1 and 6 cost)

GLYPH_W, GLYPH_H, GLYPH_ADVANCE = 5, 7, 6
KIND_GT_BOX, KIND_DETECTION = 0, 1       # mrcnn_draw_item.kind
# caps of mrcnn_draw_overlay (include/mrcnn_hip.h)
MAX_ITEMS, MAX_TEXTS, MAX_TEXT_CHARS, MAX_COLOURS, MAX_SCALE, MAX_DIM, MAX_COORD = 4096, 4096, 256, 256, 64, 16384, 1 << 20
MAX_CANVAS = 65536

_FONT_ROWS = {
    '0': ".###. #...# #..## #.#.# ##..# #...# .###.", '1': "..#.. .##.. ..#.. ..#.. ..#.. ..#.. .###.",
    '2': ".###. #...# ....# ...#. ..#.. .#... #####", '3': ".###. #...# ....# ..##. ....# #...# .###.",
    '4': "...#. ..##. .#.#. #..#. ##### ...#. ...#.", '5': "##### #.... ####. ....# ....# #...# .###.",
    '6': "..##. .#... #.... ####. #...# #...# .###.", '7': "##### ....# ...#. ..#.. .#... .#... .#...",
    '8': ".###. #...# #...# .###. #...# #...# .###.", '9': ".###. #...# #...# .#### ....# ...#. .##..",
    '.': "..... ..... ..... ..... ..... .##.. .##..", '-': "..... ..... ..... ##### ..... ..... .....",
    '_': "..... ..... ..... ..... ..... ..... #####", ' ': "..... ..... ..... ..... ..... ..... .....",
    'a': ".###. #...# #...# ##### #...# #...# #...#", 'b': "####. #...# #...# ####. #...# #...# ####.",
    'c': ".###. #...# #.... #.... #.... #...# .###.", 'd': "####. #...# #...# #...# #...# #...# ####.",
    'e': "##### #.... #.... ####. #.... #.... #####", 'f': "##### #.... #.... ####. #.... #.... #....",
    'g': ".###. #...# #.... #.### #...# #...# .####", 'h': "#...# #...# #...# ##### #...# #...# #...#",
    'i': ".###. ..#.. ..#.. ..#.. ..#.. ..#.. .###.", 'j': "..### ...#. ...#. ...#. ...#. #..#. .##..",
    'k': "#...# #..#. #.#.. ##... #.#.. #..#. #...#", 'l': "#.... #.... #.... #.... #.... #.... #####",
    'm': "#...# ##.## #.#.# #.#.# #...# #...# #...#", 'n': "#...# ##..# #.#.# #..## #...# #...# #...#",
    'o': ".###. #...# #...# #...# #...# #...# .###.", 'p': "####. #...# #...# ####. #.... #.... #....",
    'q': ".###. #...# #...# #...# #.#.# #..#. .##.#", 'r': "####. #...# #...# ####. #.#.. #..#. #...#",
    's': ".#### #.... #.... .###. ....# ....# ####.", 't': "##### ..#.. ..#.. ..#.. ..#.. ..#.. ..#..",
    'u': "#...# #...# #...# #...# #...# #...# .###.", 'v': "#...# #...# #...# #...# #...# .#.#. ..#..",
    'w': "#...# #...# #...# #.#.# #.#.# ##.## #...#", 'x': "#...# #...# .#.#. ..#.. .#.#. #...# #...#",
    'y': "#...# #...# .#.#. ..#.. ..#.. ..#.. ..#..", 'z': "##### ....# ...#. ..#.. .#... #.... #####",
}
# FONT[ch]: bool [7, 5], row 0 on top, column 0 on the left
FONT = {ch: np.array([[c == '#' for c in row] for row in rows.split()], bool) for ch, rows in _FONT_ROWS.items()}
FILLED_GLYPH = np.ones((GLYPH_H, GLYPH_W), bool)         # any character the font does not cover


def glyph(ch):
    return FONT.get(ch.lower(), FILLED_GLYPH)


_GLYPH_BITS = {}


def glyph_bits(ch):
    """The glyph as one integer: bit 5 * row + column."""
    ch = ch.lower()
    if ch not in _GLYPH_BITS:
        g = glyph(ch)
        _GLYPH_BITS[ch] = sum(1 << (GLYPH_W * r + c) for r in range(GLYPH_H) for c in range(GLYPH_W) if g[r, c])
    return _GLYPH_BITS[ch]


def colour8(colour):
    return tuple(int(c * 255) for c in colour)


def default_scale(H, W):
    return max(1, 1024 // (max(int(H), int(W)) + 2 * MARGIN))


def apply_mask(image, mask, color, alpha=SHADE_ALPHA):
    """visualize.apply_mask (mrcnn/visualize.py:72-80) on the reference's uint32 image: a float64 expression per channel, stored
    back into the integer image (truncation).  In place, and returned."""
    for c in range(3):
        image[:, :, c] = np.where(mask == 1, image[:, :, c] * (1 - alpha) + alpha * color[c] * 255, image[:, :, c])
    return image


def shade_table(colours, alpha=SHADE_ALPHA):
    """[K, 3, 256] uint8: apply_mask's expression for every 8-bit value.  A value in 0 .. 255 stays there (the expression is a
    convex combination with 255 * c, c <= 1), so looking the table up per mask, in order, IS the chain of apply_mask calls."""
    v = np.arange(256, dtype=np.uint32)
    out = np.zeros((len(colours), 3, 256), np.uint32)
    for k, color in enumerate(colours):
        for c in range(3):
            out[k, c] = v * (1 - alpha) + alpha * color[c] * 255
    assert int(out.max(initial=0)) <= 255
    return out.astype(np.uint8)


def canvas_shape(H, W, scale):
    return (scale * (H + 2 * MARGIN), scale * (W + 2 * MARGIN), 3)


def _fill(region, y1, y2, x1, x2, value):
    Hc, Wc = region.shape
    y1, y2, x1, x2 = max(y1, 0), min(y2, Hc), max(x1, 0), min(x2, Wc)
    if y2 > y1 and x2 > x1:
        region[y1:y2, x1:x2] = value


def box_outline(shape, scale, box, t):
    """bool [Hc, Wc]: the canvas rectangle of the box minus the same rectangle shrunk by t on every side, clipped."""
    region = np.zeros(shape, bool)
    y1, x1, y2, x2 = (int(v) for v in box)
    if y2 <= y1 or x2 <= x1:
        return region
    Y1, Y2, X1, X2 = scale * (y1 + MARGIN), scale * (y2 + MARGIN), scale * (x1 + MARGIN), scale * (x2 + MARGIN)
    _fill(region, Y1, Y2, X1, X2, True)
    _fill(region, Y1 + t, Y2 - t, X1 + t, X2 - t, False)
    return region


def mask_contour(mask, scale, t):
    """bool [Hc, Wc]: set canvas pixels with an unset canvas pixel at distance t above, below, left or right."""
    H, W = mask.shape
    s, m = scale, MARGIN
    big = np.zeros((s * (H + 2 * m) + 2 * t, s * (W + 2 * m) + 2 * t), bool)           # t unset canvas pixels on every side
    big[t + s * m:t + s * (m + H), t + s * m:t + s * (m + W)] = np.repeat(np.repeat(np.asarray(mask) == 1, s, axis=0), s, axis=1)
    Hc, Wc = s * (H + 2 * m), s * (W + 2 * m)
    centre = big[t:t + Hc, t:t + Wc]
    around = big[0:Hc, t:t + Wc] & big[2 * t:2 * t + Hc, t:t + Wc] & big[t:t + Hc, 0:Wc] & big[t:t + Hc, 2 * t:2 * t + Wc]
    return centre & ~around


def text_region(shape, scale, text, xa, ya):
    """bool [Hc, Wc]: the cells of the text, its block's bottom-left corner at frame point (xa, ya); clipped, never wrapped."""
    region = np.zeros(shape, bool)
    s = scale
    top, left = s * (int(ya) + MARGIN) - GLYPH_H * s, s * (int(xa) + MARGIN)
    for k, ch in enumerate(text):
        g = glyph(ch)
        for r in range(GLYPH_H):
            for c in range(GLYPH_W):
                if g[r, c]:
                    _fill(region, top + r * s, top + (r + 1) * s, left + (GLYPH_ADVANCE * k + c) * s, left + (GLYPH_ADVANCE * k + c + 1) * s, True)
    return region


def _blend(canvas, region, colour):
    below = canvas[region].astype(np.uint32)
    canvas[region] = ((BOX_ALPHA_NUM[0] * np.array(colour, np.uint32) + BOX_ALPHA_NUM[1] * below + 127) // 255).astype(np.uint8)


def render_host(scene):
    """The raster of DESIGN.md 4.12 -> uint8 [s (H + 4), s (W + 4), 3]."""
    image = np.asarray(scene["image"])
    H, W = image.shape[:2]
    s, m = int(scene["scale"]), MARGIN
    shape = canvas_shape(H, W, s)
    t1, t2 = max(1, s // 4), max(1, s // 2)
    work = image.astype(np.uint32).copy()
    if scene["shaded"]:
        for mask, colour in zip(scene["masks"], scene["colours"]):
            work = apply_mask(work, np.asarray(mask), colour)
    canvas = np.full(shape, 255, np.uint8)
    canvas[s * m:s * (m + H), s * m:s * (m + W)] = np.repeat(np.repeat(work.astype(np.uint8), s, axis=0), s, axis=1)
    YY, XX = np.mgrid[0:shape[0], 0:shape[1]]
    dash = ((XX + YY) // (4 * t1)) % 2 == 0
    for box, colour in zip(scene["gt_boxes"], scene["gt_colours"]):
        _blend(canvas, box_outline(shape[:2], s, box, t1) & dash, colour8(colour))
    for mask, colour, box in zip(scene["masks"], scene["colours"], scene["boxes"]):
        _blend(canvas, box_outline(shape[:2], s, box, t2), colour8(colour))
        canvas[mask_contour(np.asarray(mask), s, t1)] = colour8(colour)
    for text, xa, ya, colour in scene["texts"]:
        canvas[text_region(shape[:2], s, text, xa, ya)] = colour
    return canvas


# ---- the tables of mrcnn_draw_overlay ------------------------------------------------------------------------------------------
ITEM_DTYPE = np.dtype([("kind", "<i4"), ("y1", "<i4"), ("x1", "<i4"), ("y2", "<i4"), ("x2", "<i4"), ("colour", "<i4"), ("plane", "<i4"),
                       ("pad", "<i4")])
TEXT_DTYPE = np.dtype([("ya", "<i4"), ("xa", "<i4"), ("colour", "<i4"), ("first", "<i4"), ("count", "<i4"), ("pad", "<i4", (3,))])


def device_tables(scene):
    """The scene as the POD tables of mrcnn_draw_overlay: dict of items (ITEM_DTYPE, ground-truth boxes first, then the detections,
    detection i on plane i), texts (TEXT_DTYPE), glyphs (uint64, one per character), palette (uint8 [K, 4]) and shade
    (uint8 [K, 3, 256]; None when the scene is not shaded)."""
    index, rgb8, rgbf = {}, [], []

    def colour_of(c8, cf):
        key = (tuple(c8), None if cf is None else tuple(float(v) for v in cf))
        if key not in index:
            index[key] = len(rgb8)
            rgb8.append(key[0])
            rgbf.append(key[1] if key[1] is not None else tuple(v / 255. for v in key[0]))
        return index[key]
    gt, det = scene["gt_boxes"], scene["boxes"]
    items = np.zeros(len(gt) + len(det), ITEM_DTYPE)
    for k, (box, colour) in enumerate(zip(gt, scene["gt_colours"])):
        items[k] = (KIND_GT_BOX,) + tuple(int(v) for v in box) + (colour_of(colour8(colour), colour), -1, 0)
    for i, (box, colour) in enumerate(zip(det, scene["colours"])):
        items[len(gt) + i] = (KIND_DETECTION,) + tuple(int(v) for v in box) + (colour_of(colour8(colour), colour), i, 0)
    texts = np.zeros(len(scene["texts"]), TEXT_DTYPE)
    glyphs = []
    for k, (text, xa, ya, colour) in enumerate(scene["texts"]):
        texts[k] = (int(ya), int(xa), colour_of(colour, None), len(glyphs), len(text), (0, 0, 0))
        glyphs.extend(glyph_bits(ch) for ch in text)
    if not rgb8:
        colour_of((0, 0, 0), None)
    palette = np.zeros((len(rgb8), 4), np.uint8)
    palette[:, :3] = np.array(rgb8, np.uint8)
    return {"items": items, "texts": texts, "glyphs": np.array(glyphs, np.uint64), "palette": palette,
            "shade": shade_table(rgbf) if scene["shaded"] else None}


def check_tables(H, W, scale, n_planes, tables):
    """The CPU restatement of mrcnn_draw_check: 0, -1 (MRCNN_ERR_ARG: a malformed table) or -4 (MRCNN_ERR_UNSUPPORTED: past a cap)."""
    items, texts, glyphs, palette = tables["items"], tables["texts"], tables["glyphs"], tables["palette"]
    K = len(palette)
    if H <= 0 or W <= 0 or scale <= 0 or n_planes < 0 or K <= 0:
        return -1
    if tables["shade"] is not None and tuple(np.shape(tables["shade"])) != (K, 3, 256):
        return -1
    for it in items:
        if it["kind"] not in (KIND_GT_BOX, KIND_DETECTION) or not 0 <= it["colour"] < K or not -1 <= it["plane"] < n_planes:
            return -1
        if it["kind"] == KIND_GT_BOX and it["plane"] != -1:
            return -1
    for t in texts:
        if not 0 <= t["colour"] < K or t["first"] < 0 or t["count"] < 0 or int(t["first"]) + int(t["count"]) > len(glyphs):
            return -1
    if any(int(g) >> (GLYPH_W * GLYPH_H) for g in glyphs):
        return -1
    past = H > MAX_DIM or W > MAX_DIM or scale > MAX_SCALE or len(items) > MAX_ITEMS or len(texts) > MAX_TEXTS or K > MAX_COLOURS
    past = past or len(glyphs) > MAX_TEXTS * MAX_TEXT_CHARS or any(int(t["count"]) > MAX_TEXT_CHARS for t in texts)
    for it in items:
        past = past or any(abs(int(it[k])) > MAX_COORD for k in ("y1", "x1", "y2", "x2"))
    for t in texts:
        past = past or abs(int(t["ya"])) > MAX_COORD or abs(int(t["xa"])) > MAX_COORD
    if not past:
        Hc, Wc, _ = canvas_shape(H, W, scale)
        past = Hc > MAX_CANVAS or Wc > MAX_CANVAS or 3 * Hc * Wc > 2 ** 31 - 1
    return -4 if past else 0


# ---- PNG -------------------------------------------------------------------------------------------------------------------------
def png_bytes(canvas, level=None):
    """uint8 [h, w, 3] -> an 8-bit RGB, non-interlaced PNG (filter type 0 on every row)."""
    canvas = np.ascontiguousarray(canvas, dtype=np.uint8)
    assert canvas.ndim == 3 and canvas.shape[2] == 3 and canvas.shape[0] > 0 and canvas.shape[1] > 0
    h, w = canvas.shape[:2]
    rows = np.zeros((h, 1 + 3 * w), np.uint8)
    rows[:, 1:] = canvas.reshape(h, 3 * w)

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)
    return b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)) + \
        chunk(b"IDAT", zlib.compress(rows.tobytes(), PNG_LEVEL if level is None else level)) + chunk(b"IEND", b"")


def write_png(outfile, canvas, level=None):
    with open(outfile, "wb") as fp:
        fp.write(png_bytes(canvas, level))
