"""The detection overlay on the host (caesar-mrcnn_amd/draw.py, Analyzer.draw_results): the shading against the
reference's apply_mask (tests/golden/draw.npz), the raster against pictures worked out here from the text of 4.12 -- a scalar,
pixel-by-pixel restatement (``pixel_statement``) and arrays written down by hand -- the font, the PNG writer, file naming and
gating, the command line, and the table validation of ops.draw_overlay restated on the CPU."""
import importlib.util
import os

import numpy as np
import pytest

import caesar_mrcnn_amd  # noqa: F401
from caesar_mrcnn_amd import analyze, draw

import analyze_post_cases as post
import draw_cases as cases
import tester_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLUE, RED, YELLOW = (0, 0, 1), (1, 0, 0), (1, 1, 0)


# ---- the shading: pinned to the reference ---------------------------------------------------------------------------------------
def test_shading_equals_reference_at_every_step():
    g = cases.golden()
    assert g["image"].shape == (37, 70, 3) and g["image"].dtype == np.uint32 and g["masks"].shape == (5, 37, 70)
    assert float(g["alpha"]) == draw.SHADE_ALPHA and [1, 0.647, 0] in g["colours"].tolist()
    assert sorted(set(map(tuple, g["colours"].tolist()))) == sorted(set(draw.CLASS_COLOR_MAP[k] for k in
                                                                     ("bkg", "spurious", "compact", "extended", "extended-multisland", "flagged")))
    work = g["image"].copy()
    table = draw.shade_table([tuple(c) for c in g["colours"]])
    looked_up = g["image"].astype(np.uint8)
    for k in range(5):
        work = draw.apply_mask(work, g["masks"][k], tuple(g["colours"][k]))
        assert work.dtype == np.uint32 and np.array_equal(work, g["steps"][k]), k
        for c in range(3):                                         # the device form: one table look-up per mask and channel
            looked_up[:, :, c] = np.where(g["masks"][k] == 1, table[k, c][looked_up[:, :, c]], looked_up[:, :, c])
        assert np.array_equal(looked_up, g["steps"][k].astype(np.uint8)), k
    assert (g["steps"][4] != g["steps"][3]).any() and (g["steps"][1] != g["steps"][0]).any()
    # the whole picture's frame region is the last step, scaled
    canvas = cases.expected("golden")
    sc = cases.golden_scene()
    s = sc["scale"]
    inner = canvas[2 * s:-2 * s, 2 * s:-2 * s]
    plain = dict(sc, boxes=[], masks=[], colours=[], texts=[], shaded=False, image=g["steps"][4].astype(np.uint8))
    assert np.array_equal(draw.render_host(plain)[2 * s:-2 * s, 2 * s:-2 * s][::s, ::s], g["steps"][4].astype(np.uint8))
    assert inner.shape == (37 * s, 70 * s, 3)


# ---- the raster, pixel by pixel, from the text of DESIGN.md 4.12 ----------------------------------------------------------------
def pixel_statement(sc, Y, X):
    """One canvas pixel, layer by layer, in plain Python integers."""
    img = np.asarray(sc["image"])
    H, W = img.shape[:2]
    s, m = sc["scale"], 2
    Hc, Wc = s * (H + 2 * m), s * (W + 2 * m)
    t1, t2 = max(1, s // 4), max(1, s // 2)

    def set_at(mask, y, x):                                        # canvas pixel (y, x) of the scaled mask; unset off the frame
        if y < 0 or x < 0 or y >= Hc or x >= Wc:
            return False
        fy, fx = y // s - m, x // s - m
        return 0 <= fy < H and 0 <= fx < W and mask[fy][fx] == 1

    def on_outline(box, t):
        y1, x1, y2, x2 = box
        if y2 <= y1 or x2 <= x1:
            return False
        Y1, Y2, X1, X2 = s * (y1 + m), s * (y2 + m), s * (x1 + m), s * (x2 + m)
        inside = Y1 <= Y < Y2 and X1 <= X < X2
        shrunk = Y1 + t <= Y < Y2 - t and X1 + t <= X < X2 - t
        return inside and not shrunk

    def blend(colour, below):
        return [(179 * int(c * 255) + 76 * b + 127) // 255 for c, b in zip(colour, below)]

    fy, fx = Y // s - m, X // s - m
    if 0 <= fy < H and 0 <= fx < W:
        px = [int(v) for v in img[fy][fx]]
        if sc["shaded"]:
            for mask, colour in zip(sc["masks"], sc["colours"]):
                if mask[fy][fx] == 1:
                    px = [int(px[c] * (1 - 0.3) + 0.3 * colour[c] * 255) for c in range(3)]
        px = [v % 256 for v in px]
    else:
        px = [255, 255, 255]
    for box, colour in zip(sc["gt_boxes"], sc["gt_colours"]):
        if on_outline(box, t1) and ((X + Y) // (4 * t1)) % 2 == 0:
            px = blend(colour, px)
    for mask, colour, box in zip(sc["masks"], sc["colours"], sc["boxes"]):
        if on_outline(box, t2):
            px = blend(colour, px)
        if set_at(mask, Y, X) and not (set_at(mask, Y - t1, X) and set_at(mask, Y + t1, X) and set_at(mask, Y, X - t1) and set_at(mask, Y, X + t1)):
            px = [int(c * 255) for c in colour]
    for text, xa, ya, colour in sc["texts"]:
        top, left = s * (ya + m) - 7 * s, s * (xa + m)
        if top <= Y < top + 7 * s and X >= left:
            k, cell = (X - left) // (6 * s), ((X - left) % (6 * s)) // s
            if k < len(text) and cell < 5 and draw.glyph(text[k])[(Y - top) // s][cell]:
                px = list(colour)
    return px


def picture(sc):
    img = np.asarray(sc["image"])
    Hc, Wc = sc["scale"] * (img.shape[0] + 4), sc["scale"] * (img.shape[1] + 4)
    return np.array([[pixel_statement(sc, Y, X) for X in range(Wc)] for Y in range(Hc)], np.uint8)


def _frame(value=100):
    rng = np.random.default_rng(5)
    return rng.integers(0, 256, (6, 7, 3)).astype(np.uint8) if value is None else np.full((6, 7, 3), value, np.uint8)


def _mask(*rects):
    m = np.zeros((6, 7), np.uint8)
    for y1, y2, x1, x2 in rects:
        m[y1:y2, x1:x2] = 1
    return m


def _scene(image, scale, masks=(), colours=(), boxes=None, gt_boxes=(), gt_colours=(), texts=(), shaded=False):
    masks = list(masks)
    return {"image": image, "scale": scale, "shaded": shaded, "masks": masks, "colours": list(colours),
            "boxes": [cases.bbox(m) for m in masks] if boxes is None else list(boxes), "gt_boxes": list(gt_boxes),
            "gt_colours": list(gt_colours), "texts": list(texts)}


SCALES = [1, 2, 5]


def test_one_mask_one_box_written_down_by_hand():
    """s = 1 on a grey 6 x 7 frame: a 3 x 3 mask at rows 1 .. 3, columns 2 .. 4, its box and its score."""
    mask = _mask((1, 4, 2, 5))
    sc = _scene(_frame(100), 1, [mask], [BLUE], texts=cases.score_texts([cases.bbox(mask)], [0.9]))
    assert sc["boxes"] == [[1, 2, 4, 5]] and sc["texts"] == [("0.90", -1, 0, (0, 206, 209))]
    want = np.full((10, 11, 3), 255, np.uint8)
    want[2:8, 2:9] = 100
    # the box outline is the ring of the 3 x 3 canvas rectangle rows 3 .. 5, columns 4 .. 6, blended: (179 c + 76 * 100 + 127) // 255
    ring = [(y, x) for y in (3, 4, 5) for x in (4, 5, 6) if (y, x) != (4, 5)]
    assert (179 * 0 + 7600 + 127) // 255 == 30 and (179 * 255 + 7600 + 127) // 255 == 209
    for y, x in ring:
        want[y, x] = (30, 30, 209)
    # ... and the contour (the same eight pixels: the centre has its four neighbours set) covers it with the opaque colour
    for y, x in ring:
        want[y, x] = (0, 0, 255)
    # "0.90" at frame point (-1, 0): the block's bottom is canvas row 2, so only the glyphs' rows 5 and 6 show, in rows 0 and 1;
    # it starts at canvas column 1; the '.' starts at column 7 and its fifth cell, the '9' and the last '0' lie off the canvas
    for y, x in ((0, 1), (0, 5), (1, 2), (1, 3), (1, 4), (0, 8), (0, 9), (1, 8), (1, 9)):
        want[y, x] = (0, 206, 209)
    got = draw.render_host(sc)
    assert got.dtype == np.uint8 and got.shape == (10, 11, 3) and np.array_equal(got, want)
    assert np.array_equal(picture(sc), want)
    only_box = draw.render_host(_scene(_frame(100), 1, [np.zeros((6, 7), np.uint8)], [BLUE], boxes=[[1, 2, 4, 5]]))
    assert [tuple(only_box[y, x]) for y, x in ring] == [(30, 30, 209)] * 8 and tuple(only_box[4, 5]) == (100, 100, 100)


@pytest.mark.parametrize("s", SCALES)
def test_one_mask_one_box_every_pixel(s):
    mask = _mask((1, 4, 2, 5), (4, 5, 3, 4))
    sc = _scene(_frame(None), s, [mask], [YELLOW], texts=cases.score_texts([cases.bbox(mask)], [0.97]))
    got = draw.render_host(sc)
    assert got.shape == (10 * s, 11 * s, 3) and np.array_equal(got, picture(sc))
    img = sc["image"]
    # margin: white, two frame pixels wide, except where the caption reaches into it
    blank = draw.render_host(dict(sc, texts=[]))
    assert (blank[:2 * s] == 255).all() and (blank[-2 * s:] == 255).all() and (blank[:, :2 * s] == 255).all() and (blank[:, -2 * s:] == 255).all()
    # nearest neighbour: a frame pixel no layer touches fills its s x s cell
    assert (blank[2 * s:3 * s, 2 * s:3 * s] == img[0, 0]).all() and (blank[7 * s:8 * s, 8 * s:9 * s] == img[5, 6]).all()
    t1, t2 = max(1, s // 4), max(1, s // 2)
    # contour thickness t1 inside the mask's left edge (canvas column 4 s), outline thickness t2 at the box's top edge
    row = (2 + 2) * s + s // 2                                    # through frame row 2
    assert all(tuple(blank[row, 4 * s + d]) == (255, 255, 0) for d in range(t1))
    if s == 5:
        assert tuple(blank[row, 4 * s + t2]) != (255, 255, 0)     # past both: the frame pixel again (t2 = 2 > t1 = 1)
        assert (blank[row, 4 * s + t2] == img[2, 2]).all()


@pytest.mark.parametrize("s", SCALES)
def test_dashed_gt_box_pattern(s):
    sc = _scene(_frame(40), s, gt_boxes=[[0, 1, 5, 6], [2, 2, 2, 5], [4, 5, 3, 1]], gt_colours=[RED, BLUE, BLUE])
    got = draw.render_host(sc)
    assert np.array_equal(got, picture(sc))
    t1 = max(1, s // 4)
    changed = (got != draw.render_host(dict(sc, gt_boxes=[], gt_colours=[]))).any(axis=2)
    on = draw.box_outline(got.shape[:2], s, [0, 1, 5, 6], t1)
    YY, XX = np.mgrid[0:got.shape[0], 0:got.shape[1]]
    dash = ((XX + YY) // (4 * t1)) % 2 == 0
    assert np.array_equal(changed, on & dash) and (on & dash).any() and (on & ~dash).any()      # (the empty and inverted boxes paint nothing)
    red = ((179 * 255 + 76 * 40 + 127) // 255, (76 * 40 + 127) // 255, (76 * 40 + 127) // 255)
    assert red == (191, 12, 12) and {tuple(v) for v in got[on & dash]} == {red} and {tuple(v) for v in got[on & ~dash]} == {(40, 40, 40)}


def test_blend_on_a_known_background():
    image = _frame(0)
    image[:, :, 0], image[:, :, 1], image[:, :, 2] = 255, 128, 1
    sc = _scene(image, 1, [np.zeros((6, 7), np.uint8)], [(1, 0.647, 0)], boxes=[[0, 0, 6, 7]])
    got = draw.render_host(sc)
    assert int(0.647 * 255) == 164
    want = ((179 * 255 + 76 * 255 + 127) // 255, (179 * 164 + 76 * 128 + 127) // 255, (179 * 0 + 76 * 1 + 127) // 255)
    assert want == (255, 153, 0)
    assert tuple(got[2, 2]) == want and tuple(got[7, 8]) == want and tuple(got[3, 3]) == (255, 128, 1)
    # on the white margin: a box that reaches beyond the frame
    out = draw.render_host(_scene(image, 1, [np.zeros((6, 7), np.uint8)], [BLUE], boxes=[[-1, -1, 7, 8]]))
    assert tuple(out[1, 1]) == ((76 * 255 + 127) // 255, (76 * 255 + 127) // 255, 255) == (76, 76, 255)
    assert np.array_equal(out, picture(_scene(image, 1, [np.zeros((6, 7), np.uint8)], [BLUE], boxes=[[-1, -1, 7, 8]])))


@pytest.mark.parametrize("s", SCALES)
@pytest.mark.parametrize("shaded", [False, True])
def test_two_overlapping_detections_order_matters(s, shaded):
    a, b = _mask((0, 4, 0, 4)), _mask((2, 6, 2, 7))
    first = _scene(_frame(None), s, [a, b], [RED, BLUE], shaded=shaded)
    second = _scene(_frame(None), s, [b, a], [BLUE, RED], shaded=shaded)
    got1, got2 = draw.render_host(first), draw.render_host(second)
    assert np.array_equal(got1, picture(first)) and np.array_equal(got2, picture(second))
    assert not np.array_equal(got1, got2)
    # where a's contour crosses b's (frame pixel (2, 3): on a's right edge and on b's top edge) the later detection wins
    y, x = (2 + 2) * s, (3 + 2) * s + s - 1
    assert tuple(got1[y, x]) == (0, 0, 255) and tuple(got2[y, x]) == (255, 0, 0)
    if shaded:                                                     # inside both masks, off every line: shaded red then blue, or blue then red
        v = [int(c) for c in first["image"][3, 3]]
        rb = [int(int(v[c] * 0.7 + 0.3 * RED[c] * 255) * 0.7 + 0.3 * BLUE[c] * 255) for c in range(3)]
        br = [int(int(v[c] * 0.7 + 0.3 * BLUE[c] * 255) * 0.7 + 0.3 * RED[c] * 255) for c in range(3)]
        if s == 5:
            assert list(got1[5 * s + 2, 5 * s + 2]) == rb and list(got2[5 * s + 2, 5 * s + 2]) == br and rb != br


@pytest.mark.parametrize("s", SCALES)
def test_one_pixel_mask_and_mask_touching_all_edges(s):
    one = _mask((3, 4, 5, 6))
    full = np.ones((6, 7), np.uint8)
    hollow = full.copy()
    hollow[1:5, 1:6] = 0
    for masks in ([one], [full], [hollow], [hollow, one]):
        sc = _scene(_frame(None), s, masks, [YELLOW, RED][:len(masks)])
        assert np.array_equal(draw.render_host(sc), picture(sc))
    t1 = max(1, s // 4)
    cell = draw.mask_contour(one, s, t1)[5 * s:6 * s, 7 * s:8 * s]
    want = np.ones((s, s), bool)
    want[t1:s - t1, t1:s - t1] = False                             # a square ring of thickness t1 (the whole cell when s <= 2 t1)
    assert np.array_equal(cell, want) and draw.mask_contour(one, s, t1).sum() == want.sum()
    edge = draw.mask_contour(full, s, t1)
    ring = np.zeros_like(edge)
    ring[2 * s:8 * s, 2 * s:9 * s] = True
    ring[2 * s + t1:8 * s - t1, 2 * s + t1:9 * s - t1] = False     # the frame's border: the margin beyond it is unset
    assert np.array_equal(edge, ring)


@pytest.mark.parametrize("s", SCALES)
def test_captions_clipped_at_the_top_and_the_right(s):
    top = _mask((0, 2, 1, 3))                                      # y1 = 0: the block's bottom is one frame row above the frame
    right = _mask((3, 5, 5, 7))                                    # the text runs off the right canvas edge
    for labels in (False, True):
        boxes = [cases.bbox(top), cases.bbox(right)]
        texts = cases.label_texts(boxes, ["compact", "galaxy"], [0.9, 0.8], [BLUE, YELLOW]) if labels else cases.score_texts(boxes, [0.9, 0.8])
        sc = _scene(_frame(60), s, [top, right], [BLUE, YELLOW], texts=texts)
        got = draw.render_host(sc)
        assert np.array_equal(got, picture(sc))
        region = draw.text_region(got.shape[:2], s, texts[1][0], texts[1][1], texts[1][2])
        assert s * (texts[1][1] + 2) + 6 * s * len(texts[1][0]) > got.shape[1] and region.any()       # wider than the canvas: cut, not wrapped
        assert not region[:max(s * (texts[1][2] + 2) - 7 * s, 0)].any() and not region[s * (texts[1][2] + 2):].any()
    # score mode, y1 = 0: anchor row -1 -> the block covers canvas rows [s - 7 s, s): only its last row of cells is on the canvas
    sc = _scene(_frame(60), s, [top], [BLUE], texts=cases.score_texts([cases.bbox(top)], [0.12]))
    region = draw.text_region((10 * s, 11 * s), s, *sc["texts"][0][:3])
    assert region[:s].any() and not region[s:].any()
    assert sc["texts"][0][1:3] == (1 + 2 // 2 - 4, -1)


# ---- captions, font ---------------------------------------------------------------------------------------------------------------
def test_font_table():
    want = set("0123456789.-_ abcdefghijklmnopqrstuvwxyz")
    assert set(draw.FONT) == want and len(draw.FONT) == 40
    for ch, g in draw.FONT.items():
        assert g.shape == (7, 5) and g.dtype == np.bool_, ch
        assert g.any() == (ch != " "), ch
    shapes = {g.tobytes() for g in draw.FONT.values()}
    assert len(shapes) == 40                                      # no two characters look the same
    assert np.array_equal(draw.glyph("A"), draw.FONT["a"]) and np.array_equal(draw.glyph("Z"), draw.FONT["z"])
    for ch in "?/+%(":
        assert draw.glyph(ch).all() and draw.glyph(ch).shape == (7, 5)
    assert draw.glyph_bits("?") == 2 ** 35 - 1 and draw.glyph_bits(" ") == 0
    assert draw.glyph_bits("_") == 0b11111 << 30 and draw.glyph_bits("-") == 0b11111 << 15
    one = draw.text_region((14, 40), 2, "1", 0, 5)                 # cell = 2 canvas pixels; the block's top-left corner at (0, 4)
    assert np.array_equal(one[0:14:2, 4:14:2], draw.FONT["1"]) and one.sum() == 4 * draw.FONT["1"].sum()
    two = draw.text_region((7, 40), 1, "11", 0, 5)
    assert np.array_equal(two[:, 2:7], draw.FONT["1"]) and np.array_equal(two[:, 8:13], draw.FONT["1"]) and not two[:, 7].any()


def _planted(**settings):
    """An Analyzer after predict on the chain_of_three scenario (two final masks), nothing written."""
    name, shape, objs, _ = post.scenarios()[0]
    an = post.analyzer(objs, shape, settings, device=False)
    return post.run(an, shape), shape


def test_caption_text_and_anchor_in_both_modes():
    an, shape = _planted()
    sc = an._draw_scene()
    assert len(sc["texts"]) == len(an.masks_final) == 2 and sc["scale"] == 1024 // 104 == draw.default_scale(*shape)
    for i, (text, xa, ya, colour) in enumerate(sc["texts"]):
        y1, x1, y2, x2 = [int(v) for v in an.bboxes[i]]
        assert text == "{:.2f}".format(an.scores_final[i]) and (xa, ya) == (x1 + (x2 - x1) // 2 - 4, y1 - 1) and colour == (0, 206, 209)
    an.draw_class_label_in_caption = True
    sc = an._draw_scene()
    for i, (text, xa, ya, colour) in enumerate(sc["texts"]):
        y1, x1, y2, x2 = [int(v) for v in an.bboxes[i]]
        assert text == an.captions[i] and text.startswith("compact 0.") and (xa, ya) == (x1, y1 + 8) and colour == (0, 0, 255)
    assert an.class_color_map == {'bkg': (0, 0, 0), 'spurious': (1, 0, 0), 'compact': (0, 0, 1), 'extended': (1, 1, 0),
                                  'extended-multisland': (1, 0.647, 0), 'flagged': (0, 0, 0), 'sidelobe': (1, 0, 0),
                                  'source': (0, 0, 1), 'galaxy': (1, 1, 0)}
    assert set(an.class_color_map) == set(an.class_color_map_ds9)
    an.class_names = ["bkg", "spurious", "never-heard-of", "galaxy"]
    assert an._draw_scene()["colours"] == [(0, 1, 0), (0, 1, 0)]                      # an unknown name
    an.bboxes_gt, an.class_ids_gt_merged = [[1, 2, 3, 4], [5, 6, 7, 8]], []
    assert an._draw_scene()["gt_colours"] == [(0, 0, 0), (0, 0, 0)]                   # 'bkg' without class ids
    an.class_ids_gt_merged = [3, 1]
    assert an._draw_scene()["gt_colours"] == [(1, 1, 0), (1, 0, 0)]
    an.draw_scale = 3
    assert an.render_results(device=False).shape == (3 * (shape[0] + 4), 3 * (shape[1] + 4), 3)


def test_render_results_is_the_host_statement_and_refuses_other_images(caplog):
    an, shape = _planted()
    got = an.render_results(device=False)
    assert np.array_equal(got, draw.render_host(an._draw_scene())) and an.draw_timing == {}
    assert np.array_equal(an.render_results(), got)               # no GPU behind the stub model: the same statement
    for image in (np.zeros(shape, np.uint8), np.zeros(shape + (4,), np.uint8), np.zeros(shape + (1,), np.uint8)):
        an.image = image
        assert an.render_results() is None and an.draw_results("never.png") == -1
    an.accept_detection(shape + (3,), an.model.result, image_id="img")                # the image stayed on the device
    assert an.image is None and an.render_results() is None
    assert any("nothing is drawn" in r.getMessage() for r in caplog.records)
    assert not os.path.exists("never.png")


# ---- PNG --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1), (3, 5), (66, 93)])
def test_png_round_trip(tmp_path, shape):
    rng = np.random.default_rng(shape[0])
    canvas = rng.integers(0, 256, shape + (3,)).astype(np.uint8)
    path = str(tmp_path / "a.png")
    draw.write_png(path, canvas)
    data = open(path, "rb").read()
    pixels, names = cases.png_pixels(data)
    assert names == [b"IHDR", b"IDAT", b"IEND"] and np.array_equal(pixels, canvas)
    assert data == draw.png_bytes(canvas) and np.array_equal(cases.png_pixels(draw.png_bytes(canvas, level=9))[0], canvas)
    try:
        from PIL import Image
    except ImportError:
        return
    with Image.open(path) as im:
        assert im.mode == "RGB" and np.array_equal(np.asarray(im), canvas)


def test_png_writer_needs_neither_pil_nor_matplotlib():
    src = open(os.path.join(ROOT, "caesar-mrcnn_amd", "draw.py")).read()
    assert "import PIL" not in src and "from PIL" not in src and "import matplotlib" not in src and "pyplot" not in src


# ---- file naming and gating ---------------------------------------------------------------------------------------------------
def test_predict_draws_only_on_request(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    name, shape, objs, _ = post.scenarios()[0]
    an = post.analyzer(objs, shape, {}, device=False)
    assert an.draw is False and an.draw_shaded_masks is False and an.draw_class_label_in_caption is False and an.draw_scale is None
    post.run(an, shape)
    assert os.listdir(str(tmp_path)) == []                        # draw False: no file
    an.draw = True
    post.run(an, shape)
    assert os.listdir(str(tmp_path)) == ["out_img.png"]
    pixels, _ = cases.png_pixels(open("out_img.png", "rb").read())
    assert an.draw_timing["encode_ms"] > 0                        # (the host statement has no other phase to time)
    assert np.array_equal(pixels, an.render_results(device=False))
    an.outfile = str(tmp_path / "sub.png")
    post.run(an, shape)
    assert sorted(os.listdir(str(tmp_path))) == ["out_img.png", "sub.png"]
    assert open("out_img.png", "rb").read() == open("sub.png", "rb").read()
    an.draw_shaded_masks = True
    post.run(an, shape)
    assert open("out_img.png", "rb").read() != open("sub.png", "rb").read()
    # draw_results_host by itself
    assert an.draw_results_host(str(tmp_path / "host.png")) == 0
    assert open(str(tmp_path / "host.png"), "rb").read() == open("sub.png", "rb").read()


def test_predict_draws_nothing_when_nothing_is_detected(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    shape = (70, 100)
    for objs in ([], [(post.rect(shape, 5, 15, 5, 15), post.COMPACT, 0.5)]):
        an = post.analyzer(objs, shape, {"draw": True}, device=False)
        post.run(an, shape)
        if not objs:
            assert os.listdir(str(tmp_path)) == []
    # (a frame whose detections all fall below the score cut has objects but no final mask: the reference draws the bare frame)
    assert os.listdir(str(tmp_path)) == ["out_img.png"]
    pixels, _ = cases.png_pixels(open("out_img.png", "rb").read())
    s = draw.default_scale(*shape)
    assert (pixels[2 * s:-2 * s, 2 * s:-2 * s] == 0).all() and (pixels[:2 * s] == 255).all()


def test_inspect_results_name(tmp_path, monkeypatch):
    from caesar_mrcnn_amd import fits
    monkeypatch.chdir(tmp_path)
    ds, model = tester_cases.get_data_scene()
    path = str(tmp_path / "img_remap.fits")
    fits.write_fits(path, np.full(tester_cases.S33, 1e-4, np.float32))
    for on in (False, True):
        an = analyze.Analyzer(model, tester_cases.cfg(), ds, [], [])
        an.draw = on
        assert an.inspect_results(0, path) == 0
        pngs = sorted(f for f in os.listdir(str(tmp_path)) if f.endswith(".png"))
        assert pngs == (["out_img_remap_iduuid-0.png"] if on else [])
    pixels, _ = cases.png_pixels(open("out_img_remap_iduuid-0.png", "rb").read())
    assert len(an.bboxes_gt) == 2 and len(an.masks_final) >= 1 and np.array_equal(pixels, an.render_results(device=False))
    tester = analyze.ModelTester(model, tester_cases.cfg(), ds)
    assert tester.draw is False


def _run_py():
    spec = importlib.util.spec_from_file_location("_run_py_draw", os.path.join(ROOT, "scripts", "run.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_run_py_passes_draw_and_detect_outfile_through(caplog):
    run = _run_py()
    base = ["detect", "--image", "a.fits"]
    args = run.parse_args(base)
    assert args.draw is False and args.detect_outfile == "" and run.draw_settings(args) == (False, "")
    assert run.draw_settings(run.parse_args(base + ["--draw"])) == (True, "")
    assert run.draw_settings(run.parse_args(base + ["--detect_outfile", "x.png"])) == (True, "x.png")
    assert run.draw_settings(run.parse_args(base + ["--draw", "--detect_outfile", "x.png"])) == (True, "x.png")
    assert run.draw_settings(run.parse_args(base + ["--draw"]), ntiles=4) == (False, "")          # tiles are never drawn
    assert any("draws nothing" in r.getMessage() for r in caplog.records)
    assert run.parse_args(["test", "--datalist", "l.dat", "--reference_tester", "--draw"]).draw is True


# ---- the tables of ops.draw_overlay: validation restated on the CPU -----------------------------------------------------------------
def test_table_validation_restated():
    rows = cases.table_cases()
    assert {r[6] for r in rows} == {0, -1, -4}
    for name, H, W, scale, n_planes, tables, want in rows:
        assert draw.check_tables(H, W, scale, n_planes, tables) == want, name
    good = rows[0][5]
    assert good["items"].dtype.itemsize == 32 and good["texts"].dtype.itemsize == 32 and good["glyphs"].dtype == np.uint64
    assert good["items"]["kind"].tolist() == [0, 0, 1, 1, 1] and good["items"]["plane"].tolist() == [-1, -1, 0, 1, 2]
    assert good["shade"].shape == (len(good["palette"]), 3, 256) and draw.device_tables(dict(cases.make_scene(6, 7, 3, 2, seed=3)))["shade"] is None


def test_device_tables_of_every_frame_case_pass_the_check():
    for name in sorted(cases.FRAME_CASES):
        sc = cases.frame_case(name)
        H, W = sc["image"].shape[:2]
        assert draw.check_tables(H, W, sc["scale"], len(sc["masks"]), draw.device_tables(sc)) == 0, name


def test_failed_device_form_is_left_for_the_process_and_a_refusal_is_not(monkeypatch, caplog):
    from caesar_mrcnn_amd import ops
    an, shape = _planted()
    want = an.render_results(device=False)
    monkeypatch.setattr(analyze.Analyzer, "has_gpu", staticmethod(lambda model: True))
    post.check_failure_policy(monkeypatch, caplog, "draw_results_device",
                              lambda entered: monkeypatch.setattr(analyze.Analyzer, "_render_device", post.planted_failure(entered)),
                              an.render_results, want, np.array_equal)
    refused = []

    def refuse(self, scene):
        refused.append(1)
        raise ops.DrawUnsupported("scale 204 is above 64")
    monkeypatch.setattr(analyze, "device_forms_failed", set())
    monkeypatch.setattr(analyze.Analyzer, "_render_device", refuse)
    with caplog.at_level("DEBUG", logger="mrcnn"):
        caplog.clear()
        for k in (1, 2):                                           # this frame only: the next one tries the device again
            assert np.array_equal(an.render_results(), want) and refused == [1] * k and analyze.device_forms_failed == set()
        assert [r.levelname for r in caplog.records] == ["DEBUG", "DEBUG"]
    with pytest.raises(ops.DrawUnsupported):
        an.render_results(device=True)                             # asked for by name: raised, not taken to the host
