"""csrc/draw.hip (ops.draw_overlay, Analyzer.draw_results_device) against draw.render_host, the NumPy statement of DESIGN.md 4.12:
byte for byte throughout.  Frames are at most 64 x 70, canvases at most 481 x 962; the host statement of every case is computed
once (draw_cases.expected)."""
import ctypes

import numpy as np
import pytest
import torch

import caesar_mrcnn_amd  # noqa: F401
from caesar_mrcnn_amd import _hip, analyze, draw, ops

import analyze_post_cases as post
import draw_cases as cases

pytestmark = pytest.mark.gpu


def _planes(masks, dev):
    if not masks:
        return None
    stack = np.ascontiguousarray(np.stack([np.asarray(m) != 0 for m in masks], axis=-1))
    return ops.mask_planes_pack(torch.from_numpy(stack.view(np.uint8)).to(dev))


def _render(sc, dev, timing=None):
    image = torch.from_numpy(np.ascontiguousarray(sc["image"])).to(dev)
    return ops.draw_overlay(image, _planes(sc["masks"], dev), draw.device_tables(sc), sc["scale"], timing)


def _assert_equal(got, want, tag):
    assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == want.shape, tag
    got = got.cpu().numpy()
    if not np.array_equal(got, want):
        bad = np.argwhere((got != want).any(axis=2))
        raise AssertionError("%s: %d canvas pixels differ, the first at (Y, X) = %r: device %r, host %r" % (
            tag, len(bad), tuple(bad[0]), got[tuple(bad[0])].tolist(), want[tuple(bad[0])].tolist()))


def test_shading_fixture_through_the_device(dev):
    """tests/golden/draw.npz: the frame region of the canvas is the reference's last apply_mask step."""
    g = cases.golden()
    for scale in (1, 2):
        sc = cases.golden_scene(scale)
        got = _render(sc, dev)
        _assert_equal(got, cases.expected("golden") if scale == 2 else draw.render_host(sc), "golden, scale %d" % scale)
    bare = dict(cases.golden_scene(1), boxes=[[0, 0, 0, 0]] * 5, texts=[])            # shading only: no box, and ...
    got = _render(bare, dev).cpu().numpy()[2:-2, 2:-2]
    contour = np.zeros((37, 70), bool)
    for m in g["masks"]:
        contour |= draw.mask_contour(m, 1, 1)[2:-2, 2:-2]
    assert (~contour).sum() > 1000                                                    # ... off the contours, the reference's bytes
    assert np.array_equal(got[~contour], g["steps"][4].astype(np.uint8)[~contour])


@pytest.mark.parametrize("name", sorted(cases.FRAME_CASES))
def test_frame_cases(dev, name):
    sc = cases.frame_case(name)
    timing = {}
    got = _render(sc, dev, timing)
    _assert_equal(got, cases.expected(name), name)
    assert timing["canvas_bytes"] == got.numel() and timing["render_kernel_ms"] > 0
    assert torch.equal(_render(sc, dev), got)                                         # bitwise the same from run to run


def test_case_list_covers_what_it_says():
    widths = {cases.expected(n).shape[1] for n in cases.FRAME_CASES}
    assert {w % 4 == 0 for w in widths} == {True, False} and not any(w % 128 == 0 for w in widths)
    assert {len(cases.frame_case(n)["masks"]) for n in cases.FRAME_CASES} >= {0, 1, 40, 100}
    assert {cases.frame_case(n)["image"].shape[:2] for n in cases.FRAME_CASES} == {(37, 70), (64, 64), (1, 33)}
    assert {cases.frame_case(n)["scale"] for n in cases.FRAME_CASES} >= {1, 2, 5}
    sc = cases.frame_case("37x70_s5_n100_corner_shaded")
    boxes = np.array(sc["boxes"])
    assert boxes[:, 2].max() <= 37 // 4 + 7 and boxes[:, 3].max() <= 70 // 4 + 14    # everything in one corner
    sc = cases.frame_case("64x64_s5_n40_gt_bkg")
    assert not sc["masks"][2].any() and sc["boxes"][5][0] == sc["boxes"][5][2] and sc["boxes"][6][0] > sc["boxes"][6][2]
    assert sc["masks"][0][0].all() and sc["masks"][0][-1].all() and sc["masks"][0][:, 0].all() and sc["masks"][0][:, -1].all()
    # captions leave the canvas on all four sides
    s, (Hc, Wc) = sc["scale"], cases.expected("64x64_s5_n40_gt_bkg").shape[:2]
    tops = [s * (t[2] + 2) - 7 * s for t in sc["texts"]]
    assert min(tops) < 0 and max(s * (t[2] + 2) for t in sc["texts"]) > Hc
    assert min(s * (t[1] + 2) for t in sc["texts"]) < 0 and max(s * (t[1] + 2) + 6 * s * len(t[0]) for t in sc["texts"]) > Wc


def test_image_is_read_where_it_lies_and_not_written(dev):
    sc = cases.frame_case("37x70_s2_n40_shaded_labels_gt")
    image = torch.from_numpy(np.ascontiguousarray(sc["image"])).to(dev)
    planes = _planes(sc["masks"], dev)
    words = planes.words.clone()
    _assert_equal(ops.draw_overlay(image, planes, draw.device_tables(sc), sc["scale"]), cases.expected("37x70_s2_n40_shaded_labels_gt"), "again")
    assert torch.equal(planes.words, words) and np.array_equal(image.cpu().numpy(), sc["image"])


# ---- refusals: nothing is launched --------------------------------------------------------------------------------------------
def test_c_entry_answers_as_the_restated_check_and_launches_nothing(dev):
    L = _hip.lib()
    canary = torch.full((4096,), 7, dtype=torch.uint8, device=dev)
    p, stream = canary.data_ptr(), _hip.current_stream()
    for name, H, W, scale, n_planes, tables, want in cases.table_cases():
        assert draw.check_tables(H, W, scale, n_planes, tables) == want, name
        assert ops.draw_check(H, W, n_planes, tables, scale) == want, name
        if want == 0:
            continue
        d, items, texts, glyphs, _, _ = ops._draw_desc(H, W, n_planes, tables, scale)
        host = [a.ctypes.data_as(ctypes.c_void_p) if a.size else None for a in (items, texts, glyphs)]
        assert L.mrcnn_draw_overlay(ctypes.byref(d), host[0], host[1], host[2], p, p, p, p, p, p, p, p, p, stream) == want, name
    torch.cuda.synchronize()
    assert bool((canary == 7).all())
    # the wrapper: ValueError for malformed tables, DrawUnsupported past a cap -- before anything is allocated
    sc = cases.make_scene(6, 7, 3, 2, shaded=True, gt=2, seed=3)
    image, planes = torch.from_numpy(sc["image"]).to(dev), _planes(sc["masks"], dev)
    by_name = {r[0]: r for r in cases.table_cases()}
    with pytest.raises(ValueError):
        ops.draw_overlay(image, planes, by_name["unknown kind"][5], 2)
    with pytest.raises(ValueError):
        ops.draw_overlay(image, None, by_name["good"][5], 2)                          # detections name planes that are not there
    with pytest.raises(ops.DrawUnsupported):
        ops.draw_overlay(image, planes, by_name["good"][5], 65)
    with pytest.raises(_hip.HipPathError):
        ops.draw_overlay(torch.zeros((5, 7, 3), dtype=torch.uint8, device=dev), planes, by_name["good"][5], 2)
    assert issubclass(ops.DrawUnsupported, _hip.HipPathError)
    _assert_equal(ops.draw_overlay(image, planes, by_name["good"][5], 2), draw.render_host(sc), "good")


# ---- Analyzer ---------------------------------------------------------------------------------------------------------------------
def _analyzer_cases():
    by_name = {s[0]: s for s in post.scenarios()}
    return [by_name[k] for k in ("chain_of_three", "other_classes_touch_and_diagonal", "merge_and_select_off", "one_row_and_empty",
                                 "one_pixel_frame", "discs_24")]


@pytest.mark.parametrize("case", _analyzer_cases(), ids=lambda c: c[0])
def test_planes_left_on_the_device_give_the_same_picture(dev, case):
    """The planes extract_det_masks_device left (no upload) against planes packed from masks_final (one upload) against the host
    statement; shaded, with ground-truth boxes, in both caption modes."""
    name, shape, objs, settings = case
    pictures = []
    for postprocess_device in (True, False):
        an = post.run(post.analyzer(objs, shape, settings, device=postprocess_device), shape)
        rng = np.random.default_rng(len(objs))
        an.image = rng.integers(0, 256, tuple(shape) + (3,)).astype(np.uint8)
        an.draw_shaded_masks = True
        an.bboxes_gt, an.class_ids_gt_merged = [[0, 0, shape[0], shape[1]], [0, 0, 1, 1]], [2, 3]
        if draw.default_scale(*shape) > draw.MAX_SCALE:           # the 1 x 1 frame: 204 canvas pixels per frame pixel, past the cap
            with pytest.raises(ops.DrawUnsupported):
                an.render_results(device=True)
            assert np.array_equal(an.render_results(), an.render_results(device=False)) and an.draw_timing == {}      # this frame only
            assert "draw_results_device" not in analyze.device_forms_failed
            an.draw_scale = draw.MAX_SCALE
        for labels in (False, True):
            an.draw_class_label_in_caption = labels
            want = an.render_results(device=False)
            assert an.draw_timing == {}
            got = an.render_results(device=True)
            assert np.array_equal(got, want), (name, postprocess_device, labels)
            assert an.draw_timing["masks"] == len(an.masks_final) >= 1
            assert an.draw_timing["mask_uploads"] == (0 if postprocess_device else 1)
            assert np.array_equal(an.render_results(), want) and an.draw_timing["masks"] == len(an.masks_final)      # the default: the device
            pictures.append(want)
    assert np.array_equal(pictures[0], pictures[2]) and np.array_equal(pictures[1], pictures[3])
    assert not np.array_equal(pictures[0], pictures[1])


def test_frames_the_device_form_does_not_take(dev, monkeypatch):
    name, shape, objs, settings = post.scenarios()[0]
    an = post.run(post.analyzer(objs, shape, settings, device=False), shape)
    calls = []
    real = ops.draw_overlay
    monkeypatch.setattr(ops, "draw_overlay", lambda *a, **k: calls.append(1) or real(*a, **k))
    want = an.render_results(device=False)
    assert np.array_equal(an.render_results(), want) and calls == [1]
    an.draw_device_min_masks = 3                                  # fewer final masks than the threshold
    assert np.array_equal(an.render_results(), want) and calls == [1] and an.draw_timing == {}
    an.draw_device_min_masks = analyze.Analyzer.DRAW_DEVICE_MIN_MASKS
    an.image = an.image.astype(np.float32)                        # not 8-bit values: the reference's uint32 arithmetic, on the host
    assert an.render_results() is not None and calls == [1]
    an.image = an.image.astype(np.uint8)
    an.masks_final = [np.asarray(m).astype(np.int32) * 2 for m in an.masks_final]         # values other than 0 / 1
    assert an.render_results() is not None and calls == [1]


def test_predict_on_a_built_model_writes_the_host_statements_pixels(dev, tmp_path, monkeypatch):
    """A MaskRCNN with seeded random weights at the suite's smallest configuration: predict() with draw = True writes out_<id>.png
    from the planes the device path kept; its pixels are the host statement's."""
    import model_cases as T
    from caesar_mrcnn_amd.model import MaskRCNN
    monkeypatch.chdir(tmp_path)
    cfg = T._small_cfg("custom", 128, mode="inference")
    cfg.CLASS_NAMES = list(post.CLASS_NAMES)
    model = MaskRCNN("inference", cfg, str(tmp_path / "logs"), device=dev, weights=T._weights(cfg, 3))
    image = np.clip(T._scene(cfg, 1, 7)[0][0], 0, 255).astype(np.uint8)
    an = analyze.Analyzer(model, cfg)
    an.write_to_json = an.write_to_ds9 = False
    an.score_thr = 0.0                                            # random weights: keep every detection
    an.postprocess_device = True
    an.draw = True
    an.draw_shaded_masks = True
    assert an.predict(image, image_id="scene", bboxes_gt=[[3, 4, 50, 60]]) == 0
    assert len(an.masks_final) >= 1 and an.draw_timing["masks"] == len(an.masks_final) and an.draw_timing["mask_uploads"] == 0
    assert set(an.draw_timing) == {"masks", "mask_uploads", "planes_ms", "render_ms", "download_ms", "encode_ms"}
    pixels, _ = cases.png_pixels((tmp_path / "out_scene.png").read_bytes())
    want = an.render_results(device=False)
    assert want.shape == (7 * 132, 7 * 132, 3) and np.array_equal(pixels, want)
    assert (want[14:-14, 14:-14] != 255).any() and (pixels != np.repeat(np.repeat(np.pad(image, ((2, 2), (2, 2), (0, 0)), constant_values=255), 7, 0), 7, 1)).any()
