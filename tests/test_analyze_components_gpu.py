"""Analyzer.components_device against the host statement, exactly: the true masks of split_gtmasks, the pieces of split_masks and
the islands and minimum-area boxes of compute_det_mask_pars, on the scenes of tests/tester_cases.py and
tests/analyze_post_cases.py and on three of their own; and the fall-back when the labelling refuses a frame."""
import contextlib
import io

import numpy as np
import pytest
import torch

import analyze_post_cases as post
import tester_cases as cases
from caesar_mrcnn_amd import analyze, ops
from caesar_mrcnn_amd.utils import extract_bboxes

pytestmark = pytest.mark.gpu

S65 = cases.S65

# True masks for split_gtmasks: a compact source of three islands (component 1 stands three times in the list) with another compact
# mask touching that component; an `extended` one of two islands, never split (NO_SPLIT_CLASSES_GT); two compact pieces in
# diagonal contact only (not merged); a sidelobe of two islands whose FIRST component touches another sidelobe; an empty mask; a
# galaxy along the last column.
ISLANDS_GT = cases._sc(
    "islands_gt", S65,
    [([(2, 5, 2, 6), (2, 5, 30, 35), (8, 9, 60, 65)], 2, 0), ([(12, 16, 2, 8), (12, 16, 20, 31)], 3, 1), ([(20, 22, 31, 33)], 2, 0),
     ([(22, 24, 33, 40)], 2, 1), ([(28, 30, 0, 4), (36, 40, 60, 65)], 1, 0), ([(30, 33, 2, 9)], 1, 1), ([], 2, 0),
     ([(5, 7, 2, 4)], 2, 1), ([(0, 40, 64, 65)], 6, 0)],
    [([(2, 5, 2, 6)], 2, 0.9), ([(12, 16, 2, 8)], 3, 0.8)], split=True)

# Detections for compute_det_mask_pars: islands in diagonal contact (one island under 8-connectivity), a ring with an island in
# it, a slanted bar (its minimum-area box is not upright), one pixel, one row across the word seams, an empty mask.
_bar = [(10 + k, 11 + k, 20 + 2 * k, 24 + 2 * k) for k in range(12)]
SHAPES_DET = cases._sc(
    "shapes_det", S65, [([(4, 10, 5, 12)], 2, 0)],
    [([(1, 3, 1, 3), (3, 5, 3, 5), (5, 6, 1, 2)], 2, 0.95), ([(24, 25, 2, 14), (25, 33, 2, 3), (25, 33, 13, 14), (33, 34, 2, 14), (28, 30, 6, 9)], 3, 0.9),
     (_bar, 2, 0.85), ([(39, 40, 64, 65)], 1, 0.8), ([(30, 31, 20, 65)], 2, 0.75), ([], 2, 0.72),
     ([(0, 2, 30, 34), (2, 4, 34, 36), (0, 1, 40, 41), (6, 8, 29, 30)], 3, 0.71)])


def _analyzer(sc, components):
    an = analyze.Analyzer(None, cases.cfg(), cases.StubDataset(sc["consider"]), [], [])
    an.eval_device, an.eval_device_min_pairs = True, 0
    an.components_device = components
    return an


def _drive(sc, components, path=None):
    an = _analyzer(sc, components)
    with contextlib.redirect_stdout(io.StringIO()):
        cases.drive(an, sc, extract_bboxes)
        if path is not None:
            an.image_path = path
            assert an.compute_det_mask_pars() == 0
    return an


def _same_arrays(a, b, what):
    assert len(a) == len(b), what
    for k, (x, y) in enumerate(zip(a, b)):
        x, y = np.asarray(x), np.asarray(y)
        assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y), (what, k, x.dtype, y.dtype)


def _assert_same_gt(got, ref, what):
    _same_arrays(got.masks_gt_merged, ref.masks_gt_merged, what + " masks")
    _same_arrays(got.bboxes_gt, ref.bboxes_gt, what + " boxes")
    assert [int(c) for c in got.class_ids_gt_merged] == [int(c) for c in ref.class_ids_gt_merged], what
    assert [type(c) for c in got.class_ids_gt_merged] == [type(c) for c in ref.class_ids_gt_merged], what
    assert got.sidelobes_mixed_or_near_gt_merged == ref.sidelobes_mixed_or_near_gt_merged and got.captions_gt == ref.captions_gt, what


GT_SCENES = [dict(sc, split=True) for sc in cases.scenarios()] + [ISLANDS_GT]


@pytest.mark.parametrize("sc", GT_SCENES, ids=lambda s: s["name"])
def test_extract_gt_masks_device_equals_host(dev, sc):
    got, ref = _drive(sc, True), _drive(sc, False)
    _assert_same_gt(got, ref, sc["name"])
    if sc["gt"]:
        assert "gt_masks_ms" in got.components_timing or got.components_timing.get("gt_entries") == 0
        if got.masks_gt_merged:
            # the merged planes are registered: compute_performances_device did not upload the true masks again
            assert got._eval_planes["gt"][1] is got.masks_gt_merged
            if got.masks_final:
                assert got.eval_timing["mask_uploads"] == 1 and ref.eval_timing["mask_uploads"] == 2
    assert ref.components_timing == {}
    a, b = cases.analyzer_record(got, sc["shape"]), cases.analyzer_record(ref, sc["shape"])
    for k in a:
        assert a[k].shape == b[k].shape and bool(np.all(a[k] == b[k])), (sc["name"], k)


def test_extract_gt_masks_other_dtypes(dev):
    """bool and uint8 true masks: dtypes and values as the host statement leaves them; masks that are no 0 / 1 frames stay on it."""
    for dtype in (bool, np.uint8):
        ans = []
        for components in (True, False):
            an = _analyzer(ISLANDS_GT, components)
            an.class_names = an.class_names_gt = list(cases.CLASS_NAMES)
            an.masks_gt = np.stack([cases.rects(S65, *r, dtype=dtype) for r, _, _ in ISLANDS_GT["gt"]], axis=-1)
            an.class_ids_gt = [c for _, c, _ in ISLANDS_GT["gt"]]
            an.labels_gt = [cases.CLASS_NAMES[c] for c in an.class_ids_gt]
            an.sidelobes_mixed_or_near_gt = [f for _, _, f in ISLANDS_GT["gt"]]
            an.split_gtmasks = True
            an.extract_gt_masks()
            ans.append(an)
        assert "gt_masks_ms" in ans[0].components_timing
        _assert_same_gt(ans[0], ans[1], str(dtype))
    an = _analyzer(ISLANDS_GT, True)
    an.class_names = an.class_names_gt = list(cases.CLASS_NAMES)
    an.masks_gt = 7 * np.stack([cases.rects(S65, *r, dtype=int) for r, _, _ in ISLANDS_GT["gt"][:2]], axis=-1)
    an.class_ids_gt, an.labels_gt, an.sidelobes_mixed_or_near_gt, an.split_gtmasks = [2, 3], ["compact", "extended"], [0, 0], True
    an.extract_gt_masks()
    assert an.components_timing == {} and len(an.masks_gt_merged) == 2


# ---- split_masks ---------------------------------------------------------------------------------------------------------------
class _KeepingModel(post.StubModel):
    """A stand-in that, like MaskRCNN, keeps the device tensor of the masks it returned."""

    def __init__(self, result, dev):
        post.StubModel.__init__(self, result)
        self.last_masks_device = [torch.from_numpy(np.ascontiguousarray(result["masks"]).view(np.uint8)).to(dev)]


def _three_pieces():
    S = (70, 100)
    three = post.rect(S, 5, 15, 5, 15) | post.rect(S, 40, 52, 28, 36) | post.rect(S, 60, 61, 90, 100)     # three islands, one on the seam
    gal = post.rect(S, 55, 65, 5, 15) | post.rect(S, 55, 65, 25, 35)
    diag = post.rect(S, 20, 22, 60, 64) | post.rect(S, 22, 24, 64, 70)                                   # diagonal contact: two pieces
    return ("three_pieces", S, [(three, post.COMPACT, 0.90), (post.rect(S, 42, 54, 30, 40), post.COMPACT, 0.80), (gal, post.GALAXY, 0.85),
                                (diag, post.SPURIOUS, 0.75), (np.zeros(S, bool), post.COMPACT, 0.95), (three, post.COMPACT, 0.60)],
            {"split_masks": True})


SPLIT_SCENES = [(name, shape, objs, dict(settings, split_masks=True)) for name, shape, objs, settings in post.scenarios()] + [_three_pieces()]


@pytest.mark.parametrize("case", SPLIT_SCENES, ids=lambda c: c[0])
def test_split_masks_device_equals_host(dev, case):
    name, shape, objs, settings = case
    result = post.result(shape, objs)

    def run(postprocess, components, keep):
        an = post.analyzer(objs, shape, settings, device=postprocess, model=_KeepingModel(result, dev) if keep else post.StubModel(result))
        an.components_device = components
        return post.run(an, shape)
    ref = run(False, False, False)
    n_above = sum(1 for o in objs if np.float32(o[2]) >= 0.7)
    for keep in (True, False):
        got = run(True, True, keep)
        post.assert_same(got, ref, name)
        assert got.postprocess_timing["masks"] == len(objs)
        assert got.postprocess_timing["mask_uploads"] == (0 if keep or not n_above else 1)          # the kept tensor: no upload at all
        assert ("split_masks_ms" in got.components_timing) == bool(n_above)
    before = run(True, False, True)                                                                # the switch off: as before it existed
    post.assert_same(before, ref, name)
    assert before.components_timing == {} and before.postprocess_timing["mask_uploads"] == (1 if n_above else 0)


def test_split_masks_three_pieces_are_three_detections(dev):
    name, shape, objs, settings = _three_pieces()
    an = post.analyzer(objs, shape, dict(settings, merge_overlapped_masks=False, select_best_overlapped_masks=False), device=True,
                       model=_KeepingModel(post.result(shape, objs), dev))
    an.components_device = True
    post.run(an, shape)
    # in score order: the empty mask gives nothing, `three` its three islands, the galaxy stays whole, the compact square, two pieces
    assert [int(np.asarray(m).sum()) for m in an.masks_final] == [100, 96, 10, 200, 120, 8, 12]
    assert an.components_timing["split_pieces"] == 3 + 1 + 2 + 2 and an.postprocess_timing["mask_uploads"] == 0
    assert [np.asarray(m).dtype for m in an.masks_final] == [analyze.SPLIT_DTYPE] * 3 + [np.dtype(bool)] + [analyze.SPLIT_DTYPE] * 3


# ---- compute_det_mask_pars -------------------------------------------------------------------------------------------------------
def _scene_image(shape, path):
    from caesar_mrcnn_amd import fits
    rng = np.random.default_rng(shape[0] + shape[1])
    img = (rng.normal(size=shape) * 10 ** rng.uniform(-4, 0, size=shape)).astype(np.float32)
    fits.write_fits(path, img)


@pytest.mark.parametrize("sc", cases.scenarios() + [SHAPES_DET], ids=lambda s: s["name"])
def test_det_mask_pars_device_equals_host(dev, sc, tmp_path):
    path = str(tmp_path / "img.fits")
    _scene_image(sc["shape"], path)
    got, ref = _drive(sc, True, path), _drive(sc, False, path)
    assert len(got.det_obj_pars) == len(ref.det_obj_pars) == len(sc["dets"])
    for a, b in zip(got.det_obj_pars, ref.det_obj_pars):
        assert a == b and [type(a[k]) for k in sorted(a)] == [type(b[k]) for k in sorted(b)], (sc["name"], a, b)
    on_device = len(ref.masks_gt_merged) * len(ref.masks_final) > 0
    assert (got.components_timing.get("det_mask_shape_downloads") == 1) == on_device            # one download for all the integers
    assert "det_mask_shape_downloads" not in ref.components_timing
    if sc is SHAPES_DET:
        assert [p.get("nislands") for p in ref.det_obj_pars] == [2, 2, 1, 1, 1, None, 3] and ref.det_obj_pars[5] == {}
        # the pure host statement (count_islands, min_area_rect on full frames) says the same
        host = _analyzer(sc, False)
        host.eval_device = False
        with contextlib.redirect_stdout(io.StringIO()):
            cases.drive(host, sc, extract_bboxes)
            host.image_path = path
            assert host.compute_det_mask_pars() == 0
        for a, b in zip(got.det_obj_pars, host.det_obj_pars):
            assert {k: v for k, v in a.items() if k not in ("Stot", "snr")} == {k: v for k, v in b.items() if k not in ("Stot", "snr")}


def test_det_mask_pars_with_boxes_that_are_not_the_planes(dev, tmp_path):
    """self.bboxes sizes the workspace; when they are not the boxes of masks_final the work is done again from the planes' own."""
    path = str(tmp_path / "img.fits")
    _scene_image(SHAPES_DET["shape"], path)
    ref = _drive(SHAPES_DET, False, path)
    an = _analyzer(SHAPES_DET, True)
    with contextlib.redirect_stdout(io.StringIO()):
        cases.drive(an, SHAPES_DET, extract_bboxes)
        an.image_path = path
        an.bboxes = [np.array([0, 0, 3, 3], np.int32)] * len(an.masks_final)
        assert an.compute_det_mask_pars() == 0
    assert an.det_obj_pars == ref.det_obj_pars and an.components_timing["det_mask_shape_downloads"] == 2


# ---- the labelling refuses: the host statement takes the call -------------------------------------------------------------
def _refusing(monkeypatch, calls):
    def refuse(*a, **k):
        calls.append(1)
        raise ops.ComponentsUnsupported("planted refusal")
    monkeypatch.setattr(ops, "mask_components", refuse)


def test_refusal_falls_back_to_the_host_statement(dev, monkeypatch, caplog, tmp_path):
    monkeypatch.setattr(analyze, "device_forms_failed", set())
    path = str(tmp_path / "img.fits")
    _scene_image(S65, path)
    want_gt, want_pars = _drive(ISLANDS_GT, False), _drive(SHAPES_DET, False, path)
    name, shape, objs, settings = _three_pieces()
    want_split = post.run(post.analyzer(objs, shape, settings, device=False), shape)
    calls = []
    _refusing(monkeypatch, calls)
    with caplog.at_level("DEBUG", logger="mrcnn"):
        for what, call, check in (
                ("gt", lambda: _drive(ISLANDS_GT, True), lambda an: _assert_same_gt(an, want_gt, "refused")),
                ("pars", lambda: _drive(SHAPES_DET, True, path), lambda an: an.det_obj_pars == want_pars.det_obj_pars or pytest.fail("pars")),
                ("split", lambda: post.run(_split_analyzer(objs, shape, settings, dev), shape), lambda an: post.assert_same(an, want_split, "refused"))):
            caplog.clear()
            del calls[:]
            check(call())
            said = [r.getMessage() for r in caplog.records if "planted refusal" in r.getMessage()]
            assert calls == [1] and len(said) == 1 and said[0].endswith("the host statement takes this call"), (what, said)
    assert analyze.device_forms_failed == set()                                   # a refusal is no failure: the next frame tries again


def _split_analyzer(objs, shape, settings, dev):
    an = post.analyzer(objs, shape, settings, device=True, model=_KeepingModel(post.result(shape, objs), dev))
    an.components_device = True
    return an
