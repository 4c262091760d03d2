"""Planted detection sets for Analyzer.extract_det_masks (host statement against the bit-plane path), shared by
tests/test_analyze_post_cpu.py and tests/test_analyze_post_gpu.py.  A stand-in model returns fixed rois / class_ids / scores /
masks, as in tests/test_analyze_cpu.py.  Frames are at most 132 x 132 and hold at most 24 masks; their widths are no multiple
of 32 and the planted objects straddle the word boundaries x = 31 | 32 and 63 | 64."""
import numpy as np

CLASS_NAMES = ["bkg", "spurious", "compact", "galaxy"]           # 'galaxy' is never split (analyze.NO_SPLIT_CLASSES)
SPURIOUS, COMPACT, GALAXY = 1, 2, 3


class StubModel(object):
    def __init__(self, result):
        self.result = result

    def detect(self, images, verbose=0):
        return [self.result]


def cfg():
    from caesar_mrcnn_amd.config import run_py_config
    c = run_py_config(num_classes=4, imgsize=64, mode="inference")
    c.CLASS_NAMES = list(CLASS_NAMES)
    return c


def rect(shape, y1, y2, x1, x2):
    m = np.zeros(shape, bool)
    m[y1:y2, x1:x2] = True
    return m


def result(shape, objs):
    """objs: [(bool mask, class id, score)] -> the dict MaskRCNN.detect returns for one image."""
    n = len(objs)
    masks = np.zeros(tuple(shape) + (n,), bool)
    rois = np.zeros((n, 4), np.int32)
    for i, (m, _, _) in enumerate(objs):
        masks[:, :, i] = m
        ys, xs = np.nonzero(m)
        if ys.size:
            rois[i] = (ys.min(), xs.min(), ys.max() + 1, xs.max() + 1)
    return {"rois": rois, "masks": masks, "class_ids": np.array([o[1] for o in objs], np.int32),
            "scores": np.array([o[2] for o in objs], np.float32)}


def _disc(shape, cy, cx, r):
    yy, xx = np.mgrid[0:shape[0], 0:shape[1]]
    return (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r


def discs(shape, n, seed, rmin=2, rmax=12):
    """The generator of tools/analyze_bench.py: n discs of radius rmin .. rmax with random centres, classes and scores >= 0.7."""
    rng = np.random.default_rng(seed)
    objs = []
    for _ in range(n):
        r = int(rng.integers(rmin, rmax + 1))
        cy, cx = int(rng.integers(0, shape[0])), int(rng.integers(0, shape[1]))
        objs.append((_disc(shape, cy, cx, r), int(rng.integers(1, len(CLASS_NAMES))), float(rng.uniform(0.7, 1.0))))
    return objs


def scenarios():
    """[(name, frame shape, objs, Analyzer settings)]"""
    S = (70, 100)
    out = []
    # A-B and B-C overlap with IoU 240 / 560, A-C with 80 / 720 < 0.3: one component through B; D stands alone
    chain = [(rect(S, 10, 30, 20, 40), COMPACT, 0.95), (rect(S, 10, 30, 28, 48), COMPACT, 0.90), (rect(S, 10, 30, 36, 56), COMPACT, 0.85),
             (rect(S, 50, 60, 60, 70), COMPACT, 0.80)]
    out.append(("chain_of_three", S, chain, {}))
    # same class, IoU 80 / 720: not merged, but connected -> the better one is selected
    out.append(("same_class_below_iou_thr", S, [(rect(S, 10, 30, 20, 40), COMPACT, 0.90), (rect(S, 10, 30, 36, 56), COMPACT, 0.95)], {}))
    # other classes sharing an edge across x = 63 | 64 (touch, no overlap); a pair in diagonal-only contact at (39, 31) / (40, 32)
    touch = [(rect(S, 5, 15, 50, 64), COMPACT, 0.90), (rect(S, 5, 15, 64, 80), GALAXY, 0.80),
             (rect(S, 30, 40, 20, 32), COMPACT, 0.75), (rect(S, 40, 50, 32, 44), GALAXY, 0.85)]
    out.append(("other_classes_touch_and_diagonal", S, touch, {}))
    # four squares around (32, 32), every pair overlapping: IoU 120 / 680 (side by side) or 36 / 764 (diagonal) -> one clique of four
    four = [(rect(S, 10, 30, 10, 30), COMPACT, 0.81), (rect(S, 10, 30, 24, 44), COMPACT, 0.93), (rect(S, 24, 44, 10, 30), GALAXY, 0.77),
            (rect(S, 24, 44, 24, 44), GALAXY, 0.88)]
    out.append(("clique_of_four", S, four, {}))
    # A | B | C in a row: cliques {A, B} and {B, C}; A beats B, and B -- although dropped -- still beats C
    shared = [(rect(S, 20, 30, 10, 31), COMPACT, 0.95), (rect(S, 20, 30, 31, 33), GALAXY, 0.90), (rect(S, 20, 30, 33, 50), COMPACT, 0.80)]
    out.append(("two_cliques_sharing_a_member", S, shared, {}))
    # spurious against compact: IoU 80 / 720 < 0.3 (both kept) and 280 / 520 >= 0.3 (the better one kept)
    spur = [(rect(S, 5, 25, 20, 40), SPURIOUS, 0.90), (rect(S, 5, 25, 36, 56), COMPACT, 0.85),
            (rect(S, 40, 60, 50, 70), SPURIOUS, 0.80), (rect(S, 40, 60, 56, 76), COMPACT, 0.97)]
    out.append(("spurious_below_and_above_thr", S, spur, {}))
    out.append(("spurious_rule_off", S, spur, {"split_source_sidelobe": False}))
    # threshold 0: 0.0 < 0.0 is false, so touching alone merges same-class masks, and the spurious rule never fires
    out.append(("iou_thr_zero", S, [(rect(S, 5, 15, 50, 64), COMPACT, 0.90), (rect(S, 5, 15, 64, 80), COMPACT, 0.80),
                                    (rect(S, 16, 20, 80, 90), COMPACT, 0.75), spur[2], (rect(S, 40, 60, 66, 86), COMPACT, 0.78)],
                {"merge_overlap_iou_thr": 0.0}))
    # split_masks: a compact mask of two islands (one of them overlapping another compact mask), a galaxy of two islands (kept whole)
    two = rect(S, 5, 15, 5, 15) | rect(S, 40, 52, 60, 72)
    gal = rect(S, 55, 65, 5, 15) | rect(S, 55, 65, 25, 35)
    out.append(("split_two_islands", S, [(two, COMPACT, 0.90), (rect(S, 42, 54, 62, 74), COMPACT, 0.80), (gal, GALAXY, 0.85)],
                {"split_masks": True}))
    mixed = chain + touch[2:] + [(rect(S, 45, 65, 5, 25), GALAXY, 0.91), (rect(S, 50, 62, 15, 40), SPURIOUS, 0.72)]
    out.append(("merge_off", S, mixed, {"merge_overlapped_masks": False}))
    out.append(("select_off", S, mixed, {"select_best_overlapped_masks": False}))
    out.append(("merge_and_select_off", S, mixed, {"merge_overlapped_masks": False, "select_best_overlapped_masks": False}))
    # a mask of one row and a mask without pixels (its box is all zero: the invalid-box skip), next to an ordinary one
    out.append(("one_row_and_empty", S, [(rect(S, 69, 70, 3, 99), COMPACT, 0.90), (np.zeros(S, bool), GALAXY, 0.95),
                                         (rect(S, 0, 8, 90, 100), COMPACT, 0.80)], {}))
    out.append(("nothing_above_score_thr", S, [(rect(S, 5, 15, 5, 15), COMPACT, 0.50), (rect(S, 5, 15, 10, 20), COMPACT, 0.69)], {}))
    out.append(("one_detection", S, [(rect(S, 0, 70, 0, 100), GALAXY, 0.99)], {}))
    out.append(("one_pixel_frame", (1, 1), [(np.ones((1, 1), bool), COMPACT, 0.90), (np.ones((1, 1), bool), GALAXY, 0.80)], {}))
    out.append(("discs_24", (132, 132), discs((132, 132), 24, 3), {}))
    out.append(("discs_24_split", (131, 97), discs((131, 97), 24, 4, rmin=1, rmax=9), {"split_masks": True}))
    return out


# What extract_det_masks costs per scenario, recorded from the code before its two forms shared one decision body: the calls of
# mask_iou and are_mask_connected the host statement makes (its short-circuits decide them), and the calls of ops.mask_planes_pack,
# mask_pair_stats and mask_union the device form makes (pair_stats is called for an empty pair list too, without a launch).
PIXEL_WORK = {
    "chain_of_three":                    (6, 3, 1, 2, 1),
    "same_class_below_iou_thr":          (1, 1, 1, 2, 1),
    "other_classes_touch_and_diagonal":  (2, 6, 1, 2, 1),
    "clique_of_four":                    (2, 6, 1, 2, 1),
    "two_cliques_sharing_a_member":      (1, 3, 1, 2, 1),
    "spurious_below_and_above_thr":      (4, 6, 1, 2, 1),
    "spurious_rule_off":                 (2, 6, 1, 2, 1),
    "iou_thr_zero":                      (7, 12, 1, 2, 1),
    "split_two_islands":                 (3, 4, 1, 2, 1),
    "merge_off":                         (2, 28, 1, 1, 1),
    "select_off":                        (11, 2, 1, 1, 1),
    "merge_and_select_off":              (0, 0, 1, 0, 1),
    "one_row_and_empty":                 (1, 3, 1, 2, 1),
    "nothing_above_score_thr":           (0, 0, 0, 0, 0),
    "one_detection":                     (0, 0, 1, 2, 1),
    "one_pixel_frame":                   (0, 1, 1, 2, 1),
    "discs_24":                          (94, 276, 1, 2, 1),
    "discs_24_split":                    (89, 254, 1, 2, 1),
}


def counted(monkeypatch, owner, name, calls):
    """Count the calls of owner.name in calls[name]; the function itself still runs."""
    real = getattr(owner, name)
    calls[name] = 0

    def wrapped(*a, **k):
        calls[name] += 1
        return real(*a, **k)
    monkeypatch.setattr(owner, name, wrapped)


def planted_failure(entered):
    def broken(*a, **k):
        from caesar_mrcnn_amd import _hip
        entered.append(1)
        raise _hip.HipPathError("planted")
    return broken


def check_failure_policy(monkeypatch, caplog, name, break_device_form, call, want, same=lambda a, b: a == b):
    """The policy of analyze.device_or_host as one of its users shows it.  break_device_form(entered) makes the device form
    called `name` append 1 to `entered` and raise _hip.HipPathError("planted"); call() goes through the dispatcher, eligible for
    the device, and returns what same(got, want) compares; `want` is the host statement's result."""
    from caesar_mrcnn_amd import analyze
    monkeypatch.setattr(analyze, "device_forms_failed", set())
    entered = []
    break_device_form(entered)
    with caplog.at_level("ERROR", logger="mrcnn"):
        caplog.clear()
        assert same(call(), want) and entered == [1]               # the device form raised: the host statement's result
        assert same(call(), want) and entered == [1]               # not entered again
        said = [r.getMessage() for r in caplog.records if r.levelname == "ERROR"]
    assert len(said) == 1 and said[0].startswith(name + " failed (HipPathError: planted): this and every later call take the host statement")
    assert analyze.device_forms_failed == {name}
    analyze.device_forms_failed.clear()
    assert same(call(), want) and entered == [1, 1]                 # forgotten: entered again


def analyzer(objs, shape, settings, device, model=None):
    from caesar_mrcnn_amd import analyze
    an = analyze.Analyzer(model or StubModel(result(shape, objs)), cfg())
    an.write_to_json = an.write_to_ds9 = False
    for k, v in settings.items():
        setattr(an, k, v)
    an.postprocess_device = device
    return an


def run(an, shape):
    assert an.predict(np.zeros(tuple(shape) + (3,), np.uint8), image_id="img", xmin=7, ymin=11) == 0
    return an


def assert_same(got, ref, tag=""):
    """Everything extract_det_masks leaves behind, and what make_json_results / make_ds9_regions make of it: exact."""
    assert len(got.masks_final) == len(ref.masks_final), tag
    for k, (a, b) in enumerate(zip(got.masks_final, ref.masks_final)):
        a, b = np.asarray(a), np.asarray(b)
        assert a.dtype == b.dtype and a.shape == b.shape, (tag, k, a.dtype, b.dtype, a.shape, b.shape)
        assert np.array_equal(a, b), (tag, k)
    assert [int(c) for c in got.class_ids_final] == [int(c) for c in ref.class_ids_final], tag
    assert got.class_names_final == ref.class_names_final, tag
    assert len(got.scores_final) == len(ref.scores_final), tag
    for a, b in zip(got.scores_final, ref.scores_final):
        assert type(a) is type(b) and a == b, (tag, a, b)
    assert len(got.bboxes) == len(ref.bboxes), tag
    for a, b in zip(got.bboxes, ref.bboxes):
        assert np.asarray(a).dtype == np.asarray(b).dtype and np.array_equal(a, b), (tag, a, b)
    assert got.captions == ref.captions, tag
    assert got.results == ref.results, tag
    assert got.obj_regions == ref.obj_regions, tag
