"""The statements behind the bit-plane post-processing (csrc/maskgraph.hip), without a GPU: the 4-neighbour predicate equals
Analyzer.are_mask_connected, the plane layout round-trips, extract_det_masks dispatches to the host statement, and
extract_det_masks_device -- with NumPy stand-ins for the three kernels -- takes the host statement's decisions on the planted
scenarios of tests/analyze_post_cases.py."""
import numpy as np
import pytest

import caesar_mrcnn_amd  # noqa: F401
from caesar_mrcnn_amd import analyze

import analyze_post_cases as cases


def _an():
    return analyze.Analyzer(None, cases.cfg())


def test_masks_touch4_equals_are_mask_connected_random():
    """2400 seeded pairs on frames of 1 .. 12 px at densities 0.02 .. 0.6; each answer must occur at least 300 times, or the
    generator would not cover it."""
    rng = np.random.default_rng(20)
    an = _an()
    n_true = 0
    for _ in range(2400):
        h, w = int(rng.integers(1, 13)), int(rng.integers(1, 13))
        m1 = (rng.uniform(size=(h, w)) < rng.uniform(0.02, 0.6)).astype(np.uint8)
        m2 = (rng.uniform(size=(h, w)) < rng.uniform(0.02, 0.6)).astype(np.uint8)
        ref = an.are_mask_connected(m1, m2)
        assert analyze.masks_touch4(m1, m2) == ref and analyze.masks_touch4(m2, m1) == ref, (m1, m2)
        n_true += bool(ref)
    assert 300 <= n_true <= 2100, n_true


def test_masks_touch4_constructed_pairs():
    an = _an()

    def px(shape, *pts):
        m = np.zeros(shape, np.uint8)
        for y, x in pts:
            m[y, x] = 1
        return m
    S = (5, 6)
    pairs = [
        (px(S, (1, 1)), px(S, (2, 2)), False),                    # diagonal only
        (px(S, (1, 1), (3, 3)), px(S, (2, 2)), False),            # diagonal on two sides
        (px(S, (1, 1)), px(S, (0, 2)), False),                    # the other diagonal
        (px(S, (1, 1)), px(S, (2, 1)), True),                     # vertical only
        (px(S, (1, 1)), px(S, (1, 2)), True),                     # horizontal only
        (px(S, (1, 1), (1, 2)), px(S, (1, 2), (4, 5)), True),     # overlap
        (px(S, (1, 1)), px(S, (1, 3)), False),                    # distance 2
        (px(S, (0, 0)), px(S, (4, 5)), False),
        (px(S, (0, 0)), px(S), False),                            # one empty
        (px(S), px(S), False),                                    # both empty
        (np.ones((1, 1), np.uint8), np.ones((1, 1), np.uint8), True),
        (np.ones((1, 1), np.uint8), np.zeros((1, 1), np.uint8), False),
        (np.zeros((1, 1), np.uint8), np.zeros((1, 1), np.uint8), False),
        (px((1, 4), (0, 0)), px((1, 4), (0, 1)), True),           # one row
        (px((4, 1), (0, 0)), px((4, 1), (2, 0)), False),          # one column, distance 2
    ]
    for m1, m2, want in pairs:
        assert an.are_mask_connected(m1, m2) == want, (m1, m2)
        assert analyze.masks_touch4(m1, m2) == want and analyze.masks_touch4(m2, m1) == want, (m1, m2)
        assert analyze.masks_touch4(m1.astype(bool), m2 * 255) == want


@pytest.mark.parametrize("W", [1, 31, 32, 33, 64, 65])
def test_plane_layout_round_trip(W):
    rng = np.random.default_rng(W)
    H, n = 5, 3
    masks = rng.uniform(size=(H, W, n)) < 0.5
    masks[0, 0, 0] = masks[H - 1, W - 1, 0] = True
    masks[:, :, 2] = True                                       # a full plane: the pad bits must still be zero
    planes = analyze.pack_mask_planes(masks * np.uint8(255))
    wpr = (W + 31) // 32
    assert planes.shape == (n, H, wpr) and planes.dtype == np.dtype("<u4")
    for d in range(n):
        for y in range(H):
            for x in range(W):
                assert bool((int(planes[d, y, x >> 5]) >> (x & 31)) & 1) == bool(masks[y, x, d])
    if W % 32:
        assert not np.any(planes[:, :, -1] >> np.uint32(W % 32))
    assert int(sum(bin(int(v)).count("1") for v in planes[2].ravel())) == H * W
    back = analyze.unpack_mask_planes(planes, W)
    assert back.shape == (n, H, W) and back.dtype == np.uint8
    assert np.array_equal(back, np.moveaxis(masks, -1, 0).astype(np.uint8))
    assert np.array_equal(analyze.unpack_mask_planes(planes.view(np.int32), W), back)      # the device tensors are int32 views


@pytest.mark.parametrize("case", cases.scenarios(), ids=lambda c: c[0])
def test_dispatch_without_device_is_the_host_statement(case):
    name, shape, objs, settings = case
    via = cases.run(cases.analyzer(objs, shape, settings, device=False), shape)
    assert via.postprocess_timing == {}                         # the device path was not entered
    ref = cases.analyzer(objs, shape, settings, device=False)
    ref.extract_det_masks = ref.extract_det_masks_host
    cases.run(ref, shape)
    cases.assert_same(via, ref, name)


def test_planted_scenarios_do_what_they_are_named_for():
    """A check of the fixtures, not of the device path: under the host statement the planted scenarios produce the outcomes the
    device comparison is meant to cover."""
    got = {}
    for name, shape, objs, settings in cases.scenarios():
        an = cases.run(cases.analyzer(objs, shape, settings, device=False), shape)
        got[name] = ([int(np.asarray(m).sum()) for m in an.masks_final], list(an.class_names_final), [str(np.asarray(m).dtype) for m in an.masks_final])
    assert got["chain_of_three"][0] == [20 * 36, 100]
    assert got["same_class_below_iou_thr"][0] == [400]
    assert got["other_classes_touch_and_diagonal"][0] == [140, 120, 120]          # the diagonal pair survives whole
    assert got["clique_of_four"][0] == [400]
    assert got["two_cliques_sharing_a_member"][0] == [210]
    assert got["spurious_below_and_above_thr"][1] == ["compact", "spurious", "compact"]      # by score: 0.97, 0.90, 0.85
    assert got["spurious_rule_off"][1] == ["compact", "spurious"]
    assert got["iou_thr_zero"][:2] == ([140 + 160, 400, 40], ["compact", "spurious", "compact"])
    assert got["split_two_islands"][2] == ["int64", "int64", "bool"] and got["split_two_islands"][0] == [100, 144 + 144 - 100, 200]
    assert len(got["merge_off"][0]) < len(got["merge_and_select_off"][0]) == 8
    assert got["one_row_and_empty"][0] == [96, 80]
    assert got["nothing_above_score_thr"][0] == [] and got["one_detection"][0] == [7000] and got["one_pixel_frame"][0] == [1]


# ---- the device path's host half, with NumPy in place of the kernels ------------------------------------------------------------
def _numpy_ops(monkeypatch):
    """ops.mask_planes_pack / mask_pair_stats / mask_union restated on CPU tensors (the contract of include/mrcnn_hip.h)."""
    import torch
    from caesar_mrcnn_amd import ops
    from caesar_mrcnn_amd.utils import extract_bboxes

    def planes_of(m, W):                                        # m [n, H, W] bool
        words = analyze.pack_mask_planes(np.moveaxis(m, 0, -1))
        count = m.reshape(m.shape[0], -1).sum(1).astype(np.int32)
        box = extract_bboxes(np.moveaxis(m, 0, -1)).astype(np.int32).reshape(-1, 4)
        p = ops.MaskPlanes(torch.from_numpy(words.view(np.int32)), torch.from_numpy(count), torch.from_numpy(box), W)
        p._m = m
        return p

    def pack(masks):
        a = masks.numpy()
        return planes_of(np.moveaxis(a, -1, 0) != 0, a.shape[1])

    def pair_stats(planes, pairs):
        pairs = np.asarray(pairs).reshape(-1, 2)
        inter = [int((planes._m[i] & planes._m[j]).sum()) for i, j in pairs]
        touch = [int(analyze.masks_touch4(planes._m[i], planes._m[j])) for i, j in pairs]
        return torch.tensor(inter, dtype=torch.int32), torch.tensor(touch, dtype=torch.int32)

    def union(planes, comp_offsets, member_ids):
        m = np.zeros((len(comp_offsets) - 1,) + planes._m.shape[1:], bool)
        for c in range(m.shape[0]):
            for q in range(comp_offsets[c], comp_offsets[c + 1]):
                m[c] |= planes._m[member_ids[q]]
        return planes_of(m, planes.W)
    monkeypatch.setattr(ops, "mask_planes_pack", pack)
    monkeypatch.setattr(ops, "mask_pair_stats", pair_stats)
    monkeypatch.setattr(ops, "mask_union", union)


@pytest.mark.parametrize("case", cases.scenarios(), ids=lambda c: c[0])
def test_device_path_host_half_with_numpy_kernels(case, monkeypatch):
    import torch
    name, shape, objs, settings = case
    _numpy_ops(monkeypatch)
    got = cases.analyzer(objs, shape, settings, device=True)
    got._device = lambda: torch.device("cpu")
    cases.run(got, shape)
    assert got.postprocess_timing["masks"] == len(objs)         # the device path ran
    ref = cases.run(cases.analyzer(objs, shape, settings, device=False), shape)
    cases.assert_same(got, ref, name)


@pytest.mark.parametrize("case", cases.scenarios(), ids=lambda c: c[0])
def test_both_forms_do_the_pixel_work_they_did(case, monkeypatch):
    """One decision body serves both forms; neither may pay for it.  The host statement makes exactly the mask_iou and
    are_mask_connected calls it made before (it asks pair by pair, under its short-circuits), the device form exactly the
    pack / pair_stats / union calls (one per phase): cases.PIXEL_WORK."""
    import torch
    from caesar_mrcnn_amd import ops
    name, shape, objs, settings = case
    calls = {}
    cases.counted(monkeypatch, analyze, "mask_iou", calls)
    cases.counted(monkeypatch, analyze.Analyzer, "are_mask_connected", calls)
    an = cases.analyzer(objs, shape, settings, device=False)
    an.masks, an.boxes, an.class_ids, an.scores = (an.model.result[k] for k in ("masks", "rois", "class_ids", "scores"))
    an.extract_det_masks_host()
    assert (calls["mask_iou"], calls["are_mask_connected"]) == cases.PIXEL_WORK[name][:2]
    _numpy_ops(monkeypatch)
    for k in ("mask_planes_pack", "mask_pair_stats", "mask_union"):
        cases.counted(monkeypatch, ops, k, calls)
    an._device = lambda: torch.device("cpu")
    an.extract_det_masks_device()
    assert (calls["mask_planes_pack"], calls["mask_pair_stats"], calls["mask_union"]) == cases.PIXEL_WORK[name][2:]
    assert (calls["mask_iou"], calls["are_mask_connected"]) == cases.PIXEL_WORK[name][:2]          # none of the host's


def test_failed_device_form_is_left_for_the_process(monkeypatch, caplog):
    name, shape, objs, settings = cases.scenarios()[0]
    ref = cases.run(cases.analyzer(objs, shape, settings, device=False), shape)
    an = cases.analyzer(objs, shape, settings, device=True)

    def same(got, want):
        cases.assert_same(got, want, name)
        return True
    cases.check_failure_policy(monkeypatch, caplog, "extract_det_masks_device",
                               lambda entered: monkeypatch.setattr(analyze.Analyzer, "extract_det_masks_device", cases.planted_failure(entered)),
                               lambda: cases.run(an, shape), ref, same)


def test_one_device_resolution(monkeypatch):
    """Analyzer and SFinder ask the same two functions, which read the engine's `dev`; without a model, torch's current device."""
    import torch
    from caesar_mrcnn_amd import sfinder

    class Engine(object):
        dev = torch.device("cpu")

    class Model(object):
        engine = Engine()
    cfg = cases.cfg()
    cfg.IMG_PATH = "none.fits"
    an, sf = analyze.Analyzer(Model(), cfg), sfinder.SFinder(Model(), cfg)
    assert an._device() is Engine.dev and sf._device() is Engine.dev and analyze.model_device(Model()) is Engine.dev
    assert analyze.Analyzer.has_gpu(an.model) is False and sf._has_gpu() is False and analyze.model_has_gpu(Model()) is False
    assert sf.merge_device is False and sf.params_device is False and an.eval_device is False
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 3)
    for there in (True, False):
        monkeypatch.setattr(torch.cuda, "is_available", lambda: there)
        an, sf = analyze.Analyzer(None, cfg), sfinder.SFinder(None, cfg)
        assert an._device() == sf._device() == analyze.model_device(None) == torch.device("cuda", 3)
        assert analyze.Analyzer.has_gpu(None) is sf._has_gpu() is analyze.model_has_gpu(None) is there
        assert sf.merge_device is there and sf.params_device is there and an.eval_device is there


def test_values_other_than_0_1_take_the_host_path():
    """A lone mask is handed on as it came, so masks that are not bool and hold other values than 0 / 1 cannot go through
    bit planes."""
    S = (20, 40)
    res = cases.result(S, [(cases.rect(S, 2, 8, 2, 8), cases.COMPACT, 0.9)])
    res["masks"] = res["masks"].astype(np.uint8) * 7
    an = analyze.Analyzer(cases.StubModel(res), cases.cfg())
    an.write_to_json = an.write_to_ds9 = False
    an.postprocess_device = True
    cases.run(an, S)
    assert an.postprocess_timing == {} and int(an.masks_final[0].max()) == 7
