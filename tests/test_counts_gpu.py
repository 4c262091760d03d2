"""The data-dependent counts of csrc/losses.hip, csrc/targets.hip and csrc/detection.hip at their empty sides, boundaries and caps,
against the CPU oracle: more than one register group of anchors in the RPN loss, no positive anchor / ROI / active class, fewer
target rows than positives, a reused workspace; 0 .. quota positives, scarce negatives, no GT, non-contiguous GT rows, R and G at
their caps in the detection targets; 0, 1, 63, 64, 65 ... candidates, R = 1 and R = DET_CAP in the detection layer.
The seeded inputs and their oracle-side preconditions are in tests/model_cases.py; tests/test_host_cpu.py runs the preconditions
and the two reference perturbations (rank carry, compacted mask plane) without a GPU."""
import numpy as np
import pytest
import torch

import model_cases as M

pytestmark = pytest.mark.gpu


def _ops():
    from caesar_mrcnn_amd import ops
    return ops


def _loss_cfg(dice):
    from caesar_mrcnn_amd.config import run_py_config
    cfg = run_py_config(num_classes=4)
    cfg.MASK_LOSS_FUNCTION = "dice_coef_loss" if dice else "binary_crossentropy"
    return cfg


def _run_losses(dev, d, dice):
    """ops.losses_fwd_bwd on the NumPy operands d -> (losses[5], {name: gradient}) as NumPy."""
    D = lambda a: torch.tensor(np.ascontiguousarray(a), device=dev)
    out = _ops().losses_fwd_bwd(D(d["rpn_match"]), D(d["rpn_bbox_t"]), D(d["rpn_logits"]), D(d["rpn_bbox"]), D(d["tcls"]), D(d["tbbox"]),
                                D(d["tmask"]), D(d["active"][0].copy()), D(d["logits"]), D(d["mbbox"]), D(d["mmask"]), M.LOSS_WEIGHTS, dice)
    torch.cuda.synchronize()
    return out[0].cpu().numpy(), {n: g.cpu().numpy() for n, g in zip(M.LOSS_GRADS, out[1:])}


def _report(tag, got, ref):
    fl, fg = M.tolerance_fractions(got[0], got[1], ref[0], ref[1])
    print("[%s] worst fraction of the tolerance: losses %.3g, gradients %.3g" % (tag, fl, fg))


# ---- 1. losses ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A", M.RANK_CASE_ANCHORS)
def test_losses_rank_across_groups(dev, A):
    """A = 33 797 (two register groups of 32 768 anchors, ragged last slice) and A = 98 309 (four, the last of 5 anchors): the rank of a positive anchor
    is carried from group to group.  Positives sit on both sides of every group edge and on the last anchor; image 0 has an empty
    first group, image 1 an empty last one.  Losses, gradients at the tolerances of test_losses; d_rpn_bbox is non-zero exactly on
    the positive anchors."""
    d = M.losses_rank_inputs(A)
    per_group = M.rank_case_group_positives(d)
    assert per_group.shape[1] == -(-A // M.LOSS_GROUP) and (per_group.sum(0) > 0).all()
    assert per_group[0, 0] == 0 and per_group[1, -1] == 0 and (per_group[0, 1:] > 0).all() and (per_group[1, :-1] > 0).all()
    ref = M.losses_reference(_loss_cfg(False), d)
    got = _run_losses(dev, d, False)
    _report("losses A=%d" % A, got, ref)
    assert np.isfinite(got[0]).all() and all(np.isfinite(g).all() for g in got[1].values())
    M.assert_losses_close(got[0], got[1], ref[0], ref[1])
    pos = d["rpn_match"][:, :, 0] == 1
    assert (got[1]["rpn_bbox"][pos] != 0).all() and (got[1]["rpn_bbox"][~pos] == 0).all()
    assert (ref[1]["rpn_bbox"][pos] != 0).all()


@pytest.mark.parametrize("dice", [False, True])
@pytest.mark.parametrize("case", M.EMPTY_SIDE_CASES)
def test_losses_empty_sides(dev, case, dice):
    """One side of the losses empty (model_cases.losses_empty_inputs): the loss of an empty side and its gradient are exactly 0,
    everything else matches the oracle at the tolerances of test_losses; with no active class the class loss and its gradient are
    NaN on both sides (0 / 0, as in the reference) and the other four finite."""
    d = M.losses_empty_inputs(case)
    ref = M.losses_reference(_loss_cfg(dice), d)
    got = _run_losses(dev, d, dice)
    _report("losses empty side %s dice=%s" % (case, dice), got, ref)
    ls, g = got
    npos_a = int((d["rpn_match"] == 1).sum()); nnon = int((d["rpn_match"] != 0).sum()); npos_r = int((d["tcls"] > 0).sum())
    if case == "g":
        assert d["active"].sum() == 0
        assert np.isnan(ls[2]) and np.isnan(ref[0][2]) and np.isnan(g["logits"]).all() and np.isnan(ref[1]["logits"]).all()
        assert np.isfinite(ls[[0, 1, 3, 4]]).all() and all(np.isfinite(g[n]).all() for n in M.LOSS_GRADS if n != "logits")
        M.assert_losses_close(ls, g, ref[0], ref[1], names=[n for n in M.LOSS_GRADS if n != "logits"], which=[0, 1, 3, 4])
        return
    assert np.isfinite(ls).all() and all(np.isfinite(v).all() for v in g.values())
    M.assert_losses_close(ls, g, ref[0], ref[1])
    if case == "a":
        assert npos_a == 0 and nnon > 0
        assert ls[1] == 0 and (g["rpn_bbox"] == 0).all() and ls[0] > 0
    elif case == "b":
        assert nnon == 0
        assert ls[0] == 0 and ls[1] == 0 and (g["rpn_logits"] == 0).all() and (g["rpn_bbox"] == 0).all()
    elif case == "c":
        assert (d["rpn_match"][1] == 0).all() and (d["rpn_match"][0] == 1).sum() > 0
        assert (g["rpn_logits"][1] == 0).all() and (g["rpn_bbox"][1] == 0).all() and ls[0] > 0 and ls[1] > 0
    elif case == "d":
        assert npos_r == 0
        assert ls[3] == 0 and ls[4] == 0 and (g["mbbox"] == 0).all() and (g["mmask"] == 0).all() and ls[2] > 0
    elif case == "e":
        assert npos_r == 1 and d["tcls"][-1, -1] > 0
        assert ls[3] > 0 and ls[4] > 0 and (g["mbbox"][:, :-1] == 0).all() and (g["mbbox"][0] == 0).all() and g["mbbox"][-1, -1].any()
    elif case == "f":
        assert npos_r == d["tcls"].size
        assert (np.abs(g["mbbox"]).sum((2, 3)) > 0).all() and (np.abs(g["mmask"]).sum((2, 3, 4)) > 0).all()


def test_losses_more_positives_than_target_rows(dev):
    """rpn_bbox_t with fewer rows than an image has positive anchors: the surplus positives (the last in anchor order) leave the box
    loss and stay in the class loss.  Reference: the class loss of the full match, the box loss of the match with the surplus set to -1."""
    d, match_box = M.losses_surplus_inputs()
    rows = d["rpn_bbox_t"].shape[1]
    npos = (d["rpn_match"][:, :, 0] == 1).sum(1)
    assert npos.max() > rows and (match_box == 1).sum() < (d["rpn_match"] == 1).sum()
    assert ((match_box[:, :, 0] == 1).sum(1) <= rows).all() and ((match_box != 0) == (d["rpn_match"] != 0)).all()
    ref = M.losses_reference(_loss_cfg(False), d, rpn_match_box=match_box)
    got = _run_losses(dev, d, False)
    _report("losses, surplus positives", got, ref)
    M.assert_losses_close(got[0], got[1], ref[0], ref[1])
    dropped = (d["rpn_match"][:, :, 0] == 1) & (match_box[:, :, 0] != 1)
    assert dropped.sum() > 0 and (got[1]["rpn_bbox"][dropped] == 0).all() and (got[1]["rpn_logits"][dropped] != 0).all()


@pytest.mark.parametrize("dice", [False, True])
def test_losses_workspace_reuse(dev, dice):
    """The grown workspace (rank[], scal[]) of the A = 98 309 call is reused by the A = 4092 call without a positive anchor and by an
    ordinary call: each gives what the same inputs give on a workspace of their own.  Exact, except for what passes through the
    float atomics on scal[] (the five losses, and with the Dice loss d_mmask, which is scaled by two such sums): loss tolerances."""
    ops = _ops()
    cases = [M.losses_rank_inputs(98309), M.losses_empty_inputs("a"), M.losses_inputs(4, False)]

    def fresh():
        for k in [k for k in ops._ws_cache if k[1] == "losses"]:
            del ops._ws_cache[k]

    first = []
    for d in cases:
        fresh()
        first.append(_run_losses(dev, d, dice))
    fresh()
    sizes = []
    for d, (ls0, g0) in zip(cases, first):
        ls, g = _run_losses(dev, d, dice)
        sizes.append([v.numel() for k, v in ops._ws_cache.items() if k[1] == "losses"])
        np.testing.assert_allclose(ls, ls0, **M.LOSS_TOL)
        for n in M.LOSS_GRADS:
            if dice and n == "mmask":
                np.testing.assert_allclose(g[n], g0[n], **M.LOSS_TOL)
            else:
                assert np.array_equal(g[n], g0[n]), n
    assert sizes[0] == sizes[1] == sizes[2] and len(sizes[0]) == 1          # one buffer, grown once


# ---- 2. detection targets -----------------------------------------------------------------------------------------------------------------
def _run_detection_targets(dev, s, cfg):
    got = _ops().detection_targets(*(torch.tensor(s[k], device=dev) for k in ("props", "gt_cls", "gt_boxes", "gt_masks", "keys")),
                                   s["T"], cfg.ROI_POSITIVE_RATIO, cfg.BBOX_STD_DEV, cfg.MASK_SHAPE, use_mini_mask=bool(cfg.USE_MINI_MASK))
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in got]


def _detection_targets_scene(dev, name, mini):
    counts_ref = M.check_detection_target_case(name, mini)               # the scene's preconditions, from the oracle side
    s, cfg, ref = M.detection_target_case(name, mini)
    rois, tcls, tbbox, tmask, assign, counts = _run_detection_targets(dev, s, cfg)
    assert [tuple(c) for c in counts.tolist()] == [tuple(c) for c in counts_ref]
    for b, (r_rois, r_cls, r_bb, r_m, (P, N)) in enumerate(ref):
        np.testing.assert_array_equal(rois[b], r_rois)
        np.testing.assert_array_equal(tcls[b], r_cls)
        np.testing.assert_allclose(tbbox[b], r_bb, rtol=1e-5, atol=1e-5)
        np.testing.assert_array_equal(tmask[b], r_m)
        assert (assign[b, P:] == -1).all() and (assign[b, :P] >= 0).all()
    return s, ref, assign


@pytest.mark.parametrize("name", M.DT_SCENES)
def test_detection_targets_counts(dev, name):
    """The scenes of model_cases.DT_SCENES against OracleMaskRCNN.detection_targets, as strict as test_detection_targets: ROIs, class
    ids, mask targets and the counts (P, N) exact, box targets to 1e-5.  `sweep`: 0 .. 68 positives in one launch (quota 66), N with
    its float32 steps; `layout`, `t48`, `t512`, `equal_keys`, `zero_keys`: GT rows at non-contiguous indices with a duplicate box,
    T = 200 / 48 / 512, ties by lowest row; `thresholds`: IoU of exactly 0.5 and the crowd limit 0.001 from both sides; `scarce`:
    fewer negatives than asked for; `no_gt`, `only_crowds`, `zero_proposals`: P = N = 0, all outputs zero; `single`: R = 1;
    `caps`: R = 2048, G = 512 with the GT in the last rows."""
    s, ref, assign = _detection_targets_scene(dev, name, False)
    if name in ("layout", "t48", "t512", "equal_keys", "zero_keys"):
        for b, r in enumerate(ref):
            assert set(assign[b, :r[4][0]].tolist()) == set(M.LAYOUT_INSTANCES)     # original rows; the duplicate resolves to row 4
    if name == "caps":
        assert set(assign[0, :66].tolist()) == {509, 510, 511}


@pytest.mark.parametrize("name", M.DT_MINI_SCENES)
def test_detection_targets_counts_mini_mask(dev, name):
    """The layout and threshold scenes with USE_MINI_MASK: the ROI is re-expressed in the frame of the GT box of the ORIGINAL row."""
    _detection_targets_scene(dev, name, True)


def test_detection_targets_beyond_caps(dev):
    """R = 2049 (> DT_CAP) and G = 513 (> DT_GCAP) are refused, not truncated."""
    from caesar_mrcnn_amd._hip import HipPathError
    ops = _ops()
    cfg = M.detection_target_cfg(200)
    z = lambda *shape, dt=torch.float32: torch.zeros(shape, dtype=dt, device=dev)
    for R, G in ((2049, 8), (16, 513)):
        with pytest.raises(HipPathError):
            ops.detection_targets(z(1, R, 4), z(1, G, dt=torch.int32), z(1, G, 4), z(1, 8, 8, G, dt=torch.uint8), z(1, R), 200,
                                  cfg.ROI_POSITIVE_RATIO, cfg.BBOX_STD_DEV, cfg.MASK_SHAPE)
    torch.cuda.synchronize()


# ---- 3. detection layer ---------------------------------------------------------------------------------------------------------------------
def _run_detections(dev, inp, cfg):
    rois, probs, deltas, windows = inp
    out = _ops().detections(torch.tensor(rois, device=dev), torch.tensor(probs, device=dev), torch.tensor(deltas, device=dev),
                            torch.tensor(windows, device=dev), cfg.DETECTION_MAX_INSTANCES, cfg.DETECTION_MIN_CONFIDENCE,
                            cfg.DETECTION_NMS_THRESHOLD, cfg.BBOX_STD_DEV)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _assert_detections(got, ref):
    for b in range(len(ref)):
        assert np.array_equal(got[b][:, 4], ref[b][:, 4]), "class ids / order differ"
        assert np.array_equal(got[b][:, 5], ref[b][:, 5])
        np.testing.assert_allclose(got[b][:, :4], ref[b][:, :4], rtol=0, atol=2e-6)


@pytest.mark.parametrize("R,n,maxi,minconf", M.DETECTION_COUNT_CASES)
def test_detection_layer_counts(dev, R, n, maxi, minconf):
    """refine_detections with exactly n candidates per image (model_cases.DETECTION_COUNT_CASES): none, one, the edges of the 64-wide
    chunks of the scan and tiles of the suppression matrix, R = 1, 63 and DET_CAP, max_instances above and below the survivors.
    As strict as test_detection_layer: class ids, scores and order exact, boxes to 2e-6."""
    inp, cfg, ref, nvalid = M.detection_count_case(R, n, maxi, minconf)
    got = _run_detections(dev, inp, cfg)
    assert got.shape == (2, maxi, 6)
    _assert_detections(got, ref)
    for b in range(2):
        if nvalid[b] == 0:
            assert (got[b] == 0).all()


def test_detection_layer_empty_call_between_full_ones(dev):
    """A call without any candidate between two ordinary ones on the same workspace: nvalid, keep[] and the suppression words the
    first call left behind are not read by the second, nor the (absent) ones of the second by the third."""
    full = M.detection_count_case(1000, (1000, 1000), 100, 0)
    none = M.detection_count_case(1000, (0, 0), 100, 0)
    assert none[3] == [0, 0] and full[3] == [1000, 1000]
    outs = [_run_detections(dev, c[0], c[1]) for c in (full, none, full)]
    _assert_detections(outs[0], full[2])
    assert (outs[1] == 0).all()
    _assert_detections(outs[2], full[2])
    assert np.array_equal(outs[0], outs[2])


def test_detection_layer_beyond_cap(dev):
    """R = 2049 (> DET_CAP) is refused."""
    from caesar_mrcnn_amd._hip import HipPathError
    cfg = M.detection_count_case(1, (1, 1), 100, 0)[1]
    z = lambda *shape: torch.zeros(shape, device=dev)
    with pytest.raises(HipPathError):
        _ops().detections(z(1, 2049, 4), z(1, 2049, 4), z(1, 2049, 4, 4), z(1, 4), 100, 0, cfg.DETECTION_NMS_THRESHOLD, cfg.BBOX_STD_DEV)
    torch.cuda.synchronize()
