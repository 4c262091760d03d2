"""csrc/proposal.hip and csrc/rpn_targets.hip at the sizes, counts, ties and exact thresholds at which their code branches, against
the CPU oracle (cases and their oracle-side expectations: tests/rpn_cases.py; preconditions and perturbation checks without a GPU:
tests/test_rpn_cases_cpu.py).  ProposalLayer: K = 1 .. 8192 across the padding, shuffle and LDS stages of the sort network, the
three selection paths and their edges, limit == A and A - 1, all-equal / two-valued / 0.0 and 1.0 scores, NMS scans that stop at
proposal_count, at it exactly, or run out of boxes, chains through both remove registers, zero-area boxes, thresholds 0 and 1,
decode extremes, a reused workspace, refusals.  RPN targets: A = 258 .. 16 368, G = 1 and 512, n_train = 1 .. 32 736, P and N at
their caps and one over, equal keys, IoU of exactly 0.3 and 0.7, images without GT or with crowds only, a reused workspace.
As strict as test_proposal_layer, test_proposal_nms_at_exact_threshold_pairs and test_rpn_targets_device."""
import numpy as np
import pytest
import torch

import mrcnn_oracle as orc
import rpn_cases as R

pytestmark = pytest.mark.gpu


def _ops():
    from caesar_mrcnn_amd import ops
    return ops


# ---- ProposalLayer ----------------------------------------------------------------------------------------------------------------
def _run_proposals(dev, name):
    """-> [rois, top_idx, keep_idx, num_keep, boxes] as NumPy, status words [B,3]"""
    c, d = R.PROPOSAL_CASES[name], R.proposal_inputs(name)
    probs = torch.tensor(d["probs"], device=dev)
    out = _ops().proposals(probs, torch.tensor(d["deltas"], device=dev), torch.tensor(d["anchors"], device=dev), c.limit, c.count,
                           c.thr, R.RPN_BBOX_STD_DEV, debug=True)
    torch.cuda.synchronize()
    out = [t.cpu().numpy().copy() for t in out]
    return out, _ops().proposal_status(probs, c.limit, c.count)


def _assert_shapes_and_status(name, out, status):
    c = R.PROPOSAL_CASES[name]
    K = min(c.limit, c.A)
    rois, top_idx, keep_idx, num_keep, boxes = out
    assert rois.shape == (c.B, c.count, 4) and top_idx.shape == (c.B, K) and keep_idx.shape == (c.B, c.count) and boxes.shape == (c.B, K, 4)
    assert (num_keep <= min(K, c.count)).all()
    assert status.tolist() == [list(R.proposal_expected_status(name))] * c.B, status


@pytest.mark.parametrize("name", R.PROPOSAL_RANDOM + ["reuse_A65472"])
def test_proposal_random_cases(dev, name):
    """top_idx exact, decoded boxes at 2e-6 (expf against np.exp), num_keep and keep_idx exact against tf_non_max_suppression re-run on
    the GPU-decoded boxes, keep_idx padded with -1, rois the gathered boxes and exactly zero behind them; the selection's health
    words {collected, announced, refused} are {K, K, 0} from A = 32 768 on and {0, 0, 0} below."""
    c, d = R.PROPOSAL_CASES[name], R.proposal_inputs(name)
    _, details = R.proposal_reference(name)
    out, status = _run_proposals(dev, name)
    _assert_shapes_and_status(name, out, status)
    rois, top_idx, keep_idx, num_keep, boxes = out
    for b, (ix, ref_boxes, _) in enumerate(details):
        assert np.array_equal(top_idx[b], ix.astype(np.int32)), "top-k order differs"
        np.testing.assert_array_equal(ix, orc.tf_top_k_indices(d["fg"][b], d["K"]))
        print("[%s] image %d: largest box difference %.3g" % (name, b, np.abs(boxes[b] - ref_boxes).max()))
        np.testing.assert_allclose(boxes[b], ref_boxes, rtol=0, atol=2e-6)
        keep2 = orc.tf_non_max_suppression(boxes[b], d["fg"][b][ix], c.count, c.thr)
        n = int(num_keep[b])
        assert n == len(keep2)
        assert np.array_equal(keep_idx[b, :n], keep2.astype(np.int32))
        assert (keep_idx[b, n:] == -1).all()
        np.testing.assert_array_equal(rois[b, :n], boxes[b][keep2])
        assert (rois[b, n:] == 0).all()


@pytest.mark.parametrize("name", R.PROPOSAL_EXACT)
def test_proposal_exact_cases(dev, name):
    """Anchors on multiples of 1/128, zero deltas: everything bit-identical to the oracle's own end-to-end proposal_layer."""
    c = R.PROPOSAL_CASES[name]
    ref_rois, details = R.proposal_reference(name)
    out, status = _run_proposals(dev, name)
    _assert_shapes_and_status(name, out, status)
    rois, top_idx, keep_idx, num_keep, boxes = out
    for b, (ix, ref_boxes, keep) in enumerate(details):
        assert np.array_equal(top_idx[b], ix.astype(np.int32))
        np.testing.assert_array_equal(boxes[b], ref_boxes)
        n = int(num_keep[b])
        assert n == len(keep), (n, len(keep))
        assert np.array_equal(keep_idx[b, :n], keep.astype(np.int32)) and (keep_idx[b, n:] == -1).all()
    np.testing.assert_array_equal(rois, ref_rois)


def test_proposal_workspace_reuse(dev):
    """A = 65 472 with K = 6000, then A = 1023, then K = 4097 (65 words per row), then the first again, on one stream and one
    grow-only workspace: each result equals that call's result on a workspace of its own.  The lower-triangular words of the bit
    matrix are never written, so the later calls find the earlier calls' boxes and bits in them, and the health words of the call
    without a pre-selection lie where the first call kept suppression bits."""
    ops = _ops()

    def fresh():
        for k in [k for k in ops._ws_cache if k[1] == "proposal"]:
            del ops._ws_cache[k]

    first = []
    for name in R.PROPOSAL_REUSE_SEQUENCE:
        fresh()
        first.append(_run_proposals(dev, name))
    fresh()
    sizes = []
    for name, (out0, st0) in zip(R.PROPOSAL_REUSE_SEQUENCE, first):
        out, st = _run_proposals(dev, name)
        sizes.append([v.numel() for k, v in ops._ws_cache.items() if k[1] == "proposal"])
        for a, a0 in zip(out, out0):
            assert np.array_equal(a, a0), name
        assert st.tolist() == st0.tolist() == [list(R.proposal_expected_status(name))] * R.PROPOSAL_CASES[name].B, (name, st, st0)
    assert len(sizes[0]) == 1 and all(s == sizes[0] for s in sizes)          # one buffer, grown once


def test_proposal_refusals(dev):
    """pre_nms_limit = 8193 (with A = 9000, so K = 8193) and proposal_count = 8193 are refused by the host-side argument check."""
    from caesar_mrcnn_amd._hip import HipPathError
    for A, limit, count in R.PROPOSAL_REFUSALS:
        z = lambda *shape: torch.zeros(shape, device=dev)
        with pytest.raises(HipPathError):
            _ops().proposals(z(1, A, 2), z(1, A, 4), z(A, 4), limit, count, 0.7, R.RPN_BBOX_STD_DEV, debug=True)
    torch.cuda.synchronize()


# ---- RPN targets ------------------------------------------------------------------------------------------------------------------
def _run_rpn_targets(dev, s, images=None):
    sel = slice(None) if images is None else images
    match, bbox = _ops().rpn_targets(torch.tensor(s["anchors"], device=dev), torch.tensor(np.ascontiguousarray(s["gt_cls"][sel]), device=dev),
                                     torch.tensor(np.ascontiguousarray(s["gt_boxes"][sel]), device=dev),
                                     torch.tensor(np.ascontiguousarray(s["keys"][sel]), device=dev), s["n_train"], R.RPN_BBOX_STD_DEV)
    torch.cuda.synchronize()
    return match.cpu().numpy().copy(), bbox.cpu().numpy().copy()


@pytest.mark.parametrize("name", list(R.RPN_SCENES))
def test_rpn_target_scenes(dev, name):
    """rpn_match exact, rpn_bbox at rtol 2e-6 / atol 1e-6 against build_rpn_targets with the keyed draw; images without an instance
    among their GT rows against rpn_cases.rpn_expected_without_gt (the reference raises there)."""
    s = R.rpn_scene(name)
    ref = R.rpn_expected(s)
    match, bbox = _run_rpn_targets(dev, s)
    B, A = s["keys"].shape
    assert match.shape == (B, A, 1) and bbox.shape == (B, s["n_train"], 4)
    for b, (rm, rb) in enumerate(ref):
        np.testing.assert_array_equal(match[b, :, 0], rm)
        np.testing.assert_allclose(bbox[b], rb.astype(np.float32), rtol=2e-6, atol=1e-6)
        assert not bbox[b, int((rm == 1).sum()):].any()
    if name == "empties":                      # the ordinary images of the batch equal their single-image results
        for b in (1, 3):
            m1, b1 = _run_rpn_targets(dev, s, images=[b])
            assert np.array_equal(m1[0], match[b]) and np.array_equal(b1[0], bbox[b])
        assert not bbox[0].any() and not bbox[2].any() and not (match[0] == 1).any() and not (match[2] == 1).any()


def test_rpn_targets_workspace_reuse(dev):
    """A 256 x 256 call (G = 300), a 32 x 32 call (G = 8), the first again on one workspace: colmax is cleared per call, arg is not,
    and the small call's arg[] lies inside the large call's colmax / arg."""
    ops = _ops()

    def fresh():
        for k in [k for k in ops._ws_cache if k[1] == "rpn_targets"]:
            del ops._ws_cache[k]

    scenes = [R.rpn_scene(n) for n in R.RPN_REUSE_SEQUENCE]
    first = []
    for s in scenes:
        fresh()
        first.append(_run_rpn_targets(dev, s))
    fresh()
    for s, (m0, b0) in zip(scenes, first):
        m, bb = _run_rpn_targets(dev, s)
        assert np.array_equal(m, m0) and np.array_equal(bb, b0)
        for b, (rm, rb) in enumerate(R.rpn_expected(s)):
            np.testing.assert_array_equal(m[b, :, 0], rm)
            np.testing.assert_allclose(bb[b], rb.astype(np.float32), rtol=2e-6, atol=1e-6)
    assert len([k for k in ops._ws_cache if k[1] == "rpn_targets"]) == 1


def test_rpn_targets_refuses_more_than_512_gt_rows(dev):
    """G = 513 (> RT_MAXG) is refused by the host-side argument check, not truncated."""
    from caesar_mrcnn_amd._hip import HipPathError
    s = R.rpn_scene("small_A258")
    A, G = s["anchors"].shape[0], R.RT_MAXG + 1
    with pytest.raises(HipPathError):
        _ops().rpn_targets(torch.tensor(s["anchors"], device=dev), torch.zeros((1, G), dtype=torch.int32, device=dev),
                           torch.zeros((1, G, 4), dtype=torch.int32, device=dev), torch.zeros((1, A), device=dev), 64, R.RPN_BBOX_STD_DEV)
    torch.cuda.synchronize()
