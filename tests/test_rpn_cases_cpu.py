"""The cases of tests/rpn_cases.py, checked without a GPU: each has the property it exists for (ties at the K-th score, the scan
ending at `count` or running out of boxes, IoUs of exactly 0.3 and 0.7, P and N at their caps), and its expected output changes
when the oracle is perturbed the way a kernel could plausibly fail -- so tests/test_rpn_counts_gpu.py can tell such a kernel from
a right one.  The perturbed rules are local to this file; oracle/mrcnn_oracle.py has no switches."""
import numpy as np
import pytest

import mrcnn_oracle as orc
import rpn_cases as R


# ---- perturbed rules ----------------------------------------------------------------------------------------------------------
def top_k_highest_index_first(scores, k):
    """tf_top_k_indices with the tie rule reversed"""
    n = len(scores)
    return n - 1 - np.argsort(-scores[::-1].astype(np.float32), kind="stable")[:k]


def nms_variant(boxes, scores, max_output_size, thr, ge=False, dead_suppress=False):
    """orc.tf_non_max_suppression; ge: suppress at IoU >= threshold; dead_suppress: a suppressed box still suppresses"""
    boxes = boxes.astype(np.float32)
    order = np.argsort(-scores.astype(np.float32), kind="stable")
    alive = np.ones(len(order), dtype=bool)
    keep = []
    thr = np.float32(thr)
    for pos in range(len(order)):
        if alive[pos]:
            if len(keep) >= max_output_size:
                break
            keep.append(order[pos])
        elif not dead_suppress:
            continue
        rest = np.where(alive[pos + 1:])[0] + pos + 1
        if rest.size:
            iou = orc.tf_iou(boxes, order[pos], order[rest])
            alive[rest[(iou >= thr) if ge else (iou > thr)]] = False
    return np.array(keep, dtype=np.int64)


def rpn_match_variant(anchors, gt_boxes, pos=lambda v: v >= 0.7, neg=lambda v: v < 0.3):
    """rpn_match of build_rpn_targets before the draws, for a scene without crowds, with the two threshold tests injectable"""
    ov = orc.compute_overlaps(anchors, gt_boxes)
    mx = ov.max(axis=1)
    m = np.zeros(anchors.shape[0], np.int32)
    m[neg(mx)] = -1
    m[np.argwhere(ov == ov.max(axis=0))[:, 0]] = 1
    m[pos(mx)] = 1
    return m


class HighestIndexFirst(orc.KeyedChoice):
    """the keyed draw with the tie rule reversed"""

    def choice(self, ids, n, replace=False):
        ids = np.asarray(ids)
        return ids[np.lexsort((-ids, self.keys[ids]))[:n]]


def test_variants_with_the_right_rule_are_the_oracle():
    d = R.proposal_inputs("nms_thr0")
    ix, boxes, keep = R.proposal_reference("nms_thr0")[1][0]
    assert np.array_equal(nms_variant(boxes, d["fg"][0][ix], 1000, 0.0), keep)
    s = R.rpn_scene("thresholds")
    assert np.array_equal(rpn_match_variant(s["anchors"], s["gt_boxes"][0][:len(R.THRESHOLD_GTS)]), R.rpn_expected(s)[0][0])


# ---- ProposalLayer ----------------------------------------------------------------------------------------------------------------
def _check_expect(c, details):
    for ix, boxes, keep in details:
        assert len(ix) == min(c.limit, c.A) and len(keep) <= min(c.count, len(ix))
        if c.expect == "runs_out":
            assert len(keep) < c.count
        elif c.expect == "hits_count":
            assert len(keep) == c.count


@pytest.mark.parametrize("name", R.PROPOSAL_RANDOM + ["reuse_A65472"])
def test_proposal_random_case_preconditions(name):
    c = R.PROPOSAL_CASES[name]
    d = R.proposal_inputs(name)
    rois, details = R.proposal_reference(name)
    K = d["K"]
    _check_expect(c, details)
    assert np.abs(d["deltas"] * R.RPN_BBOX_STD_DEV.astype(np.float32)).max() < 80          # no exp overflow: no NaN box in the reference
    assert np.isfinite(rois).all()
    for b, (ix, boxes, keep) in enumerate(details):
        cnt_eq, need_eq = R.threshold_ties(d["fg"][b], K)
        print("[%s] image %d: K = %d, %d scores at the K-th value for %d slots, %d of %d kept" % (name, b, K, cnt_eq, need_eq, len(keep), c.count))
        assert (rois[b, len(keep):] == 0).all()
        if c.ties is True:
            assert cnt_eq > need_eq                                                         # the ordered compaction runs
            assert not np.array_equal(top_k_highest_index_first(d["fg"][b], K), ix)         # and its order is visible
        elif c.ties is False:
            assert cnt_eq == need_eq
    assert R.proposal_expected_status(name) == ((K, K, 0) if c.A >= 32768 else (0, 0, 0))
    if name.startswith("tiny"):
        assert c.count > K
    if c.scores == "equal":
        assert all(np.array_equal(ix, np.arange(K)) for ix, _, _ in details)               # the order is the anchor index
    if c.scores == "two":
        fg, ix = d["fg"][0], details[0][0]
        last = int(ix[fg[ix] == np.float32(0.25)].max())                                    # the last tie taken
        assert last == R.TIES_TWO_LAST_TAKEN[name]
        assert 4 <= last % 64 <= 59 and (fg[:last] == np.float32(0.75)).sum() > 0 and (fg[last + 1:] == np.float32(0.25)).sum() > 0
        step, base = (256, last - last % 4000) if c.A >= R.PRE_MIN else (1024, 0)          # the kernel's iteration that holds it
        assert 64 <= (last - base) % step < step - 64 and (last - base) // step > 0
    if name == "ties_zero_one":
        fg = d["fg"]
        assert (fg[0] == 0).all() and (fg[2] == 1).all() and len(np.unique(fg[1])) == c.A and fg[1].min() == 0 and fg[1].max() == 1
        assert np.array_equal(details[0][0], np.arange(K)) and np.array_equal(details[2][0], np.arange(K))
    if name == "decode_extremes":
        sd = d["deltas"] * R.RPN_BBOX_STD_DEV.astype(np.float32)
        assert np.isclose(sd[..., :2].max(), 20) and np.isclose(sd[..., :2].min(), -20)
        assert np.isclose(sd[..., 2:].max(), 20) and np.isclose(sd[..., 2:].min(), -20)
        assert not ((np.abs(sd[..., :2]) > 3).any(-1) & (np.abs(sd[..., 2:]) > 3).any(-1)).any()      # never both in one anchor
        for ix, boxes, keep in details:
            area = (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])
            assert (area == 0).sum() > 100 and (area == 1).sum() > 100 and ((area > 0) & (area < 1)).sum() > 100


@pytest.mark.parametrize("name", R.PROPOSAL_EXACT)
def test_proposal_exact_case_preconditions(name):
    c = R.PROPOSAL_CASES[name]
    d = R.proposal_inputs(name)
    rois, details = R.proposal_reference(name)
    assert c.B == 1 and not d["deltas"].any() and np.array_equal(d["anchors"] * 128, np.round(d["anchors"] * 128))
    assert len(np.unique(d["fg"][0])) == c.A
    _check_expect(c, details)
    ix, boxes, keep = details[0]
    fg = d["fg"][0][ix]
    np.testing.assert_array_equal(boxes, np.clip(d["anchors"][ix], 0, 1))                   # decode and clip are exact
    assert np.array_equal(nms_variant(boxes, fg, c.count, c.thr), keep)
    ge = nms_variant(boxes, fg, c.count, c.thr, ge=True)
    dead = nms_variant(boxes, fg, c.count, c.thr, dead_suppress=True)
    print("[%s] %d of %d kept (count %d); with >=: %d, with suppression by dead boxes: %d" % (name, len(keep), c.A, c.count, len(ge), len(dead)))
    if c.builder == "disjoint":
        assert np.array_equal(keep, np.arange(min(c.count, 200)))
    elif c.builder == "clusters":
        assert np.array_equal(keep, np.arange(min(c.count, 70)))
    elif c.builder == "identical":
        assert np.array_equal(keep, [0])
    elif name == "nms_thr0":
        k = boxes[keep]
        pair = np.array([orc.tf_iou(k, i, np.arange(len(k))) for i in range(len(k))])
        assert (pair[~np.eye(len(k), dtype=bool)] == 0).all() and 1 < len(keep) < c.A
        touching = sum(int(((k[:, 2] == b[0]) | (k[:, 0] == b[2]) | (k[:, 3] == b[1]) | (k[:, 1] == b[3])).sum()) for b in k)
        print("[%s] kept boxes sharing an edge coordinate: %d" % (name, touching))
        assert len(ge) == 1                                                                 # IoU >= 0 suppresses everything
    elif name == "nms_thr1":
        assert len(keep) == c.A and len(ge) <= c.A - 20                                     # the duplicates sit at IoU == 1 exactly
    elif c.builder == "zero_area":
        area = (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])
        zero = np.where(area == 0)[0]
        assert len(zero) >= 40 and np.isin(zero, keep).all() and len(keep) < c.A
        same = sum(int((boxes[zero] == boxes[z]).all(1).sum()) - 1 for z in zero)
        assert same >= 40                                                                   # identical zero-area boxes, none suppressed
        clipped = (np.clip(d["anchors"][ix], 0, 1) != d["anchors"][ix]).any(1) & (area > 0)
        assert clipped.sum() >= 10
    elif c.builder == "chain":
        pa, pb, pc = R.CHAIN_POSITIONS[name]
        assert np.array_equal(boxes[[pa, pb, pc]] * 128, R.CHAIN)
        assert pa in keep and pb not in keep and pc in keep and len(keep) == c.A - 1
        assert pc not in dead and len(dead) == c.A - 2                                      # a dead b would have taken c with it
        iou = orc.tf_iou(boxes, pa, np.array([pb, pc]))
        assert iou[0] > c.thr and iou[1] <= c.thr and orc.tf_iou(boxes, pb, np.array([pc]))[0] > c.thr
        if c.A > 4096:
            assert pc >= 4096 and pb // 64 < 64 <= pc // 64                                 # c's bit lives in word 64: rem1


def test_proposal_case_list_is_the_announced_one():
    A_K = {(c.A, min(c.limit, c.A)) for c in R.PROPOSAL_CASES.values() if c.kind == "random"}
    for A in (1, 7, 8, 9, 63, 64, 65, 127, 128, 129):
        assert (A, A) in A_K
    for K in (511, 512, 513, 1023, 1024, 1025, 4096, 4097):
        assert (K + 37, K) in A_K
    for A in (1023, 1024, 1025):
        assert (A, A) in A_K
    for A in (16384, 16385, 25575, 32767, 32768, 262144, 262145, 409200, 6001):
        assert (A, 6000) in A_K
    assert {(200, 64), (8192, 8192), (9000, 8192), (6000, 6000), (32768, 8192)} <= A_K
    assert {c.B for c in R.PROPOSAL_CASES.values()} == {1, 2, 3}
    assert [R.PROPOSAL_CASES["nms_disjoint_c%d" % n].count for n in R.DISJOINT_COUNTS] == [1, 63, 64, 65, 128, 199, 200, 201, 300]
    assert all(min(l, A) > R.SORT_CAP or n > R.SORT_CAP for A, l, n in R.PROPOSAL_REFUSALS)


# ---- RPN targets ------------------------------------------------------------------------------------------------------------------
def _counts(e):
    return [(int((m == 1).sum()), int((m == -1).sum())) for m, _ in e]


@pytest.mark.parametrize("name", list(R.RPN_SCENES))
def test_rpn_scene_preconditions(name):
    s = R.rpn_scene(name)
    e = R.rpn_expected(s)
    nt, A = s["n_train"], s["anchors"].shape[0]
    B, G = s["gt_cls"].shape
    counts = _counts(e)
    print("[%s] A = %d, G = %d, n_train = %d, (P, N) = %s" % (name, A, G, nt, counts))
    assert A == {32: 258, 64: 1023, 128: 4092, 256: 16368}[s["S"]] and G <= R.RT_MAXG
    for (P, N), (m, bb) in zip(counts, e):
        assert P <= nt // 2 and P + N <= nt and bb.shape == (nt, 4) and not bb[P:].any()
    if name.startswith("small"):
        assert all(P > 0 and N > 0 for P, N in counts)
    elif name == "g1":
        assert G == 1 and counts[0][0] >= 1
    elif name == "g512_full":
        assert G == 512 and (s["gt_cls"] > 0).all() and counts == [(128, 128)]
    elif name == "g512_last_rows":
        assert G == 512 and not s["gt_cls"][:, :507].any() and (s["gt_cls"][:, 507:] > 0).all() and counts[0][0] > 0
    elif name.startswith("ntrain"):
        P0 = int((R.rpn_uncapped_match(s, 0) == 1).sum()); N0 = int((R.rpn_uncapped_match(s, 0) == -1).sum())
        assert P0 >= 4
        if nt == 512:
            assert nt > A and counts == [(P0, N0)]                                          # nothing dropped
        else:
            assert counts == [{1: (0, 1), 2: (1, 1), 7: (3, 4)}[nt]]
    elif name.startswith("caps"):
        P0, N0 = R.rpn_uncapped_counts()
        want = {"caps_pos_exact": (P0, nt - P0), "caps_pos_drop1": (P0 - 1, nt - P0 + 1), "caps_neg_exact": (P0, N0),
                "caps_neg_drop1": (P0, N0 - 1)}[name]
        assert counts == [want]
        if name == "caps_pos_exact":
            assert P0 == nt // 2
        if name.startswith("caps_neg"):
            assert nt // 2 >= P0 and nt - P0 == {"caps_neg_exact": N0, "caps_neg_drop1": N0 - 1}[name]
    elif name in R.RPN_KEY_TIE_SCENES:
        dropped_pos = dropped_neg = False
        for b in range(B):
            m0, m = R.rpn_uncapped_match(s, b), e[b][0]
            dp, dn = np.where((m0 == 1) & (m == 0))[0], np.where((m0 == -1) & (m == 0))[0]
            dropped_pos |= len(dp) > 0
            dropped_neg |= len(dn) > 0
            other = R.rpn_expected_image(s["anchors"], s["gt_cls"][b], s["gt_boxes"][b], s["keys"][b], nt, rng=HighestIndexFirst(s["keys"][b]))[0]
            assert not np.array_equal(other, m)                                             # the tie rule is visible
            if name != "keys_three_values":
                assert len(np.unique(s["keys"][b])) == 1 and s["keys"][b, 0] == (0.5 if name == "keys_equal" else 0.0)
                for ids, d in ((np.where(m0 == 1)[0], dp), (np.where(m0 == -1)[0], dn)):
                    assert np.array_equal(d, ids[:len(d)])                                  # the lowest anchor indices are dropped
            else:
                v = s["keys"][b][dn].max()                                                  # the key at the threshold of the negative draw
                grp = np.where((m0 == -1) & (s["keys"][b] == v))[0]
                kept = np.isin(grp, dn, invert=True)
                assert kept.any() and not kept.all() and len(np.unique(grp // 16)) > 100    # chunk = ceil(16 368 / 1024) = 16
                assert (np.isin(np.arange(15, A - 1, 16), grp) & np.isin(np.arange(16, A, 16), grp)).sum() > 10   # ties on both sides of a chunk edge
        assert dropped_pos and dropped_neg
    elif name == "thresholds":
        gts = s["gt_boxes"][0][:len(R.THRESHOLD_GTS)]
        ov = orc.compute_overlaps(s["anchors"], gts)
        idx = [R.threshold_anchor_index(cy, cx) for _, cy, cx, _, _ in R.THRESHOLD_GTS]
        iou = [ov[a, g] for g, a in enumerate(idx)]
        assert iou[0] == 0.7 and iou[3] == 0.3 and iou[1] < 0.7 < iou[2] and iou[4] < 0.3 < iou[5]
        assert all(ov[a].max() == v for a, v in zip(idx, iou))                              # nothing else matches the named anchors better
        m = e[0][0]
        assert [int(m[a]) for a in idx] == [1, 1, 1, 0, -1, 0]
        assert counts[0][0] + counts[0][1] == int((R.rpn_uncapped_match(s, 0) != 0).sum())  # nothing dropped: every anchor is visible
        le = rpn_match_variant(s["anchors"], gts, neg=lambda v: v <= 0.3)
        assert le[idx[3]] == -1 and (le != m).sum() == 1
        # "> 0.7" changes nothing here and cannot: the named anchor is the best anchor of its GT, so the reference's third rule
        # (every GT keeps its best anchors) makes it positive whatever the second says.  No integer GT box has an IoU of exactly
        # 0.7 with a ratio-1 anchor and a larger one with any other anchor of the pyramid (searched: none for scales 8 .. 64).
        assert ov[:, 0].max() == 0.7 and np.array_equal(rpn_match_variant(s["anchors"], gts, pos=lambda v: v > 0.7), m)
    elif name == "empties":
        cls = s["gt_cls"]
        assert not cls[0].any() and (cls[2][cls[2] != 0] < 0).all() and (cls[2] < 0).sum() == 3 and (cls[1] > 0).sum() == 4
        assert (cls[3] > 0).sum() == 4 and (cls[3] < 0).sum() == 1
        for b in (0, 2):                                                                    # the reference itself cannot say
            nz = cls[b] != 0
            with pytest.raises(ValueError):
                orc.build_rpn_targets(s["anchors"], cls[b][nz], s["gt_boxes"][b][nz], nt, R.RPN_BBOX_STD_DEV, rng=orc.KeyedChoice(s["keys"][b]))
            assert counts[b] == (0, nt)
        crowd_iou = orc.compute_overlaps(s["anchors"], s["gt_boxes"][2][cls[2] < 0]).max(1)
        near = crowd_iou >= 0.001
        assert near.sum() > 100 and not (e[2][0][near] == -1).any()
        free = np.where(~near)[0]
        drop = orc.KeyedChoice(s["keys"][2]).choice(free, len(free) - nt)
        assert np.array_equal(np.where(e[2][0] == -1)[0], np.setdiff1d(free, drop))
        assert counts[1][0] > 0 and counts[3][0] > 0


def test_rpn_scene_list_is_the_announced_one():
    shapes = {(s["anchors"].shape[0], s["gt_cls"].shape[0]) for s in map(R.rpn_scene, R.RPN_SCENES)}
    assert {258, 1023, 4092, 16368} == {a for a, _ in shapes} and {1, 4} <= {b for _, b in shapes}
    assert [R.rpn_scene(n)["anchors"].shape[0] for n in R.RPN_REUSE_SEQUENCE] == [16368, 258, 16368]
    assert R.rpn_scene(R.RPN_REUSE_SEQUENCE[0])["gt_cls"].shape[1] != R.rpn_scene(R.RPN_REUSE_SEQUENCE[1])["gt_cls"].shape[1]
