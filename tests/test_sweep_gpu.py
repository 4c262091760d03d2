"""csrc/apsweep.hip (ops.ap_sweep) against its host statement metrics.sweep_tables_host, integer for integer; metrics.sweep_metrics_device
against sweep_metrics_host and the recorded tool; ModelTester.compute_mAP with sweep_map on a real model, device against host."""
import contextlib
import io
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sweep_cases as cases                                 # noqa: E402
import tester_cases as tcases                               # noqa: E402
from caesar_mrcnn_amd import _hip, analyze, metrics, ops    # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = np.load(cases.GOLDEN)
T10 = cases.IOU_THRESHOLDS
P_CAP, G_CAP, T_CAP, C_CAP = 128, 320, 16, 4096             # include/mrcnn_hip.h: MRCNN_AP_SWEEP_MAX_*


def _device_tables(pr, thr, dev):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    tp, status = ops.ap_sweep(t(pr.det_box), pr.det_off, t(pr.gt_box), pr.gt_off, t(np.asarray(thr, np.float64)))
    return tp.cpu().numpy(), status.cpu().numpy()


def _assert_tables(pr, thr, dev, what, overflowing=()):
    """Device tables == host tables on every problem whose status is 0; the status is set exactly on `overflowing`."""
    want, _ = metrics.sweep_tables_host(pr, thr)
    got, status = _device_tables(pr, thr, dev)
    assert got.dtype == want.dtype == np.int32 and got.shape == want.shape and status.shape == (pr.N,), what
    assert np.flatnonzero(status).tolist() == sorted(overflowing) and set(status.tolist()) <= {0, ops.AP_SWEEP_OVER_CANDIDATES}, (what, status)
    start, rows = metrics.sweep_table_entries(pr, len(thr))
    for p in overflowing:
        seg = slice(start[p], start[p] + len(thr) * rows[p])
        assert not got[seg].any() and want[seg].any(), what
        want[seg] = 0
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "%s: differs at %s: got %s, want %s" % (what, bad[:8].tolist(), got[bad[:8]].tolist(), want[bad[:8]].tolist())
    return want


def _crowd(n_det, n_gt, rng, label="source"):
    """One image: n_gt true boxes of 11 x 11 on a lattice 14 apart, n_det detections -- most of them a true box moved by up to 2.5
    pixels (a float, so IoUs differ), every eighth an exact copy (IoU 1, tied with the other copies), a few far away."""
    gt = [[14.0 * (j // 20), 14.0 * (j % 20), 14.0 * (j // 20) + 10, 14.0 * (j % 20) + 10, label] for j in range(n_gt)]
    pred = []
    for i in range(n_det):
        score = round(float(rng.uniform(0.05, 1.0)), 2)
        if n_gt == 0 or i % 7 == 6:
            y, x = (float(v) for v in rng.uniform(400, 600, 2))
            pred.append([y, x, y + 10, x + 10, label, score])
        else:
            g = gt[int(rng.integers(0, n_gt))]
            dy, dx = (0.0, 0.0) if i % 8 == 0 else (float(v) for v in rng.uniform(-2.5, 2.5, 2))
            pred.append([g[0] + dy, g[1] + dx, g[2] + dy, g[3] + dx, label, score])
    return gt, pred


SHAPES = [(p, g) for p in (0, 1, 63, 64, 65, P_CAP) for g in (0, 1, 65, G_CAP)]


@pytest.fixture(scope="module")
def shapes_set():
    rng = np.random.default_rng(20261020)
    images = [_crowd(p, g, rng) for p, g in SHAPES]
    return [im[0] for im in images], [im[1] for im in images]


@pytest.mark.parametrize("thr", [T10, (0.5,), (0.75, 0.5)], ids=["T10", "T1", "T2_unsorted"])
def test_ap_sweep_every_shape_in_one_launch(dev, shapes_set, thr):
    """P of 0, 1, 63, 64, 65 and the cap against G of 0, 1, 65 and the cap: 24 images, 48 problems (class-blind and the one
    class), one launch.  Many suffixes are more than one pass of the 256 lanes at T = 10."""
    gt, pred = shapes_set
    pr = metrics.SweepProblems(gt, pred)
    assert ops.ap_sweep_caps() == {"det": P_CAP, "gt": G_CAP, "thr": T_CAP, "cand": C_CAP}
    assert sorted(zip(np.diff(pr.det_off)[:24].tolist(), np.diff(pr.gt_off)[:24].tolist())) == sorted(SHAPES)
    want = _assert_tables(pr, thr, dev, "shapes")
    start, rows = metrics.sweep_table_entries(pr, len(thr))
    full = SHAPES.index((P_CAP, G_CAP))
    first = want[start[full]:start[full] + rows[full]]
    assert first[0] > 10 and first[0] > first[P_CAP // 2] > first[P_CAP] == 0     # the tables hold something to get wrong
    again, _ = _device_tables(pr, thr, dev)
    assert np.array_equal(again, _device_tables(pr, thr, dev)[0])                 # the same bits on every run


@pytest.mark.parametrize("name", cases.golden_sets(GOLDEN))
def test_ap_sweep_fixture_sets(dev, name):
    """The recorded sets -- an IoU of exactly n / 20 for each of the ten thresholds, tied IoUs whose order changes the match
    count, images without detections or ground truths -- at T = 10 and T = 1; the device metrics equal the host's, and the
    tool's recorded answer where it is pinned."""
    gt, pred, tied, _, want, _ = cases.load(GOLDEN, name)
    pr = metrics.SweepProblems(gt, pred)
    _assert_tables(pr, T10, dev, name)
    for th in (0.5, 0.75, T10[-1]):
        _assert_tables(pr, (th,), dev, "%s T=1 at %r" % (name, th))
    back = []
    got = metrics.sweep_metrics_device(gt, pred, device=dev, handed_back=back)
    assert back == [] and metrics.same_sweep(got, metrics.sweep_metrics_host(gt, pred)), name
    if not tied:
        assert cases.differences(cases.record(got), want) == [], name


def test_ap_sweep_ties_decide_the_count(dev):
    gt, pred, _ = cases.sets()["tied_pairs"]
    pr = metrics.SweepProblems(gt, pred)
    tp, status = _device_tables(pr, (0.5,), dev)
    assert status.tolist() == [0, 0] and tp[:5].tolist() == [2, 1, 1, 0, 0]      # the earlier pair first would give [2, 2, 1, 0, 0]


def _overflow_image():
    """70 identical detections on 70 identical true boxes, half of each under either class: 4900 pairs of IoU 1 class-blind
    (past the 4096 the kernel keeps), 1225 under each class (within)."""
    labels = ["galaxy", "source"]
    return ([[0, 0, 9, 9, labels[k % 2]] for k in range(70)],
            [[0, 0, 9, 9, labels[k % 2], 0.2 + 0.005 * k] for k in range(70)])


def test_ap_sweep_candidate_overflow_is_reported_per_problem(dev):
    gt, pred = cases.seeded(6, 30, 20, 5, 2)
    og, op_ = _overflow_image()
    gt, pred = gt[:3] + [og] + gt[3:], pred[:3] + [op_] + pred[3:]
    pr = metrics.SweepProblems(gt, pred)
    assert pr.N == 4 * 7
    _assert_tables(pr, T10, dev, "overflow", overflowing=(3,))                    # the class-blind problem of image 3, no other
    back = []
    got = metrics.sweep_metrics_device(gt, pred, device=dev, handed_back=back)
    assert back == [3] and metrics.same_sweep(got, metrics.sweep_metrics_host(gt, pred))
    # exactly at the cap: 64 x 64 identical pairs fit
    pr = metrics.SweepProblems([[[0, 0, 9, 9, "s"]] * 64], [[[0, 0, 9, 9, "s", 0.01 * k] for k in range(64)]])
    want = _assert_tables(pr, (0.5, 0.95), dev, "at the cap")
    assert want[:65].tolist() == list(range(64, -1, -1))


def test_problems_past_the_row_caps_stay_on_the_host(dev):
    rng = np.random.default_rng(3)
    big_p, big_g = _crowd(P_CAP + 1, 30, rng), _crowd(20, G_CAP + 1, rng)
    small = _crowd(20, 30, rng)
    gt, pred = [big_p[0], small[0], big_g[0]], [big_p[1], small[1], big_g[1]]
    pr = metrics.SweepProblems(gt, pred)
    with pytest.raises(ops.ApSweepUnsupported):
        _device_tables(pr, T10, dev)
    with pytest.raises(ops.ApSweepUnsupported):
        _device_tables(metrics.SweepProblems(small[:1], small[1:]), tuple(0.3 + 0.01 * k for k in range(T_CAP + 1)), dev)
    back = []
    got = metrics.sweep_metrics_device(gt, pred, device=dev, handed_back=back)
    assert back == [0, 2, 3, 5] and metrics.same_sweep(got, metrics.sweep_metrics_host(gt, pred))
    # more thresholds than one launch takes: several launches, the same numbers
    many = tuple(0.5 + 0.02 * k for k in range(T_CAP + 3))
    assert metrics.same_sweep(metrics.sweep_metrics_device(small[:1], small[1:], iou_thresholds=many, device=dev),
                              metrics.sweep_metrics_host(small[:1], small[1:], iou_thresholds=many))


def test_ap_sweep_empty_and_refused(dev):
    L = _hip.lib()
    t = torch.zeros(64, dtype=torch.float64, device=dev)
    p, s = t.data_ptr(), _hip.current_stream()
    for D, G, N, T in ((1, 1, 0, 1), (-1, 1, 1, 1), (1, -1, 1, 1), (1, 1, 1, 0)):
        assert L.mrcnn_ap_sweep(p, p, D, p, p, G, N, p, T, p, p, s) == -1
    assert L.mrcnn_ap_sweep(None, p, 1, p, p, 1, 1, p, 1, p, p, s) == -1
    assert L.mrcnn_ap_sweep(p, p, 1, p, p, 1, 1, p, 1, p, None, s) == -1
    assert L.mrcnn_ap_sweep(p, p, 1, p, p, 1, 1, p, T_CAP + 1, p, p, s) == ops.ERR_UNSUPPORTED
    up = lambda a: torch.from_numpy(np.asarray(a, np.float64).reshape(-1, 4)).to(dev)
    thr = torch.tensor([0.5], dtype=torch.float64, device=dev)
    for det_off, gt_off in (([0], [0]), ([], []), ([0, 1], [0, 1, 1])):           # no problem, or tables of different lengths
        with pytest.raises(_hip.HipPathError):
            ops.ap_sweep(up([cases.B10]), det_off, up([cases.B10]), gt_off, thr)
    for det_off, gt_off in (([0, 2], [0, 1]), ([1, 1], [0, 1]), ([0, 1, 0, 1], [0, 0, 0, 1]), ([0, 1], [0, 0])):
        with pytest.raises(_hip.HipPathError):
            ops.ap_sweep(up([cases.B10]), det_off, up([cases.B10]), gt_off, thr)
    with pytest.raises(_hip.HipPathError):
        ops.ap_sweep(up([cases.B10]), [0, 1], up([cases.B10]), [0, 1], thr[:0])
    # problems without a row are problems: their tables are the single 0 per threshold
    tp, status = ops.ap_sweep(up([]), [0, 0, 0], up([cases.B10]), [0, 0, 1], thr)
    assert tp.cpu().tolist() == [0, 0] and status.cpu().tolist() == [0, 0]
    tp, status = ops.ap_sweep(up([cases.B10]), [0, 1, 1], up([]), [0, 0, 0], thr)
    assert tp.cpu().tolist() == [0, 0, 0] and status.cpu().tolist() == [0, 0]
    for gt, pred in (([], []), ([[], []], [[], []]), ([[cases.B10 + ["galaxy"]]], [[]])):
        assert metrics.same_sweep(metrics.sweep_metrics_device(gt, pred, device=dev), metrics.sweep_metrics_host(gt, pred))


def test_sweep_metrics_device_seeded_set(dev):
    """30 seeded images of three classes, equal scores frequent: every problem is computed on the device."""
    gt, pred = cases.seeded(30, 40, 25, 77, 2)
    assert sum(map(len, pred)) > 300 and len(set(r[4] for img in pred for r in img)) == 3
    back = []
    got = metrics.sweep_metrics_device(gt, pred, device=dev, handed_back=back)
    want = metrics.sweep_metrics_host(gt, pred)
    assert back == [] and metrics.same_sweep(got, want)
    assert want["results"][0]["avg_prec"] > want["results"][9]["avg_prec"] >= 0 and want["results"][0]["precisions"].size > 50
    assert metrics.format_sweep(got) == metrics.format_sweep(want)
    gt, pred = cases.seeded(8, 30, 20, 78, 1, grid=8)                            # tied IoUs throughout
    back = []
    assert metrics.same_sweep(metrics.sweep_metrics_device(gt, pred, device=dev, handed_back=back), metrics.sweep_metrics_host(gt, pred))
    assert back == []


def test_sweep_metrics_selects_by_size(dev, monkeypatch):
    gt, pred = cases.seeded(10, 20, 15, 9, 2)
    calls = []
    real = ops.ap_sweep
    monkeypatch.setattr(ops, "ap_sweep", lambda *a, **k: calls.append(1) or real(*a, **k))
    n = sum(map(len, pred))
    for constant in (None, n + 1):
        monkeypatch.setattr(metrics, "SWEEP_DEVICE_MIN_DETECTIONS", constant)
        a = metrics.sweep_metrics(gt, pred)
        assert calls == []
    monkeypatch.setattr(metrics, "SWEEP_DEVICE_MIN_DETECTIONS", n)
    b = metrics.sweep_metrics(gt, pred)
    assert calls == [1] and metrics.same_sweep(a, b)


# ---- ModelTester.test() with compute_mAP_metrics and sweep_map on a real model ----------------------------------------------
def test_model_tester_sweep_map_real_model(dev, tmp_path, monkeypatch):
    """A MaskRCNN with seeded random weights through ModelTester.test() with compute_mAP_metrics and sweep_map: the sweep from the
    device equals the host's, the printed block ends in the tool's lines, and without sweep_map nothing of it appears."""
    import model_cases as T
    import analyze_post_cases as post
    import test_map_gpu as MG
    import test_tester_gpu as TG
    from caesar_mrcnn_amd.model import MaskRCNN
    cfg = T._small_cfg("custom", 128, mode="inference")
    cfg.CLASS_NAMES = list(post.CLASS_NAMES)
    model = MaskRCNN("inference", cfg, "/tmp/mrcnn_logs", device=dev, weights=T._weights(cfg, 3))
    images = [im.astype(np.float32) for im in T._scene(cfg, 2, 7)[0]]
    paths, gts, ids = [], [], []
    for k, image in enumerate(images):
        paths.append(str(tmp_path / ("scene%d.fits" % k)))
        TG._scene_image((128, 128), paths[-1])
        first = model.detect([image], verbose=0)[0]
        n = min(first["masks"].shape[-1], 3)
        assert n >= 1
        gts.append(np.concatenate([first["masks"][:, :, :n], post.rect((128, 128), 100, 110, 5, 25)[:, :, None]], axis=-1).astype(bool))
        c = [int(v) for v in first["class_ids"][:n]] + [1]
        c[0] = 1 + c[0] % (cfg.NUM_CLASSES - 1)
        ids.append(c)
    monkeypatch.chdir(tmp_path)
    launches = []
    real = ops.ap_sweep
    monkeypatch.setattr(ops, "ap_sweep", lambda *a, **k: launches.append(1) or real(*a, **k))

    def run(sweep_map, device):
        monkeypatch.setattr(metrics, "SWEEP_DEVICE_MIN_DETECTIONS", 0 if device else None)
        ds = MG._TwoImages(images, paths, gts, ids, cfg.CLASS_NAMES, dict(tcases.META, nx=128, ny=128))
        tester = analyze.ModelTester(model, cfg, ds)
        tester.score_thr, tester.compute_mAP_metrics, tester.sweep_map = 0.0, True, sweep_map
        tester.outfilename_completeness, tester.outfilename_reliability = "c.csv", "r.csv"
        out = io.StringIO()
        with contextlib.redirect_stdout(out):
            assert tester.test() == 0
        return tester, out.getvalue()
    t_dev, out_dev = run(True, True)
    assert launches == [1]
    t_host, out_host = run(True, False)
    t_off, out_off = run(False, True)
    assert launches == [1] and t_off.sweep is None
    assert metrics.same_sweep(t_dev.sweep, t_host.sweep) and out_dev == out_host
    assert len(t_dev.sweep["thresholds"]) == 10 and len(t_dev.sweep["classes"]) >= 1
    tail = "".join(l + "\n" for l in metrics.format_sweep(t_dev.sweep))
    assert out_dev == out_off + tail and "map: " not in out_off
    # a random-weight model's detections may share one score (no model threshold, every AP 0): the same testers' compute_mAP on
    # rows with a curve to get wrong
    gt, pred = cases.seeded(2, 30, 20, 21, 2)
    sweeps = []
    for tester, constant in ((t_dev, 0), (t_host, None)):
        monkeypatch.setattr(metrics, "SWEEP_DEVICE_MIN_DETECTIONS", constant)
        with contextlib.redirect_stdout(io.StringIO()):
            assert tester.compute_mAP(gt, pred) == 0
        sweeps.append(tester.sweep)
    assert launches == [1, 1] and metrics.same_sweep(*sweeps) and metrics.same_sweep(sweeps[0], metrics.sweep_metrics_host(gt, pred))
    assert sweeps[0]["results"][0]["precisions"].size >= 10 and sweeps[0]["results"][0]["avg_prec"] > 0
