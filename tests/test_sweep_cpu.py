"""The sweep mAP (metrics.sweep_metrics_host, sweep_tables_host, format_sweep) against tests/golden/sweep.npz -- the reference's
vendored tarlen5-calculate-mean-ap tool, recorded by tests/golden/make_sweep_fixtures.py -- and against a brute-force statement
of the tool's loop; ModelTester.compute_mAP and run.py with and without the sweep.  No GPU."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import map_cases as mcases                                  # noqa: E402
import sweep_cases as cases                                 # noqa: E402
import tester_cases as tcases                               # noqa: E402
from caesar_mrcnn_amd import _hip, analyze, datagen, metrics, ops, utils   # noqa: E402

GOLDEN = np.load(cases.GOLDEN)
SETS = cases.golden_sets(GOLDEN)
PINNED = [s for s in SETS if not cases.load(GOLDEN, s)[2]]
TIED = [s for s in SETS if cases.load(GOLDEN, s)[2]]


def test_fixture_holds_the_sets():
    built = cases.sets()
    assert SETS == sorted(built) and len(PINNED) >= 6 and len(TIED) >= 2
    for name, (gt, pred, tied) in built.items():
        g, p, t, classes, rec, lines = cases.load(GOLDEN, name)
        assert (g, p, t) == (json.loads(json.dumps(gt)), json.loads(json.dumps(pred)), tied), name
        assert cases.has_tied_ious(gt, pred, metrics.sweep_iou_matrix) == tied, name
        assert (lines is not None) == (name in cases.MAIN_SETS), name
        assert len(gt) <= 20 and max(map(len, pred)) <= 70 and max(map(len, gt)) <= 40, name
    assert bool(GOLDEN["malformed/raises"][0])
    # what the sets are there for
    gt, pred = built["seeded_small"][:2]
    assert any(not g for g in gt) and any(not p for p in pred)
    scores = [r[5] for img in pred for r in img]
    assert len(set(scores)) < len(scores) and any(len(set(r[5] for r in img)) < len(img) for img in pred if img)
    assert cases.load(GOLDEN, "one_score")[4]["t0/precisions"].size == 0 and cases.load(GOLDEN, "one_score")[4]["t0/avg_prec"][0] == 0.0
    assert cases.load(GOLDEN, "no_detections")[4]["mAP"][0] == 0.0


@pytest.mark.parametrize("name", PINNED)
def test_sweep_metrics_host_equals_the_tool(name):
    gt, pred, _, classes, want, _ = cases.load(GOLDEN, name)
    got = metrics.sweep_metrics_host(gt, pred)
    assert got["classes"] == classes and got["thresholds"] == list(cases.IOU_THRESHOLDS) and got["class_thresholds"] == [0.5, 0.6]
    assert cases.differences(cases.record(got), want) == [], name


@pytest.mark.parametrize("name", TIED)
def test_tied_sets_follow_the_stable_order(name):
    """Bit-equal IoUs within an image: the tool's order is NumPy's unstable sort's, the record is one machine's.  The host
    statement must equal the tool's loop with np.argsort(kind="stable")[::-1]; how it compares with the record is reported."""
    gt, pred, _, _, want, _ = cases.load(GOLDEN, name)
    got = metrics.sweep_metrics_host(gt, pred)
    assert metrics.same_sweep(got, cases.brute_result(gt, pred)), name
    print("%s against the recorded tool output (its order of equal IoUs is not defined): differs at %s" % (
        name, cases.differences(cases.record(got), want) or "nothing"))


@pytest.mark.parametrize("name", PINNED)
def test_host_equals_the_tools_loop_by_brute_force(name):
    gt, pred = cases.load(GOLDEN, name)[:2]
    brute = cases.brute_result(gt, pred)
    assert metrics.same_sweep(metrics.sweep_metrics_host(gt, pred), brute)
    assert not metrics.same_sweep(metrics.sweep_metrics_host(gt, pred, iou_thresholds=cases.IOU_THRESHOLDS[:9]), brute)


@pytest.mark.parametrize("name", SETS)
def test_suffix_tables_equal_every_suffix_matched_alone(name):
    gt, pred = cases.load(GOLDEN, name)[:2]
    pr = metrics.SweepProblems(gt, pred)
    assert pr.N == (1 + len(pr.classes)) * len(gt) and pr.det_off[-1] == pr.D and pr.gt_off[-1] == pr.G
    assert pr.D == (2 if pr.classes else 1) * sum(map(len, pred))                # every row once class-blind and once under its class
    for p in range(pr.N):
        s = pr.det_score[pr.det_off[p]:pr.det_off[p + 1]]
        assert bool(np.all(s[1:] >= s[:-1]))
    thr = cases.IOU_THRESHOLDS
    tp, status = metrics.sweep_tables_host(pr, thr)
    assert tp.dtype == np.int32 and tp.shape == (len(thr) * (pr.D + pr.N),) and status.tolist() == [0] * pr.N
    assert np.array_equal(tp, cases.brute_tables(pr, thr))
    start, rows = metrics.sweep_table_entries(pr, len(thr))
    assert all(tp[start[p] + t * rows[p] + rows[p] - 1] == 0 for p in range(pr.N) for t in range(len(thr)))
    only = [p for p in range(pr.N) if p % 2]
    part, _ = metrics.sweep_tables_host(pr, thr, only=only)
    for p in range(pr.N):
        seg = slice(start[p], start[p] + len(thr) * rows[p])
        assert np.array_equal(part[seg], tp[seg]) if p in only else not part[seg].any()


def test_format_sweep_prints_the_tools_lines():
    for name in cases.MAIN_SETS:
        gt, pred, _, _, _, lines = cases.load(GOLDEN, name)
        got = metrics.format_sweep(metrics.sweep_metrics_host(gt, pred), classes=cases.LABELS)
        assert got == lines, (name, got, lines)
        assert [l.split(":")[0] for l in got] == ["Source avg precision", "Sidelobe avg precision", "Galaxy avg precision", "avg precision",
                                                  "map", "avg precs", "iou_thrs", "map", "avg precs", "iou_thrs"]
        assert got[6] == "iou_thrs:   [0.5, 0.55, 0.6, 0.65, 0.7, 0.75, 0.8, 0.85, 0.9, 0.95]" and got[9] == "iou_thrs:   [0.5, 0.6, 0.5, 0.6, 0.5, 0.6]"
    # the default order is the result's sorted labels; a label the data does not hold has AP 0
    r = metrics.sweep_metrics_host(*cases.sets()["equal_scores"][:2])
    assert r["classes"] == ["source"]
    lines = metrics.format_sweep(r)
    assert lines[0] == "Source avg precision: %.4f" % r["per_class"]["source"][0]["avg_prec"] and len(lines) == 8
    assert metrics.format_sweep(r, classes=("galaxy", "source"))[0] == "Galaxy avg precision: 0.0000"


def test_the_rules_on_rows_whose_answer_can_be_read_off():
    s = "source"
    # IoU exactly 0.5 is no candidate at 0.5 (`>`); exactly 0.6 is one at 0.5 and 0.55, not at 0.6
    assert metrics.sweep_iou_matrix(np.array([[0., 0, 9, 4]]), np.array([[0., 0, 9, 9]]))[0, 0] == 0.5
    pr = metrics.SweepProblems([[cases.B10 + [s]]], [[cases.inside(5) + [s, 0.9], cases.inside(6) + [s, 0.8]]])
    tp, _ = metrics.sweep_tables_host(pr, (0.5, 0.55, 0.6))
    assert pr.det_score[:2].tolist() == [0.8, 0.9]                                # ascending: row 0 is the 10 x 6 box
    assert tp[:9].reshape(3, 3).tolist() == [[1, 0, 0], [1, 0, 0], [0, 0, 0]]
    # boxes that share one pixel row overlap (10 / 160), boxes one pixel apart do not
    iou = metrics.sweep_iou_matrix(np.array([[9., 0, 15, 9], [10., 0, 15, 9]]), np.array([[0., 0, 9, 9]]))
    assert iou[:, 0].tolist() == [10.0 / 160.0, 0.0]
    # this is not the VOC tool's IoU renamed: the arguments of the division are the same, the statement is the tool's own
    assert metrics.sweep_iou_matrix is not metrics.box_iou_matrix
    # tied IoUs: the later-enumerated pair first costs a match here
    gt, pred, _ = cases.sets()["tied_pairs"]
    pr = metrics.SweepProblems(gt, pred)
    tp, _ = metrics.sweep_tables_host(pr, (0.5,))
    assert pr.det_score[:4].tolist() == [0.3, 0.6, 0.8, 0.9] and tp[:5].tolist() == [2, 1, 1, 0, 0]    # k = 1: rows 1 and 2 find one
    boxes = pr.det_box[1:3].tolist()
    other = [cases.iou_one(b, g[:4]) for b in boxes for g in gt[0]]
    assert other[0] == other[1] > other[3] > 0.5 > other[2]                        # the earlier pair first would find two matches
    # fewer than two distinct scores: no point, AP 0
    r = metrics.sweep_metrics_host(*cases.sets()["one_score"][:2])
    assert r["mAP"] == 0.0 and r["results"][0]["model_thrs"] == [] and r["results"][0]["precisions"].shape == (0,)
    r = metrics.sweep_metrics_host([], [])
    assert r["classes"] == [] and r["mAP"] == 0.0 and r["per_class"] == {}


def test_argument_errors():
    gt, pred = cases.MALFORMED
    with pytest.raises(ValueError):
        metrics.sweep_metrics_host(gt, pred)
    with pytest.raises(ValueError):
        metrics.sweep_metrics_host([[[0, 5, 9, 4, "source"]]], [[]])
    with pytest.raises(ValueError):
        metrics.sweep_metrics_host([[]], [[[0, 0, float("nan"), 4, "source", 0.5]]])
    with pytest.raises(ValueError):
        metrics.sweep_metrics_host([[]], [[[0, 0, 9, 4, "source", float("inf")]]])
    with pytest.raises(ValueError):
        metrics.sweep_metrics_host([[]], [[], []])
    good = cases.sets()["equal_scores"][:2]
    for kw in ({"iou_thresholds": (0.0, 0.5)}, {"iou_thresholds": ()}, {"class_thresholds": (-0.5,)}):
        with pytest.raises(ValueError):
            metrics.sweep_metrics_host(*good, **kw)
    # ops.ap_sweep refuses host tensors before it touches the library
    import torch
    z = torch.zeros((0, 4), dtype=torch.float64)
    with pytest.raises(_hip.HipPathError):
        ops.ap_sweep(z, [0, 0], z, [0, 0], torch.tensor([0.5], dtype=torch.float64))
    assert issubclass(ops.ApSweepUnsupported, _hip.HipPathError)


def test_sweep_metrics_takes_the_host_form(monkeypatch):
    import torch
    gt, pred = cases.sets()["hand_mixed"][:2]
    want = metrics.sweep_metrics_host(gt, pred)
    monkeypatch.setattr(metrics, "sweep_metrics_device", lambda *a, **k: pytest.fail("the device form"))
    assert sum(map(len, pred)) < metrics.SWEEP_DEVICE_MIN_DETECTIONS                # below the measured break-even
    assert metrics.same_sweep(metrics.sweep_metrics(gt, pred), want)
    monkeypatch.setattr(metrics, "SWEEP_DEVICE_MIN_DETECTIONS", 0)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)                # at any size without a GPU
    assert metrics.same_sweep(metrics.sweep_metrics(gt, pred), want)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(metrics, "SWEEP_DEVICE_MIN_DETECTIONS", None)             # None: never
    assert metrics.same_sweep(metrics.sweep_metrics(gt, pred), want)


@pytest.mark.parametrize("caps", [{"det": 128, "gt": 320, "thr": 16, "cand": 4096}, {"det": 6, "gt": 5, "thr": 4, "cand": 4096}])
def test_device_form_sums_with_tables_from_the_host_statement(monkeypatch, caps):
    """The device form's plumbing on CPU tensors: ops.ap_sweep replaced by the host statement (the kernel itself is compared in
    tests/test_sweep_gpu.py).  With small caps most problems are kept back, the thresholds go in three launches, and one sent
    problem comes back with its status set."""
    import torch
    gt, pred = cases.sets()["seeded_small"][:2]
    sent = []

    def fake(det_box, det_off, gt_box, gt_off, thr):
        pr = object.__new__(metrics.SweepProblems)
        pr.det_box, pr.gt_box, pr.det_off, pr.gt_off = det_box.numpy(), gt_box.numpy(), np.asarray(det_off), np.asarray(gt_off)
        pr.N, pr.D, pr.G = len(det_off) - 1, int(det_off[-1]), int(gt_off[-1])
        assert np.diff(pr.det_off).max() <= caps["det"] and np.diff(pr.gt_off).max() <= caps["gt"] and len(thr) <= caps["thr"]
        tp, status = metrics.sweep_tables_host(pr, thr.numpy())
        start, rows = metrics.sweep_table_entries(pr, len(thr))
        tp[start[1]:start[1] + len(thr) * rows[1]] = 0
        status[1] = ops.AP_SWEEP_OVER_CANDIDATES
        sent.append(pr.N)
        return torch.from_numpy(tp), torch.from_numpy(status)
    monkeypatch.setattr(ops, "ap_sweep", fake)
    monkeypatch.setattr(ops, "ap_sweep_caps", lambda: dict(caps))
    back = []
    got = metrics.sweep_metrics_device(gt, pred, device=torch.device("cpu"), handed_back=back)
    assert metrics.same_sweep(got, metrics.sweep_metrics_host(gt, pred))
    pr = metrics.SweepProblems(gt, pred)
    over = np.flatnonzero((np.diff(pr.det_off) > caps["det"]) | (np.diff(pr.gt_off) > caps["gt"]))
    assert len(sent) == -(-10 // caps["thr"]) and sent[0] == pr.N - over.size
    assert len(back) == over.size + 1 and set(over.tolist()) < set(back) and (over.size > 0) == (caps["det"] == 6)


# ---- ModelTester.compute_mAP ---------------------------------------------------------------------------------------------
def _tester(monkeypatch):
    monkeypatch.setattr(datagen, "load_image_gt", mcases.map_image_gt(utils.extract_bboxes))
    ds = mcases.MapDataset()
    tester = analyze.ModelTester(mcases.MapModel(utils.extract_bboxes), tcases.cfg(), ds)
    tester.iou_thr = 0.6
    tester.inspected = [(i, ds.image_info[i]["path"]) for i in ds.image_ids]
    return tester


def test_compute_map_with_and_without_the_sweep(monkeypatch, tmp_path, capsys):
    map_golden = np.load(mcases.GOLDEN)
    files = {str(n): map_golden["compute_map/file%d" % k].tobytes() for k, n in enumerate(map_golden["compute_map/files"])}
    tester = _tester(monkeypatch)
    assert tester.sweep_map is False and tester.sweep is None
    monkeypatch.setattr(metrics, "sweep_metrics", lambda *a, **k: pytest.fail("the sweep without sweep_map"))
    tester.metrics_outdir = str(tmp_path / "plain")
    assert tester.compute_mAP(mcases.MAP_GT, mcases.MAP_PRED) == 0
    plain = capsys.readouterr().out
    assert tester.sweep is None and mcases.tree_bytes(tester.metrics_outdir) == files
    # the block as it was: the header, the mask mAP, per threshold the classes' lines and the VOC mAP -- and nothing else
    lines = plain.splitlines()
    assert lines[:2] == ["== Mean AveragePrecision (mAP) ==", "mAP=%f" % tester.mAP] and len(lines) == 2 + 2 * (3 + 1)
    assert all(l.startswith("VOC IoU>=") for l in lines[2:])
    monkeypatch.undo()
    tester = _tester(monkeypatch)
    tester.sweep_map, tester.metrics_outdir = True, str(tmp_path / "sweep")
    assert tester.compute_mAP(mcases.MAP_GT, mcases.MAP_PRED) == 0
    out = capsys.readouterr().out
    want = metrics.sweep_metrics_host(mcases.MAP_GT, mcases.MAP_PRED)
    assert metrics.same_sweep(tester.sweep, want) and tester.sweep["classes"] == ["compact", "extended", "spurious"]
    assert out == plain + "".join(l + "\n" for l in metrics.format_sweep(want))
    assert "Compact avg precision: " in out and out.count("map: ") == 2
    assert mcases.tree_bytes(tester.metrics_outdir) == files


# ---- run.py ------------------------------------------------------------------------------------------------------------------
def test_cli_flag(tmp_path, monkeypatch, capsys):
    import test_tester_cpu as TT
    run = TT._run_py()
    base = ["test", "--imgsize", "33", "--classdict", TT.CLASSDICT]
    assert run.parse_args(base + ["--reference_tester", "--compute_map"]).sweep_map is False
    assert run.parse_args(base + ["--reference_tester", "--compute_map", "--sweep_map"]).sweep_map is True
    for bad in (base + ["--sweep_map"], base + ["--reference_tester", "--sweep_map"], base + ["--compute_map", "--sweep_map"],
                ["detect", "--imgsize", "33", "--classdict", TT.CLASSDICT, "--reference_tester", "--compute_map", "--sweep_map"]):
        with pytest.raises(SystemExit):
            run.parse_args(bad)
    capsys.readouterr()
    model = TT._SceneModel()
    tmp = str(tmp_path)
    made = [TT._write_scene(tmp, k, model) for k in range(2)]
    with open(os.path.join(tmp, "json.dat"), "w") as fp:
        for _, _, jpath, _, _ in made:
            fp.write(jpath + "\n")
    monkeypatch.chdir(tmp)
    common = ["--reference_tester", "--dataloader", "datalist_json", "--datalist", os.path.join(tmp, "json.dat"), "--compute_map"]
    args = run.parse_args(base + common)
    assert run.test(args, model, run.build_config(args, json.loads(TT.CLASSDICT))) == 0
    plain = capsys.readouterr().out
    assert "avg precision" not in plain and "map: " not in plain
    args = run.parse_args(base + common + ["--sweep_map"])
    assert run.test(args, model, run.build_config(args, json.loads(TT.CLASSDICT))) == 0
    out = capsys.readouterr().out
    assert out.startswith(plain)
    tail = out[len(plain):].splitlines()
    assert tail[-6].startswith("map: ") and tail[-5].startswith("avg precs:  [") and tail[-1] == "iou_thrs:   " + str([0.5, 0.6] * ((len(tail) - 7)))
    assert tail[len(tail) - 7] .startswith("avg precision: ") and all(" avg precision: " in l for l in tail[:len(tail) - 7])
