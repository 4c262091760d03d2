"""metrics.py, utils.compute_ap_range and ModelTester.compute_mAP against tests/golden/map.npz -- the vendored Pascal-VOC tool,
``compute_ap_range`` and ``compute_mAP`` of the reference, recorded by tests/golden/make_map_fixtures.py -- without a GPU."""
import contextlib
import io
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import map_cases as cases                                   # noqa: E402
import tester_cases as tcases                               # noqa: E402
from caesar_mrcnn_amd import analyze, datagen, metrics, utils   # noqa: E402

GOLDEN = np.load(cases.GOLDEN)
CASES = cases.golden_cases(GOLDEN)


def test_fixture_holds_the_cases():
    assert ["sample_" + f for f in cases.SAMPLE_FORMATS] == [c for c in CASES if c.startswith("sample_")]
    assert sorted("hand_" + n for n in cases.hand_cases()) == [c for c in CASES if c.startswith("hand_")]
    gt, pred, classes, thr, rec = cases.load(GOLDEN, "sample_xywh")
    assert (len(gt), sum(map(len, gt)), sum(map(len, pred))) == (11, 41, 47) and classes == ["galaxy", "source"] and thr == [0.5, 0.6]
    # the tool's own numbers on its sample files (the results file it ships rounds them to 57.14 % and 63.22 %)
    assert [rec["t0/galaxy/" + k][0] for k in ("total positives", "total TP", "total FP")] == [14, 8, 0]
    assert [rec["t0/source/" + k][0] for k in ("total positives", "total TP", "total FP")] == [27, 20, 19]
    assert round(rec["t0/galaxy/AP"][0], 4) == 0.5714 and round(rec["t0/source/AP"][0], 4) == 0.6322
    # the hand-built rows in the fixture are the ones of map_cases.py
    for name, (g, p) in cases.hand_cases().items():
        assert cases.load(GOLDEN, "hand_" + name)[:2] == (json.loads(json.dumps(g)), json.loads(json.dumps(p))), name


@pytest.mark.parametrize("case", CASES)
def test_voc_metrics_host_equals_the_tool(case):
    gt, pred, classes, thr, want = cases.load(GOLDEN, case)
    got = metrics.voc_metrics_host(gt, pred, thr)
    assert got["classes"] == classes and got["thresholds"] == thr
    cases.assert_record(cases.record(got), want, case)


def test_the_three_rules():
    hand = cases.hand_cases()
    r = metrics.voc_metrics_host(*hand["iou_exact"], iou_thresholds=cases.THRESHOLDS)
    g5, g6 = r["results"][0]["classes"]["galaxy"], r["results"][1]["classes"]["galaxy"]
    assert g5["TP"].tolist() == [1, 1] and g6["TP"].tolist() == [0, 1]          # IoU 0.5 at 0.5 and IoU 0.6 at 0.6 are TP: `>=`
    r = metrics.voc_metrics_host(*hand["gt_only_class"])["results"][0]
    assert r["classes"]["source"]["AP"] == 0 and r["classes"]["source"]["total positives"] == 1 and r["mAP"] == 0.5
    r = metrics.voc_metrics_host(*hand["det_only_class"])["results"][0]
    assert np.isnan(r["classes"]["source"]["AP"]) and r["classes"]["source"]["total FP"] == 1 and r["mAP"] == 1.0
    with pytest.raises(ValueError):
        metrics.voc_metrics_host(*hand["twin_gts"], iou_thresholds=(0.0,))
    with pytest.raises(ValueError):
        metrics.voc_metrics_host([[]], [[], []])


def test_voc_match_host_statement():
    """Best ground truth, its IoU and the flags per detection, on rows whose answer can be read off."""
    gt, pred = cases.hand_cases()["twin_gts"]
    flat = metrics.Flat(gt, pred)
    best_gt, best_iou, tp = metrics.voc_match_host(flat, (0.5,))
    assert best_gt.tolist() == [0, 0] and best_iou.tolist() == [1.0, 1.0] and tp.tolist() == [[1, 0]]
    flat = metrics.Flat(*cases.hand_cases()["edge_pixel"])
    best_gt, best_iou, tp = metrics.voc_match_host(flat, (0.5,))
    assert best_gt.tolist() == [0] and best_iou[0] == 1.0 / (100.0 + 49.0 - 1.0) and tp.tolist() == [[0]]
    flat = metrics.Flat(*cases.hand_cases()["apart"])
    best_gt, best_iou, tp = metrics.voc_match_host(flat, (0.5,))
    assert best_gt.tolist() == [-1] and best_iou.tolist() == [0.0]
    # the later row with the higher score takes the ground truth
    flat = metrics.Flat(*cases.hand_cases()["twin_scores"])
    assert metrics.voc_match_host(flat, (0.5, 0.6))[2].tolist() == [[0, 1], [0, 1]]
    flat = metrics.Flat(*cases.hand_cases()["twin_equal"])
    assert metrics.voc_match_host(flat, (0.5, 0.7))[2].tolist() == [[1, 0], [0, 1]]     # at 0.7 the first one (IoU 0.6) claims nothing


def test_voc_metrics_takes_the_host_form_without_a_gpu(monkeypatch):
    import torch
    gt, pred = cases.hand_cases()["all"]
    monkeypatch.setattr(metrics, "DEVICE_MIN_DETECTIONS", 0)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    monkeypatch.setattr(metrics, "voc_metrics_device", lambda *a, **k: pytest.fail("device form without a GPU"))
    assert metrics.same_metrics(metrics.voc_metrics(gt, pred, cases.THRESHOLDS), metrics.voc_metrics_host(gt, pred, cases.THRESHOLDS))


def _golden_files():
    names = [str(n) for n in GOLDEN["compute_map/files"]]
    return {n: GOLDEN["compute_map/file%d" % k].tobytes() for k, n in enumerate(names)}


def test_write_metric_files_bytes(tmp_path):
    out = str(tmp_path / "deep" / "er")
    written = metrics.write_metric_files(cases.MAP_GT, cases.MAP_PRED, list(cases.MAP_PATHS), out)
    got, want = cases.tree_bytes(out), _golden_files()
    assert sorted(got) == sorted(want) and len(written) == len(want) == 8
    for name in sorted(want):
        assert got[name] == want[name], name
    assert sorted(os.listdir(out)) == ["Object-Detection-Metrics", "metric-computation", "tarlen5-calculate-mean-ap"]


def test_compute_ap_range_equals_the_reference(capsys):
    names, values = [str(n) for n in GOLDEN["ap_range/names"]], GOLDEN["ap_range/values"]
    assert names == [sc["name"] for sc in cases.ap_scenes()] and len(names) >= 10
    for name, want in zip(names, values):
        args = cases.ap_inputs(tcases.scenario(name), utils.extract_bboxes)
        with np.errstate(divide="ignore", invalid="ignore"):
            got = utils.compute_ap_range(*args, verbose=0)
        assert got == want or (np.isnan(got) and np.isnan(want)), (name, got, want)
    assert capsys.readouterr().out == ""
    utils.compute_ap_range(*cases.ap_inputs(tcases.scenario("thr_exact"), utils.extract_bboxes), iou_thresholds=[0.5, 0.75])
    assert capsys.readouterr().out == "AP @0.50:\t 1.000\nAP @0.75:\t 0.000\nAP @0.50-0.75:\t 0.500\n"


@pytest.mark.parametrize("sc", cases.ap_scenes(), ids=lambda s: s["name"])
def test_compute_ap_with_given_overlaps(sc, monkeypatch):
    args = cases.ap_inputs(sc, utils.extract_bboxes)
    want = utils.compute_ap(*args, iou_threshold=0.6)
    M = want[3]
    monkeypatch.setattr(utils, "compute_overlaps_masks", lambda *a: pytest.fail("the full-frame product was formed"))
    got = utils.compute_ap(*args, iou_threshold=0.6, overlaps=M)
    for a, b in zip(got, want):
        assert np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)
    m_got, m_want = utils.compute_matches(*args, iou_threshold=0.6, overlaps=M), None
    monkeypatch.undo()
    m_want = utils.compute_matches(*args, iou_threshold=0.6)
    for a, b in zip(m_got, m_want):
        assert np.array_equal(a, b, equal_nan=True)
    assert utils.compute_ap_range(*args, verbose=0, overlaps=M) == utils.compute_ap_range(*args, verbose=0)
    if M.size:
        with pytest.raises(AssertionError):
            utils.compute_ap(*args, overlaps=M[:, :-1])


# ---- ModelTester.compute_mAP --------------------------------------------------------------------------------------------
def _tester(monkeypatch):
    monkeypatch.setattr(datagen, "load_image_gt", cases.map_image_gt(utils.extract_bboxes))
    model = cases.MapModel(utils.extract_bboxes)
    ds = cases.MapDataset()
    tester = analyze.ModelTester(model, tcases.cfg(), ds)
    tester.iou_thr = 0.6
    tester.inspected = [(i, ds.image_info[i]["path"]) for i in ds.image_ids]
    return tester, model


def test_compute_map_with_a_stand_in_model(monkeypatch, tmp_path, capsys):
    tester, model = _tester(monkeypatch)
    assert tester.compute_mAP_metrics is False and tester.metrics_outdir is None and tester.APs == [] and tester.voc is None
    monkeypatch.chdir(tmp_path)
    assert tester.compute_mAP(cases.MAP_GT, cases.MAP_PRED) == 0
    out = capsys.readouterr().out
    # the reference's loop stops after the first image: its mAP is the first entry here
    assert model.calls == 2 and len(tester.APs) == 2 and tester.APs[0] == GOLDEN["compute_map/mAP"][0]
    for k, name in enumerate(cases.MAP_IMAGES):
        assert tester.APs[k] == utils.compute_ap(*cases.ap_inputs(tcases.scenario(name), utils.extract_bboxes), iou_threshold=0.6)[0]
    assert tester.mAP == np.mean(tester.APs)
    assert metrics.same_metrics(tester.voc, metrics.voc_metrics_host(cases.MAP_GT, cases.MAP_PRED, (0.5, 0.6)))
    assert tester.voc["thresholds"] == [0.5, 0.6] and tester.voc["classes"] == ["compact", "extended", "spurious"]
    lines = out.splitlines()
    ref_lines = GOLDEN["compute_map/printed"].tobytes().decode().splitlines()
    assert ref_lines[0] == "== Mean AveragePrecision (mAP) ==" and lines[0] == ref_lines[0] and lines[1] == "mAP=%f" % tester.mAP
    assert ref_lines[1] == "mAP=%f" % tester.APs[0]
    assert sum(l.startswith("VOC IoU>=0.50 class ") for l in lines) == 3 and "VOC IoU>=0.60 mAP=%f" % tester.voc["results"][1]["mAP"] in lines
    assert os.listdir(str(tmp_path)) == []                                        # nothing written unless a directory is named
    tester.metrics_outdir = str(tmp_path / "out")
    tester.compute_mAP(cases.MAP_GT, cases.MAP_PRED)
    assert cases.tree_bytes(tester.metrics_outdir) == _golden_files()


def test_test_calls_compute_map_between_performances_and_save(monkeypatch):
    tester, model = _tester(monkeypatch)
    order = []

    def inspect(self, image_id, image_path):
        self.gt_data.append(cases.MAP_GT[image_id])
        self.pred_data.append(cases.MAP_PRED[image_id])
        return 0 if image_id == 0 else -1
    monkeypatch.setattr(analyze.Analyzer, "inspect_results", inspect)
    monkeypatch.setattr(analyze.ModelTester, "update_performances", lambda self, an: order.append("update"))
    monkeypatch.setattr(analyze.ModelTester, "compute_performances", lambda self: order.append("performances"))
    monkeypatch.setattr(analyze.ModelTester, "save", lambda self: order.append("save"))
    real = analyze.ModelTester.compute_mAP

    def spy(self, gt_data, pred_data):
        order.append("map")
        assert gt_data == cases.MAP_GT and pred_data == cases.MAP_PRED
        return real(self, gt_data, pred_data)
    monkeypatch.setattr(analyze.ModelTester, "compute_mAP", spy)
    with contextlib.redirect_stdout(io.StringIO()):
        assert tester.test() == 0
    assert order == ["update", "performances", "save"] and tester.voc is None
    del order[:]
    tester.compute_mAP_metrics = True
    with contextlib.redirect_stdout(io.StringIO()):
        assert tester.test() == 0
    assert order == ["update", "performances", "map", "save"]
    assert tester.inspected == [(0, cases.MAP_PATHS[0])] and len(tester.APs) == 1 and tester.voc is not None


# ---- run.py ------------------------------------------------------------------------------------------------------------------
def test_cli_flags(tmp_path, monkeypatch, capsys):
    import test_tester_cpu as TT
    run = TT._run_py()
    base = ["test", "--imgsize", "33", "--classdict", TT.CLASSDICT]
    args = run.parse_args(base + ["--reference_tester"])
    assert args.compute_map is False and args.map_outdir == ""
    args = run.parse_args(base + ["--reference_tester", "--compute_map", "--map_outdir", "m"])
    assert args.compute_map is True and args.map_outdir == "m"
    for bad in (base + ["--compute_map"], base + ["--map_outdir", "m"], base + ["--reference_tester", "--map_outdir", "m"],
                ["detect", "--imgsize", "33", "--classdict", TT.CLASSDICT, "--reference_tester", "--compute_map"]):
        with pytest.raises(SystemExit):
            run.parse_args(bad)
    capsys.readouterr()
    # the reference tester on two planted scenes: the block is printed after the tables and the files land where they are sent
    model = TT._SceneModel()
    tmp = str(tmp_path)
    made = [TT._write_scene(tmp, k, model) for k in range(2)]
    with open(os.path.join(tmp, "json.dat"), "w") as fp:
        for _, _, jpath, _, _ in made:
            fp.write(jpath + "\n")
    monkeypatch.chdir(tmp)
    common = ["--reference_tester", "--dataloader", "datalist_json", "--datalist", os.path.join(tmp, "json.dat")]
    args = run.parse_args(base + common)
    assert run.test(args, model, run.build_config(args, json.loads(TT.CLASSDICT))) == 0
    plain = capsys.readouterr().out
    assert "Mean AveragePrecision" not in plain and not os.path.exists("Object-Detection-Metrics")
    model.calls = 0
    args = run.parse_args(base + common + ["--compute_map", "--map_outdir", "maps"])
    assert run.test(args, model, run.build_config(args, json.loads(TT.CLASSDICT))) == 0
    out = capsys.readouterr().out
    assert out.startswith(plain) and out[len(plain):].startswith("== Mean AveragePrecision (mAP) ==\nmAP=")
    assert "VOC IoU>=0.50 mAP=" in out and model.calls == 4
    assert sorted(os.listdir("maps")) == ["Object-Detection-Metrics", "metric-computation", "tarlen5-calculate-mean-ap"]
    assert sorted(os.listdir(".")) == sorted(set(os.listdir(".")) - {"Object-Detection-Metrics"})
    names = json.load(open("maps/metric-computation/predicted_boxes.json"))
    assert sorted(names) == ["img0.fits", "img1.fits"]
