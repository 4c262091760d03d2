"""The tester on the host: Analyzer.extract_gt_masks / compute_performances / get_data and ModelTester against the record taken
from the reference (tests/golden/tester.npz, made by tests/golden/make_tester_fixtures.py), value for value and byte for byte;
the device path of the two pixel steps with NumPy stand-ins for its kernels against the host statement; the closed forms of
the two restated third-party pieces (minimum-area rectangle, island count); and ``run.py test`` with and without
``--reference_tester``."""
import contextlib
import importlib.util
import io
import json
import math
import os

import numpy as np
import pytest
import torch

import caesar_mrcnn_amd  # noqa: F401
from caesar_mrcnn_amd import analyze, fits, ops
from caesar_mrcnn_amd.utils import extract_bboxes

import tester_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    return np.load(cases.GOLDEN)


def _analyzer(sc, device=False):
    an = analyze.Analyzer(None, cases.cfg(), cases.StubDataset(sc["consider"]), [], [])
    an.eval_device, an.eval_device_min_pairs = device, 0            # every scene, however few pairs it has
    return an


def _drive(sc, device=False):
    with contextlib.redirect_stdout(io.StringIO()):
        return cases.drive(_analyzer(sc, device), sc, extract_bboxes)


# ---- the host statement against the reference's record -----------------------------------------------------------
@pytest.mark.parametrize("sc", cases.scenarios(), ids=lambda s: s["name"])
def test_host_statement_equals_reference(golden, sc):
    an = _drive(sc)
    cases.assert_record(cases.analyzer_record(an, sc["shape"]), golden, sc["name"])


def test_rules_the_record_holds(golden):
    """What the scenarios were built to show is in the record itself."""
    rec = {s["name"]: cases.unflatten(golden, s["name"]) for s in cases.scenarios()}
    assert rec["twin_dets"]["detobj_classids"].tolist() == [3] and rec["twin_dets"]["detobj_scores"].tolist() == [float(np.float32(0.8))]
    assert rec["twin_gts"]["matchobj_classids"].tolist() == [3] and rec["twin_gts"]["nobjs_det_right"].sum() == 0
    assert rec["thr_exact"]["detobj_ious"].tolist() == [0.6, -999.0] and rec["thr_exact"]["is_gt_obj_detected"].tolist() == [1, 0]
    assert rec["class_mismatch"]["confusion_matrix"][2, 1] == 1 and rec["class_mismatch"]["nobjs_det_right"].sum() == 0
    assert rec["unmatched"]["detobj_class_names"].tolist() == ["compact", "not-detected"]
    assert rec["unmatched"]["matchobj_class_names"].tolist() == ["compact", "not-matched"]
    assert rec["empty_det"]["is_det_obj_matching_to_gt_obj"].tolist() == [0, 1, 0]
    assert rec["thr_zero"]["matchobj_ious"].tolist() == [1.0, 0.0] and rec["thr_zero"]["matchobj_classids"].tolist() == [2, 2]
    assert rec["sidelobe_off"]["is_gt_obj_detected"].size == 2 and rec["sidelobe_off"]["is_det_obj_matching_to_gt_obj"].tolist() == [1, 1, 1]
    split = rec["split_gt"]
    assert split["class_ids_gt_merged"].tolist() == [2, 1, 2, 3, 6] and split["sidelobes_mixed_or_near_gt_merged"].tolist() == [0, 1, 0, 0, 1]
    m = split["masks_gt_merged"]
    assert m[0].sum() == 12 and m[0][:, 30:].sum() == 0                      # the repeated-component rule: component 1 only
    assert m[1].sum() == 40 + 88 and m[3].sum() == 2 * 30 - 30 + 12 and m[4].sum() == 16 + 60       # merged; left whole


@pytest.mark.parametrize("run", sorted(cases.TESTER_RUNS))
def test_model_tester_equals_reference(golden, run, tmp_path):
    tester = analyze.ModelTester(None, cases.cfg(), cases.StubDataset())
    rec = cases.run_tester(tester, _analyzer, cases.TESTER_RUNS[run], extract_bboxes, str(tmp_path))
    assert rec["completeness_csv"].tobytes().startswith(b"# img,telescope,img_rms,img_bkg,sname,class_id,class_name,class_id_det,"
                                                        b"class_name_det,detected,score,iou,snr,maxBeamSize,aspectRatio,border\r\n")
    assert rec["reliability_csv"].tobytes().startswith(b"# img,telescope,img_rms,img_bkg,sname,class_id_det,class_name_det,class_id,"
                                                       b"class_name,matching_gt,score,iou,snr,maxBeamSize,aspectRatio,border\r\n")
    cases.assert_record(rec, golden, "tester_" + run)


def test_model_tester_defaults():
    t = analyze.ModelTester(None, cases.cfg(), cases.StubDataset())
    assert (t.n_max_img, t.remap_classids, t.classid_map, t.score_thr, t.iou_thr) == (-1, False, {}, 0.7, 0.6)
    assert t.n_classes == len(cases.CLASS_NAMES) and t.classification_matrix.shape == (t.n_classes, t.n_classes)
    assert (t.outfilename_completeness, t.outfilename_reliability) == ("completeness.csv", "reliability.csv")
    assert t.compute_mAP_metrics is False and t.purity.shape == (1, t.n_classes)
    an = analyze.Analyzer(None, cases.cfg())
    assert an.split_gtmasks is False and an.remap_classids is False and an.classid_map == {} and an.det_obj_pars == []
    assert an.confusion_matrix.shape == (7, 7) and an.gt_data is None and an.pred_data is None
    assert an.eval_device is (analyze.Analyzer.EVAL_DEVICE_MIN_PAIRS is not None and analyze.Analyzer.has_gpu(None))


def test_update_performances_leaves_out_rows_the_reference_would_raise_on(tmp_path, caplog):
    """Object info for all three true objects but per-object lists for one: the reference's counter runs off the lists."""
    sc = cases.scenario("table_off")
    an = _drive(sc)
    an.detobj_gtinfo = cases.gt_objs(sc)                                     # three entries against two results
    tester = analyze.ModelTester(None, cases.cfg(), cases.StubDataset())
    tester.outfilename_completeness, tester.outfilename_reliability = str(tmp_path / "c.csv"), str(tmp_path / "r.csv")
    with caplog.at_level("ERROR", logger="mrcnn"):
        assert tester.update_performances(an) == 0
    assert tester.completeness_dict_list == [] and len(tester.reliability_dict_list) == 1
    assert any("completeness rows are left out" in r.getMessage() for r in caplog.records)
    assert not os.path.exists(tester.outfilename_completeness) and os.path.exists(tester.outfilename_reliability)


@pytest.mark.parametrize("case", sorted(cases.REMAP_CASES))
def test_get_data_equals_reference(golden, case):
    ds, model = cases.get_data_scene()
    an = analyze.Analyzer(model, cases.cfg(), ds, [], [])
    rec = cases.run_get_data(an, case)
    assert int(rec["status"]) == (-1 if case == "remap_missing" else 0)
    cases.assert_record(rec, golden, "get_data_" + case)


# ---- the device path on NumPy stand-ins for the kernels -------------------------------------------------------------
def _fake_pack(masks):
    m = masks.numpy() != 0
    words = analyze.pack_mask_planes(m).view(np.int32)
    n = m.shape[-1]
    return ops.MaskPlanes(torch.from_numpy(words.copy()), torch.from_numpy(m.reshape(-1, n).sum(0).astype(np.int32)),
                          torch.from_numpy(extract_bboxes(m).astype(np.int32)), m.shape[1])


def _fake_cross(a, b):
    ua = analyze.unpack_mask_planes(a.words.numpy(), a.W).astype(np.int64).reshape(a.n, -1)
    ub = analyze.unpack_mask_planes(b.words.numpy(), b.W).astype(np.int64).reshape(b.n, -1)
    return torch.from_numpy((ua @ ub.T).astype(np.int32))


def _fake_sums(img, planes, big_endian=False):
    u = analyze.unpack_mask_planes(planes.words.numpy(), planes.W).astype(bool)
    x = img.numpy()
    return torch.from_numpy(np.array([np.nansum(x[u[p]], dtype=np.float64) for p in range(planes.n)], np.float64))


@pytest.fixture
def standins(monkeypatch):
    calls = {"pack": 0, "cross": 0, "sums": 0}

    def counted(name, fn):
        def wrapped(*a, **k):
            calls[name] += 1
            return fn(*a, **k)
        return wrapped
    monkeypatch.setattr(ops, "mask_planes_pack", counted("pack", _fake_pack))
    monkeypatch.setattr(ops, "mask_cross_stats", counted("cross", _fake_cross))
    monkeypatch.setattr(ops, "mask_plane_sums", counted("sums", _fake_sums))
    monkeypatch.setattr(analyze.Analyzer, "_device", lambda self: torch.device("cpu"))
    return calls


def _image(shape, path):
    rng = np.random.default_rng(shape[0] * shape[1])
    img = (rng.normal(size=shape) * 1e-3).astype(np.float32)
    img[4:7, 6:9] += 0.05
    fits.write_fits(path, img)
    return img


def _det_pars(sc, device, path):
    an = _drive(sc, device)
    an.image_path = path
    assert an.compute_det_mask_pars() == 0
    return an


@pytest.mark.parametrize("sc", cases.scenarios(), ids=lambda s: s["name"])
def test_device_path_equals_host(standins, sc, tmp_path):
    path = str(tmp_path / "img.fits")
    _image(sc["shape"], path)
    host, dev = _det_pars(sc, False, path), _det_pars(sc, True, path)
    G, D = len(host.masks_gt_merged), len(host.masks_final)
    if G * D > 0:
        assert standins == {"pack": 2, "cross": 1, "sums": 1} and dev.eval_timing["mask_uploads"] == 2      # one launch each
    else:
        assert standins == {"pack": 0, "cross": 0, "sums": 0}                                                   # nothing to pair: host
    a, b = cases.analyzer_record(dev, sc["shape"]), cases.analyzer_record(host, sc["shape"])
    assert sorted(a) == sorted(b)
    for k in a:
        assert a[k].shape == b[k].shape and bool(np.all(a[k] == b[k])), k
    assert dev.det_obj_pars == host.det_obj_pars and len(host.det_obj_pars) == D


def test_device_failure_falls_back_to_host_and_says_so(monkeypatch, standins, caplog):
    from caesar_mrcnn_amd import _hip

    def broken(a, b):
        raise _hip.HipPathError("no kernel")
    monkeypatch.setattr(ops, "mask_cross_stats", broken)
    monkeypatch.setattr(analyze, "device_forms_failed", set())
    sc = cases.scenario("unmatched")
    with caplog.at_level("ERROR", logger="mrcnn"):
        dev = _drive(sc, True)
    host = _drive(sc, False)
    assert dev.detobj_ious == host.detobj_ious and dev.matchobj_ious == host.matchobj_ious
    assert sum("compute_performances_device failed (HipPathError: no kernel)" in r.getMessage() for r in caplog.records) == 1


@pytest.mark.parametrize("form", ["compute_performances_device", "compute_det_mask_pars_device"])
def test_failed_device_form_is_left_for_the_process(form, monkeypatch, standins, caplog, tmp_path):
    import analyze_post_cases as post
    sc = cases.scenario("unmatched")
    path = str(tmp_path / "img.fits")
    _image(sc["shape"], path)

    def same(a, b):
        ra, rb = cases.analyzer_record(a, sc["shape"]), cases.analyzer_record(b, sc["shape"])
        return sorted(ra) == sorted(rb) and all(ra[k].shape == rb[k].shape and bool(np.all(ra[k] == rb[k])) for k in ra) and \
            a.det_obj_pars == b.det_obj_pars and len(a.det_obj_pars) > 0
    post.check_failure_policy(monkeypatch, caplog, form,
                              lambda entered: monkeypatch.setattr(analyze.Analyzer, form, post.planted_failure(entered)),
                              lambda: _det_pars(sc, True, path), _det_pars(sc, False, path), same)


def test_det_mask_pars_values(tmp_path):
    """The arithmetic of compute_det_mask_pars on one block: count, flux sum, signal-to-noise, boxes, border, sizes in beams."""
    sc = cases._sc("pars", cases.S65, [], [([(4, 7, 6, 9)], 2, 0.9), ([(0, 1, 10, 14)], 1, 0.8), ([], 1, 0.8)])
    path = str(tmp_path / "img.fits")
    img = _image(cases.S65, path)
    an = _det_pars(sc, False, path)
    p, q, r = an.det_obj_pars
    md = cases.META
    stot = float(img[4:7, 6:9].astype(np.float64).sum())
    assert p["npix"] == 9 and p["Stot"] == stot and p["name"] == "Sdet1" and p["class"] == "compact" and p["nislands"] == 1
    assert p["snr"] == float((stot - md["bkg"] * 9) / (md["rms"] * np.sqrt(9)))
    beam = int(math.ceil(np.sqrt(12.0 * 9.0) / 4.0))
    assert (p["bbox_w"], p["bbox_h"], p["bbox_x"], p["bbox_y"]) == (2.0, 2.0, 7.0, 5.0) and p["border"] == 0
    assert p["minsize_beam"] == 2.0 / beam and p["maxsize_beam"] == 2.0 / beam
    assert p["minsize_img_fract"] == min(3 / 65, 3 / 40) and p["maxsize_img_fract"] == max(3 / 65, 3 / 40)
    assert p["nbeams"] == 9 / (np.pi * 12.0 * 9.0 / (4 * np.log(2)) / 16.0)
    assert q["border"] == 1 and q["minsize_beam"] == 0.0 and q["maxsize_beam"] == 3.0 / beam and r == {}
    an.image_metadata = {}                                                   # list input: the -999 branch
    assert an.compute_det_mask_pars() == 0
    p = an.det_obj_pars[0]
    assert (p["snr"], p["nbeams"], p["minsize_beam"], p["maxsize_img_fract"]) == (-999.0, -999, -999, -999) and p["npix"] == 9


# ---- the restated third-party pieces, on closed forms -------------------------------------------------------------------
def _sizes(mask):
    (_, _), (w, h), angle = analyze.min_area_rect(mask)
    assert 0.0 < angle <= 90.0
    return min(w, h), max(w, h)


def test_min_area_rect_closed_forms():
    m = np.zeros((33, 40), np.uint8)
    assert analyze.min_area_rect(m) is None
    m[7, 9] = 1
    assert analyze.min_area_rect(m)[:2] == ((9.0, 7.0), (0.0, 0.0))
    for k in (2, 5, 17):
        m[:] = 0
        m[3, 4:4 + k] = 1
        assert _sizes(m) == (0.0, k - 1.0)
        assert _sizes(m.T.copy()) == (0.0, k - 1.0)
    for a, b in ((2, 2), (3, 7), (6, 4)):
        m[:] = 0
        m[5:5 + a, 8:8 + b] = 1
        assert _sizes(m) == (min(a, b) - 1.0, max(a, b) - 1.0)
        m[6:4 + a, 9:7 + b] = 0                                              # a hole never reaches the hull
        assert _sizes(m) == (min(a, b) - 1.0, max(a, b) - 1.0)
        assert analyze.min_area_rect(m)[0] == (8 + 0.5 * (b - 1), 5 + 0.5 * (a - 1))
    for r in (1, 3, 6):
        yy, xx = np.mgrid[:33, :40]
        d = (np.abs(yy - 10) + np.abs(xx - 12) <= r).astype(np.uint8)
        lo, hi = _sizes(d)
        assert abs(lo - r * math.sqrt(2)) < 1e-12 and abs(hi - r * math.sqrt(2)) < 1e-12
        (cx, cy), _, angle = analyze.min_area_rect(d)
        assert abs(cx - 12) < 1e-12 and abs(cy - 10) < 1e-12 and angle == 45.0
    # a diagonal run of pixels: collinear, length (k - 1) * sqrt(2), no width
    m[:] = 0
    for k in range(5):
        m[2 + k, 3 + k] = 1
    lo, hi = _sizes(m)
    assert lo == 0.0 and abs(hi - 4 * math.sqrt(2)) < 1e-12


def test_count_islands_is_8_connected(monkeypatch):
    m = np.zeros((9, 12), np.uint8)
    assert analyze.count_islands(m) == 0
    m[1, 1] = m[2, 2] = m[3, 1] = 1                                          # diagonal contact joins
    m[6, 6:9] = 1                                                            # apart
    m[8, 11] = 1
    assert analyze.count_islands(m) == 3 and analyze.label_components(m)[1] == 5
    import builtins
    real = builtins.__import__

    def no_scipy(name, *a, **k):
        if name.startswith("scipy"):
            raise ImportError(name)
        return real(name, *a, **k)
    monkeypatch.setattr(builtins, "__import__", no_scipy)
    assert analyze.count_islands(m) == 3


# ---- run.py test -----------------------------------------------------------------------------------------------------
def _run_py():
    spec = importlib.util.spec_from_file_location("_run_py_tester", os.path.join(ROOT, "scripts", "run.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


CLASSDICT = '{"spurious":1,"compact":2,"extended":3}'


class _SceneModel(object):
    """detect() answers with the planted results in turn, one per image of the two-image datasets below."""

    def __init__(self):
        self.results, self.calls = [], 0

    def detect(self, images, verbose=0):
        self.calls += 1
        return [self.results[(self.calls - 1) % len(self.results)]]


def _write_scene(tmp, k, model):
    """Image k (33 x 33) with two true objects and three detections: one exact, one of another class, one spurious."""
    shape = cases.S33
    img = np.full(shape, 1e-4, np.float32)
    img[4:10, 5:12] = 0.5
    ipath = os.path.join(tmp, "img%d.fits" % k)
    fits.write_fits(ipath, img)
    gt = [cases.rects(shape, (4, 10, 5, 12)), cases.rects(shape, (20, 25, 20 + k, 30))]
    objs = []
    for j, (g, cls) in enumerate(zip(gt, ("compact", "extended"))):
        mpath = os.path.join(tmp, "mask%d_%d.fits" % (k, j))
        fits.write_fits(mpath, g.astype(np.float32))
        objs.append({"mask": os.path.basename(mpath), "class": cls, "name": "S%d" % (j + 1), "sidelobe-mixed": 0, "sidelobe-near": 0,
                     "nislands": 1, "border": 0, "snr": 20.0 + j, "maxsize_beam": 3.0, "minsize_beam": 1.5})
    meta = dict(cases.META, nx=33, ny=33)
    jpath = os.path.join(tmp, "img%d.json" % k)
    with open(jpath, "w") as fp:
        json.dump(dict(meta, img=os.path.basename(ipath), objs=objs), fp)
    det = np.stack([gt[0], gt[1], cases.rects(shape, (28, 31, 2, 6))], axis=-1)
    result = {"masks": det, "rois": extract_bboxes(det).astype(np.int32), "class_ids": np.array([2, 1, 1], np.int32),
              "scores": np.array([0.95, 0.85, 0.6 + 0.2 * k], np.float32)}
    model.results.append(result)
    return ipath, [os.path.join(tmp, "mask%d_%d.fits" % (k, j)) for j in range(2)], jpath, gt, result


def _legacy_summary(scenes, cfg):
    """What run.py test has printed so far, restated on the planted scenes: strict `>` on the IoU, one-sided matching."""
    C = cfg.NUM_CLASSES
    n_true, n_true_det, n_det, n_det_ok = np.zeros(C), np.zeros(C), np.zeros(C), np.zeros(C)
    for gt_masks, gt_ids, r in scenes:
        keep = r["scores"] >= cfg.SCORE_THR
        det_masks, det_ids = r["masks"][:, :, keep], r["class_ids"][keep]
        matched = set()
        for g in range(len(gt_masks)):
            n_true[gt_ids[g]] += 1
            best, bj = 0.0, -1
            for j in range(det_masks.shape[-1]):
                iou = analyze.mask_iou(gt_masks[g], det_masks[:, :, j])
                if iou > best:
                    best, bj = iou, j
            if best >= cfg.IOU_THR:
                n_true_det[gt_ids[g]] += 1
                matched.add(bj)
        for j in range(det_masks.shape[-1]):
            n_det[det_ids[j]] += 1
            n_det_ok[det_ids[j]] += j in matched
    lines = []
    for c in range(1, C):
        comp = n_true_det[c] / n_true[c] if n_true[c] else float("nan")
        rel = n_det_ok[c] / n_det[c] if n_det[c] else float("nan")
        lines.append("class %s: completeness %.3f (%d/%d) reliability %.3f (%d/%d)" % (cfg.CLASS_NAMES[c], comp, n_true_det[c], n_true[c],
                                                                                    rel, n_det_ok[c], n_det[c]))
    return "\n".join(lines) + "\n"


@pytest.fixture
def scenes(tmp_path):
    model = _SceneModel()
    tmp = str(tmp_path)
    made = [_write_scene(tmp, k, model) for k in range(2)]
    with open(os.path.join(tmp, "list.dat"), "w") as fp:
        for ipath, mpaths, _, _, _ in made:
            fp.write("%s,%s,compact\n" % (ipath, mpaths[0]))
    with open(os.path.join(tmp, "json.dat"), "w") as fp:
        for _, _, jpath, _, _ in made:
            fp.write(jpath + "\n")
    return tmp, model, made


def _args(run, tmp, *extra):
    args = run.parse_args(["test", "--imgsize", "64", "--classdict", CLASSDICT] + list(extra))
    return args, run.build_config(args, json.loads(CLASSDICT))


def test_run_py_test_prints_what_it_printed(scenes, capsys, monkeypatch):
    tmp, model, made = scenes
    monkeypatch.chdir(tmp)
    run = _run_py()
    args, cfg = _args(run, tmp, "--datalist", os.path.join(tmp, "list.dat"))
    assert args.reference_tester is False and args.remap_classids is False and args.consider_sources_near_mixed_sidelobes is True
    capsys.readouterr()
    assert run.test(args, model, cfg) == 0
    out = capsys.readouterr().out
    assert out == _legacy_summary([([m[3][0]], [2], m[4]) for m in made], cfg)
    args, cfg = _args(run, tmp, "--dataloader", "datalist_json", "--datalist", os.path.join(tmp, "json.dat"))
    assert run.test(args, model, cfg) == 0
    assert capsys.readouterr().out == _legacy_summary([(m[3], [2, 3], m[4]) for m in made], cfg)
    assert not os.path.exists("completeness.csv") and not os.path.exists("reliability.csv")


def test_run_py_reference_tester_writes_the_two_tables(scenes, capsys, monkeypatch):
    tmp, model, made = scenes
    monkeypatch.chdir(tmp)
    run = _run_py()
    args, cfg = _args(run, tmp, "--reference_tester", "--dataloader", "datalist_json", "--datalist", os.path.join(tmp, "json.dat"),
                      "--no_consider_sources_near_mixed_sidelobes")
    assert args.consider_sources_near_mixed_sidelobes is False
    assert run.test(args, model, cfg) == 0
    out = capsys.readouterr().out
    assert "== CLASSIFICATION MATRIX ==" in out and "== PRECISION (or PURITY) ==" in out and "completeness 1.000" not in out
    import csv
    with open("completeness.csv") as fp:
        assert fp.read(2) == "# "
        comp = list(csv.DictReader(fp))
    with open("reliability.csv") as fp:
        assert fp.read(2) == "# "
        rel = list(csv.DictReader(fp))
    assert list(comp[0]) == ["img", "telescope", "img_rms", "img_bkg", "sname", "class_id", "class_name", "class_id_det", "class_name_det",
                             "detected", "score", "iou", "snr", "maxBeamSize", "aspectRatio", "border"]
    assert list(rel[0]) == ["img", "telescope", "img_rms", "img_bkg", "sname", "class_id_det", "class_name_det", "class_id", "class_name",
                            "matching_gt", "score", "iou", "snr", "maxBeamSize", "aspectRatio", "border"]
    # two true objects per image; detections at or above 0.7: two in the first image, three in the second
    assert [r["sname"] for r in comp] == ["S1", "S2"] * 2 and [r["detected"] for r in comp] == ["1", "1"] * 2
    assert [r["class_name_det"] for r in comp] == ["compact", "spurious"] * 2 and [r["iou"] for r in comp] == ["1.0"] * 4
    assert [r["sname"] for r in rel] == ["Sdet1", "Sdet2", "Sdet1", "Sdet2", "Sdet3"]
    assert [r["matching_gt"] for r in rel] == ["1", "1", "1", "1", "0"] and rel[4]["class_name"] == "not-matched" and rel[4]["iou"] == "-999.0"
    assert [os.path.basename(r["img"]) for r in rel] == ["img0.fits"] * 2 + ["img1.fits"] * 3 and rel[0]["telescope"] == "askap"
    # --maxnimgs stops after one image; --remap_classids without a dictionary is refused
    os.remove("completeness.csv"); os.remove("reliability.csv")
    args, cfg = _args(run, tmp, "--reference_tester", "--dataloader", "datalist_json", "--datalist", os.path.join(tmp, "json.dat"),
                      "--remap_classids", "--classid_remap_dict", "{1: 3, 2: 2}")
    assert run.test(args, model, cfg) == 0
    with open("completeness.csv") as fp:
        fp.read(2)
        assert [r["class_name_det"] for r in csv.DictReader(fp)] == ["compact", "extended"] * 2
    args, cfg = _args(run, tmp, "--reference_tester", "--dataloader", "datalist_json", "--datalist", os.path.join(tmp, "json.dat"),
                      "--remap_classids")
    assert run.test(args, model, cfg) == -1


def test_run_py_reference_tester_refuses_list_input(scenes, monkeypatch, caplog):
    tmp, model, made = scenes
    monkeypatch.chdir(tmp)
    run = _run_py()
    args, cfg = _args(run, tmp, "--reference_tester", "--datalist", os.path.join(tmp, "list.dat"))
    with caplog.at_level("ERROR", logger="mrcnn"):
        assert run.test(args, model, cfg) == -1
    assert any("datalist_json or datadir_json" in r.getMessage() for r in caplog.records)
    assert not os.path.exists("completeness.csv")
