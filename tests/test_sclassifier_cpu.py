"""The source classifier on the host (caesar-mrcnn_amd/classifier.py) against what the reference's SClassifier.classify_source did
on the scenarios of sclassifier_cases.py (golden/sclassifier.npz, made by golden/make_sclassifier_fixtures.py), and against the
stated behaviour where the reference raises.  Every comparison is exact.  No GPU."""
import json
import os
import warnings

import numpy as np
import pytest

import sclassifier_cases as cases

G = np.load(cases.GOLDEN)
SCENARIOS = {sc["name"]: sc for sc in cases.scenarios()}
DEPARTURES = {sc["name"]: sc for sc in cases.departures()}


def make(sc, monkeypatch, log=None):
    """An SClassifier on scenario `sc` with the stand-in Analyzer; returns (classifier, the Analyzer's call log)."""
    from caesar_mrcnn_amd import classifier
    log = [] if log is None else log
    monkeypatch.setattr(classifier, "Analyzer", cases.analyzer_class(sc["planted"], log))
    return cases.setup(classifier.SClassifier(None, cases.Cfg()), sc, classifier.SData), log


def run(sc, monkeypatch):
    clf, log = make(sc, monkeypatch)
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        statuses, visited = cases.drive(clf)
    return clf, log, statuses, visited


@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_port_equals_reference_fixture(name, monkeypatch):
    """Return codes, visited flags after every call, the cut-outs made (names, in order), the
    local boxes handed to the Analyzer (so: windows, member lists and their order), class_id / class_name / snames of every
    class_info, and the mosaic the run leaves (the in-place NaN fill).  score: the planted one (the reference leaves 0)."""
    sc = SCENARIOS[name]
    clf, log, statuses, visited = run(sc, monkeypatch)
    rec = cases.record(clf, log, statuses, visited)
    keys = sorted(k.split("/", 1)[1] for k in G.files if k.startswith(name + "/"))
    assert keys == sorted(rec), (keys, sorted(rec))
    for k in keys:
        want, got = G[name + "/" + k], rec[k]
        assert want.dtype == got.dtype and want.shape == got.shape, (k, want.dtype, got.dtype, want.shape, got.shape)
        if want.dtype.kind == "f":
            assert np.array_equal(want.view("u%d" % want.dtype.itemsize), got.view("u%d" % got.dtype.itemsize)), k
        else:
            assert np.array_equal(want, got), (k, want, got)
    # the Analyzer got the classifier's thresholds, and writes nothing per cut-out
    assert all(e["thr"] == (clf.iou_thr, clf.score_thr) and e["writes"] == (False, False, False) for e in log)
    # scores: every class_info carries the score planted with the detection of its class in the cut-out it came from
    planted_scores = {(cid, float(s)) for p in sc["planted"].values() if p != "fail" for s, cid in zip(p[1], p[2])}
    infos = [c for s in clf.sources for c in s.class_info]
    assert infos and all((int(c.class_id), float(c.score)) in planted_scores for c in infos)


def test_fixture_holds_the_cases_it_claims():
    """The scenarios are what their comments say (so a changed scenario cannot quietly stop testing its case)."""
    v = lambda name: G[name + "/visited"]
    names = lambda name: [s[0] for s in SCENARIOS[name]["sources"]]
    ci = lambda name: list(zip(G[name + "/ci_source"].tolist(), G[name + "/ci_class_id"].tolist(), G[name + "/ci_snames"].tolist()))
    # edges: after A's cut-out the centres on the four edges are not members; the boxes touching an edge are members but cut
    first = dict(zip(names("edges"), v("edges")[0]))
    assert first["A"] and first["inL"] and first["nL"] and first["nR"]
    assert not any(first[n] for n in ("onL", "onR", "onT", "onB", "tL", "tR", "tT", "tB"))
    assert G["edges/call0_boxes"].shape[0] == 1 + 7                       # A, inL, tL, tR, tT, tB, nL, nR minus none on an edge
    # trunc: windows 40 (not 41) and 0 (not -1)
    assert G["trunc/call0_boxes"][0, 1] == 49.2 - 40 and G["trunc/call0_boxes"].shape[0] == 2
    e = list(G["trunc/call_names"]).index("E")
    assert G["trunc/call%d_boxes" % e][0, 1] == (10.2 - 2) - 0 and G["trunc/call%d_boxes" % e].shape[0] == 3
    # ties: the later of two equal IoUs wins (class 2, not 1); IoU == iou_thr is no match (B has no class_info)
    assert ci("ties") == [(0, 2, "")]
    # visit: B visited through A and skipped; C classified from A's and from D's cut-out; A and B share a detection
    assert list(G["visit/call_names"]) == ["A", "C", "D", "far"] and v("visit")[0].tolist() == [True, True, False, False, False]
    assert ci("visit") == [(0, 2, "B"), (1, 2, "A"), (2, 3, ""), (2, 3, ""), (3, 1, "")]
    assert G["nmax/statuses"].size == 2 and list(G["nmax/call_names"]) == ["A"]
    # predfail: A's cut-out marks nobody, B then gets its own
    assert G["predfail/statuses"][0] == -1 and not v("predfail")[0].any() and list(G["predfail/call_names"])[:2] == ["A", "B"]
    # nanfill: B's window holds A's fill value, below B's own minimum, and B's later fill used it
    img0, img1 = cases.nan_image(), G["nanfill/img_data"]
    assert np.nanmin(img0[8:32, 18:42]) > 0 and (img1[15:26, 28:35] == -40).all() and (img1[18:22, 40:42] == -40).all()
    assert (img1[18:22, 42:46] == -40).all() and not np.isnan(img1).any() and list(G["nanfill/call_names"]) == ["A", "B", "C", "lone"]


@pytest.mark.parametrize("name", sorted(SCENARIOS) + sorted(DEPARTURES))
def test_numpy_member_scan_equals_the_double_loop(name, monkeypatch):
    """windows, member lists and cut flags of every source: SClassifier.window / members_host / _cutout against the double loop."""
    sc = dict(SCENARIOS, **DEPARTURES)[name]
    clf, _ = make(sc, monkeypatch)
    for i in range(len(clf.sources)):
        window, js, cut = cases.literal_members(sc["sources"], i, sc["size"])
        c = clf._cutout(i)
        assert c.window == window and c.members == [i] + js and c.cut[1:] == cut
        assert c.boxes == [[s[5] - window[2], s[3] - window[0], s[6] - window[2], s[4] - window[0]] for s in (sc["sources"][k] for k in c.members)]
    w, off, mem, cut = cases.members_numpy(clf._table(), sc["size"], sc["size"])
    for i in range(len(clf.sources)):
        window, js, cf = cases.literal_members(sc["sources"], i, sc["size"])
        assert tuple(w[i]) == window and mem[off[i]:off[i + 1]].tolist() == js and cut[off[i]:off[i + 1]].astype(bool).tolist() == cf


def test_departures(monkeypatch, caplog):
    """Where the reference raises: an oversized source is warned about and cut; a degenerate box has IoU 0; a lone source with a
    detection is matched; a window with a negative corner, past the image or without a finite pixel fails alone (-1, not visited,
    nothing written), and its neighbours are classified."""
    from caesar_mrcnn_amd import utils
    clf, log, statuses, visited = run(DEPARTURES["oversized"], monkeypatch)
    assert statuses == [0, 0] and visited[0] == [False, True] and visited[1] == [False, True]
    assert [e["name"] for e in log] == ["big"] and cases.class_infos(clf) == [(0, 3, "galaxy_C2", "")]
    assert any("Cutout size" in r.getMessage() and "big" in r.getMessage() for r in caplog.records)

    assert utils.get_iou([10, 8, 10, 12], [10, 8, 10, 12]) == 0.0 and utils.get_iou([0, 0, 4, 4], [2, 5, 3, 5]) == 0.0
    assert utils.get_iou([0, 0, 4, 4], [0, 0, 4, 8]) == 0.5 and utils.get_iou([0, 0, 4, 4], [4, 4, 8, 8]) == 0.0
    assert utils.get_iou([0, 0, 4, 4], [5, 5, 8, 8]) == 0.0
    clf, log, statuses, visited = run(DEPARTURES["degenerate"], monkeypatch)
    assert statuses == [0, 0] and cases.class_infos(clf) == [(1, 2, "source", "")] and clf.sources[1].class_info[0].score == 0.8

    clf, log, statuses, visited = run(DEPARTURES["lone"], monkeypatch)
    assert statuses == [0] and cases.class_infos(clf) == [(0, 2, "source", "")] and clf.sources[0].class_info[0].score == 0.9

    sc = DEPARTURES["windows"]
    clf, log, statuses, visited = run(sc, monkeypatch)
    assert statuses == [-1, -1, -1, 0, 0]
    assert visited[2] == [False] * 5 and visited[4] == [False, False, False, True, True]
    assert [e["name"] for e in log] == ["ok"] and cases.class_infos(clf) == [(3, 2, "source", "")]
    assert np.array_equal(clf.img_data.view(np.uint32), sc["image"]().view(np.uint32))           # nothing written into a failed window


def test_crop_img_equals_read_fits_chain(tmp_path):
    """crop_img(stretch, normalize, RGB) = read_fits of the same cut, byte for byte: the identity the batched form rests on
    (ops.fits_tiles_to_rgb is pinned to read_fits).  Windows with NaNs, clipped at the far edges, tiny and of 1023 / 1025 pixels."""
    from caesar_mrcnn_amd import fits
    img = cases.nan_image()
    path = str(tmp_path / "m.fits")
    fits.write_fits(path, img)
    for (x0, y0, dx, dy) in ((20, 20, 24, 24), (30, 20, 24, 24), (70, 50, 24, 24), (40.7, 30.2, 33, 31), (41, 30, 41, 25), (12, 12, 6, 6)):
        xmin, xmax, ymin, ymax = int(x0 - dx / 2), int(x0 + dx / 2), int(y0 - dy / 2), int(y0 + dy / 2)
        data = img.copy()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            a = fits.crop_img(data, x0, y0, dx, dy, True, True, True)
            b = fits.read_fits(path, xmin, min(xmax, 80), ymin, min(ymax, 60))[0]
        assert a.dtype == np.uint8 and a.shape == b.shape and np.array_equal(a, b), (x0, y0, dx, dy)


@pytest.mark.parametrize("name", sorted(SCENARIOS) + sorted(DEPARTURES))
def test_plan_equals_the_loop(name, monkeypatch):
    """plan(failed) = the cut-outs the loop ran, in order, with the members and boxes the Analyzer was given; failed = the
    cut-outs that returned -1.  Without the failures the plan differs wherever one of them would have marked somebody."""
    sc = dict(SCENARIOS, **DEPARTURES)[name]
    clf, log, statuses, visited = run(sc, monkeypatch)
    ran = [i for i, st in enumerate(statuses) if st < 0 or (i == 0 or not visited[i - 1][i])]
    failed = frozenset(i for i, st in enumerate(statuses) if st < 0)
    fresh, _ = make(sc, monkeypatch)
    plan = fresh.plan(failed)
    assert [c.index for c in plan] == ran and [c.failed for c in plan] == [c.index in failed for c in plan]
    made = {e["name"]: e["boxes"] for e in log}
    for c in plan:
        nm = sc["sources"][c.index][0]
        if nm in made:
            assert np.array_equal(np.array(c.boxes, np.float64).reshape(-1, 4), made[nm])
    flags = [False] * len(sc["sources"])
    for c in plan:
        if not c.failed:
            fresh._mark(c, flags)
    assert flags == visited[-1]
    if name == "predfail":
        assert [c.index for c in fresh.plan()] == [0, 2, 3, 4] != ran


def test_read_table_and_scatalog(tmp_path, caplog):
    from caesar_mrcnn_amd import classifier, fits
    path = str(tmp_path / "cat.dat")
    rows = [["S1", 1, 0, 3, 7.5, 50.25, 60.5, 0, 0, 0, 0, 0, 0, 48, 53, 58, 63, "x"],
            ["S2", 2, 1, 4, 8.5, 10, 20, 0, 0, 0, 0, 0, 0, 8, 12, 18, 22, "7"],
            ["S1", 3, 0, 1, 1e-3, 1.5e2, -3, 0, 0, 0, 0, 0, 0, 1, 2, 3, 4, "y"]]
    with open(path, "w") as f:
        f.write("# name npix ...\n\n   \n#another comment\n")
        for r in rows:
            f.write("  ".join(str(v) for v in r) + "\n")
        f.write("\n")
    t = fits.read_table(path)
    assert len(t) == 3 and [len(r) for r in t] == [18] * 3
    assert [r[0] for r in t] == ["S1", "S2", "S1"] and [r[17] for r in t] == ["x", "7", "y"]          # a mixed column stays str
    assert all(isinstance(v, float) for r in t for v in r[1:17]) and t[2][4] == 1e-3 and t[2][5] == 150.0 and t[2][6] == -3.0
    assert fits.read_table(str(tmp_path / "missing.dat")) is None
    with open(str(tmp_path / "ragged.dat"), "w") as f:
        f.write("a 1 2\nb 1\n")
    assert fits.read_table(str(tmp_path / "ragged.dat")) is None
    clf = classifier.SClassifier(None, cases.Cfg())
    clf.scatalog_path = path
    assert clf.read_scatalog() == 0
    assert [(s.name, s.x0, s.y0, s.xmin, s.xmax, s.ymin, s.ymax) for s in clf.sources] == [
        ("S1", 50.25, 60.5, 48.0, 53.0, 58.0, 63.0), ("S2", 10.0, 20.0, 8.0, 12.0, 18.0, 22.0), ("S1", 150.0, -3.0, 1.0, 2.0, 3.0, 4.0)]
    assert sum("names repeat" in r.getMessage() for r in caplog.records) == 1
    clf.scatalog_path = str(tmp_path / "ragged.dat")
    assert clf.read_scatalog() == -1
    with open(str(tmp_path / "short.dat"), "w") as f:
        f.write("a 1 2\nb 1 3\n")
    clf.scatalog_path = str(tmp_path / "short.dat")
    assert clf.read_scatalog() == -1


def test_catalogue_files(tmp_path, monkeypatch):
    """run() end to end on files (FITS mosaic, ascii catalogue) with the stand-in Analyzer: sclass_<image>.json / .dat under
    outdir, byte for byte; best = highest score, the earliest of equals; nothing else is written."""
    from caesar_mrcnn_amd import classifier, fits
    sc = SCENARIOS["visit"]
    monkeypatch.setattr(classifier, "Analyzer", cases.analyzer_class(sc["planted"], []))
    fits.write_fits(str(tmp_path / "mosaic.fits"), sc["image"]())
    with open(str(tmp_path / "cat.dat"), "w") as f:
        for (n, x0, y0, a, b, c, d) in sc["sources"]:
            f.write(" ".join([n] + ["0"] * 4 + [repr(float(x0)), repr(float(y0))] + ["0"] * 6 + [str(v) for v in (a, b, c, d)]) + "\n")
    clf = classifier.SClassifier(None, cases.Cfg())
    clf.scutout_size, clf.iou_thr, clf.outdir = sc["size"], sc["iou_thr"], str(tmp_path / "out")
    monkeypatch.chdir(tmp_path)
    assert clf.run(str(tmp_path / "mosaic.fits"), str(tmp_path / "cat.dat")) == 0
    assert sorted(os.listdir(str(tmp_path))) == ["cat.dat", "mosaic.fits", "out"]
    assert sorted(os.listdir(clf.outdir)) == ["sclass_mosaic.dat", "sclass_mosaic.json"]
    want = [("A", 2, "source", 0.9, 1, "B"), ("B", 2, "source", 0.9, 1, "A"), ("C", 3, "galaxy_C2", 0.85, 2, ""), ("D", 1, "sidelobe", 0.99, 1, ""),
            ("far", -1, "", 0.0, 0, "")]
    doc = json.load(open(clf.outfile_json))
    assert doc["image"] == "mosaic.fits" and doc["scatalog"] == "cat.dat"
    assert [(r["name"], r["class_id"], r["class_name"], r["score"], r["nentries"], r["snames"]) for r in doc["sources"]] == want
    assert open(clf.outfile_dat).read() == "# name class_id class_name score nentries snames\n" + "".join(
        "%s %d %s %.6f %d %s\n" % (n, c, cn or "-", s, k, sn or "-") for n, c, cn, s, k, sn in want)
    # ties in the score go to the earliest entry
    s = clf.sources[4]
    for cid, score in ((1, 0.5), (2, 0.75), (3, 0.75)):
        c = classifier.SClassInfo()
        c.class_id, c.class_name, c.score, c.snames = cid, cases.CLASS_NAMES[cid], score, ["A"] if cid == 1 else ["D", "A"]
        s.add_class_info(c)
    assert clf.catalogue_rows()[4] == {"name": "far", "class_id": 2, "class_name": "source", "score": 0.75, "nentries": 3, "snames": "A,D"}


def test_switches_are_off_by_default():
    from caesar_mrcnn_amd import classifier
    clf = classifier.SClassifier(None, cases.Cfg())
    assert clf.cutout_batch == 0 and clf.plan_device is False and clf.save_cutout_results is False and clf.scutout_size == 132
    assert (clf.iou_thr, clf.score_thr, clf.n_max_sources, clf.outdir) == (0.6, 0.7, -1, ".")
    assert not clf._batched() and clf.member_lists() is None
    c = classifier.SClassInfo()
    assert (c.class_id, c.class_name, c.score, c.snames) == (-1, '', 0, [])
    an = clf._analyzer()
    assert (an.write_to_json, an.write_to_ds9, an.draw) == (False, False, False) and (an.iou_thr, an.score_thr) == (0.6, 0.7)
    clf.save_cutout_results = True
    an = clf._analyzer()
    assert an.write_to_json and an.write_to_ds9


def test_command_line_and_config():
    """scripts/sclassifier.py: the reference's options and defaults plus the four new ones; the reference's SClassifierConfig
    values, IMAGES_PER_GPU following --cutout_batch, no OPTIMIZER."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("sclassifier_script", os.path.join(cases.ROOT, "scripts", "sclassifier.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    a = mod.parse_args(["--image", "m.fits", "--scatalog", "c.dat", "--weights", "w.h5"])
    assert (a.scoreThr, a.iouThr, a.nsources_max, a.scutout_size) == (0.7, 0.6, -1, 132)
    assert (a.cutout_batch, a.plan_device, a.outdir, a.save_cutout_results) == (0, False, ".", False)
    a = mod.parse_args(["--image", "m", "--scatalog", "c", "--weights", "w", "--cutout_batch", "8", "--plan_device", "--outdir", "o",
                        "--save_cutout_results", "--scutout_size", "64", "--nsources_max", "5"])
    assert (a.cutout_batch, a.plan_device, a.outdir, a.save_cutout_results, a.scutout_size, a.nsources_max) == (8, True, "o", True, 64, 5)
    cfg = mod.make_config()
    assert (cfg.NAME, cfg.IMAGES_PER_GPU, cfg.BATCH_SIZE, cfg.NUM_CLASSES) == ("sources", 1, 1, 5)
    assert cfg.CLASS_NAMES == cases.CLASS_NAMES and cfg.DETECTION_MIN_CONFIDENCE == 0 and cfg.RPN_ANCHOR_SCALES == (4, 8, 16, 32, 64)
    assert (cfg.BACKBONE, cfg.IMAGE_MIN_DIM, cfg.IMAGE_MAX_DIM, cfg.RPN_NMS_THRESHOLD, cfg.MAX_GT_INSTANCES) == ("resnet101", 256, 256, 0.9, 300)
    assert list(cfg.MEAN_PIXEL) == [0, 0, 0] and cfg.USE_MINI_MASK is False and not hasattr(cfg, "OPTIMIZER")
    assert mod.make_config(4).BATCH_SIZE == 4 and tuple(cfg.IMAGE_SHAPE) == (256, 256, 3)
