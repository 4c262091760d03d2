"""The source classifier's device forms on the GPU (csrc/catalog.hip): ops.catalog_members against the NumPy member scan,
ops.catalog_window_flags / catalog_nan_fill + ops.fits_tiles_to_rgb against sequential fits.crop_img on a host copy, and
SClassifier.cutout_batch / plan_device against the loop over classify_source.  Every comparison is exact."""
import warnings

import numpy as np
import pytest

import sclassifier_cases as cases

pytestmark = pytest.mark.gpu


# ---- member lists -----------------------------------------------------------------------------------------------------------
def _member_tables():
    """(tag, table [S, 6], cut-out size).  S = 1, 2, 63, 64, 65 (a wavefront and the 64 sources of a workgroup), 256, 257 (the LDS
    tile of 256 centres)."""
    out = []
    for S in (1, 2, 63, 64, 65, 256, 257):
        out.append(("scattered S=%d" % S, cases.random_catalogue(S, 150, S), 40))
        one = cases.random_catalogue(S, 8, 100 + S)                   # all centres within 8 pixels: every window holds all of them
        one[:, :2] += 100
        one[:, 2:4] += 100
        one[:, 4:6] += 100
        out.append(("one window S=%d" % S, one, 40))
        grid = np.arange(S, dtype=np.float64)
        far = np.stack([50 * (grid % 17), 50 * (grid // 17), 50 * (grid % 17) - 2, 50 * (grid % 17) + 2, 50 * (grid // 17) - 2,
                        50 * (grid // 17) + 2], axis=1)
        out.append(("no members S=%d" % S, far, 40))
        out.append(("identical S=%d" % S, np.tile(np.array([[30.5, 41.25, 28, 33, 39, 44]]), (S, 1)), 12))
    out.append(("negative corners", cases.random_catalogue(130, 30, 9), 40))
    out.append(("integer centres", cases.random_catalogue(200, 60, 10, frac=False), 10))       # centres and boxes exactly on window edges
    for sc in cases.scenarios() + cases.departures():
        out.append((sc["name"], np.array([s[1:] for s in sc["sources"]], dtype=np.float64), sc["size"]))
    return out


def test_catalog_members_equal_numpy_statement(dev):
    from caesar_mrcnn_amd import ops
    seen = {"all": 0, "none": 0, "neg": 0, "cut": 0}
    for tag, table, size in _member_tables():
        want = cases.members_numpy(table, size, size)
        got = ops.catalog_members(table, size, size, dev)
        again = ops.catalog_members(table, size, size, dev)
        for name, w, g, a in zip(("windows", "offsets", "members", "cut"), want, got, again):
            assert w.dtype == g.dtype and w.shape == g.shape and np.array_equal(w, g), (tag, name)
            assert np.array_equal(g, a), (tag, name, "second call differs")
        S = table.shape[0]
        seen["all"] += S > 1 and int(want[1][-1]) == S * (S - 1)
        seen["none"] += S > 1 and int(want[1][-1]) == 0
        seen["neg"] += bool((want[0] < 0).any())
        seen["cut"] += bool(want[3].any()) and not bool(want[3].all())
    assert all(v > 0 for v in seen.values()), seen
    # a non-square cut-out
    t = cases.random_catalogue(100, 80, 3)
    for w, g in zip(cases.members_numpy(t, 33, 17), ops.catalog_members(t, 33, 17, dev)):
        assert np.array_equal(w, g)


def test_catalog_members_refusals(dev):
    """A catalogue above the cap (lowered to 64 for the test), coordinates outside the 32-bit range, NaN: CatalogUnsupported before
    anything is launched -- the C entries return MRCNN_ERR_UNSUPPORTED and leave their outputs alone -- and SClassifier takes the
    host scan for that catalogue without giving up on the device form."""
    import torch
    from caesar_mrcnn_amd import _hip, analyze, classifier, ops
    table = cases.random_catalogue(65, 150, 1)
    ops.tuning_set("catalog_max_sources", 64)
    try:
        with pytest.raises(ops.CatalogUnsupported):
            ops.catalog_members(table, 40, 40, dev)
        assert ops.catalog_members(table[:64], 40, 40, dev)[1][-1] == cases.members_numpy(table[:64], 40, 40)[1][-1]
        L = _hip.lib()
        cols = torch.from_numpy(np.ascontiguousarray(table.T)).to(dev)
        win = torch.full((65, 4), -7, dtype=torch.int32, device=dev)
        cnt = torch.full((65,), -7, dtype=torch.int32, device=dev)
        assert L.mrcnn_catalog_check(65) == -4 and L.mrcnn_catalog_check(64) == 0 and L.mrcnn_catalog_check(0) == -1
        assert L.mrcnn_catalog_count(_hip.ptr(cols[0]), _hip.ptr(cols[1]), 65, 40.0, 40.0, _hip.ptr(win), _hip.ptr(cnt), _hip.current_stream()) == -4
        off = torch.zeros(66, dtype=torch.int64, device=dev)
        mem = torch.full((8,), -7, dtype=torch.int32, device=dev)
        cut = torch.full((8,), 7, dtype=torch.uint8, device=dev)
        args = [_hip.ptr(cols[k]) for k in range(6)]
        assert L.mrcnn_catalog_fill(*args, 65, 40.0, 40.0, _hip.ptr(off), 8, _hip.ptr(mem), _hip.ptr(cut), _hip.current_stream()) == -4
        assert L.mrcnn_catalog_fill(*args, 64, 40.0, 40.0, _hip.ptr(off), 2 ** 31, _hip.ptr(mem), _hip.ptr(cut), _hip.current_stream()) == -4
        assert L.mrcnn_catalog_count(_hip.ptr(cols[0]), _hip.ptr(cols[1]), 64, 0.0, 40.0, _hip.ptr(win), _hip.ptr(cnt), _hip.current_stream()) == -1
        torch.cuda.synchronize()
        assert bool((win == -7).all()) and bool((cnt == -7).all()) and bool((mem == -7).all()) and bool((cut == 7).all())
        # the classifier: the host scan answers this catalogue, the device form is not written off
        clf = classifier.SClassifier(None, cases.Cfg())
        for row in table:
            s = classifier.SData()
            s.name, (s.x0, s.y0, s.xmin, s.xmax, s.ymin, s.ymax) = "s", row.tolist()
            clf.sources.append(s)
        clf.plan_device, clf.scutout_size = True, 40
        assert clf.member_lists() is None and "SClassifier.member_lists" not in analyze.device_forms_failed
        want = cases.members_numpy(table, 40, 40)
        c = clf._cutout(7)
        assert c.window == tuple(want[0][7]) and c.members[1:] == want[2][want[1][7]:want[1][8]].tolist()
    finally:
        ops.tuning_set("catalog_max_sources", ops.CATALOG_MAX_SOURCES)
    clf._lists_key = None
    got = clf.member_lists()                                                        # with the cap back the device answers
    assert got is not None and all(np.array_equal(w, g) for w, g in zip(want, got))
    for bad in (np.array([[3e9, 0, 0, 1, 0, 1]]), np.array([[np.nan, 0, 0, 1, 0, 1]]), np.array([[0, -np.inf, 0, 1, 0, 1]])):
        with pytest.raises(ops.CatalogUnsupported):
            ops.catalog_members(bad, 40, 40, dev)
    with pytest.raises(ValueError):
        ops.catalog_members(np.zeros((0, 6)), 40, 40, dev)


# ---- window flags and the ordered fill ---------------------------------------------------------------------------------------
def _fill_scenes():
    """(tag, plane, [(xmin, xmax, ymin, ymax)] in plan order)."""
    out = []
    # the chain of the CPU case: A's minimum (-40) is below B's own; C shares a NaN block with B; D lies where NaNs have been
    # filled by its turn; E is clipped at the right and the bottom edge and holds NaNs; F is all-NaN (and apart), G past the plane,
    # H has a negative corner, I is NaN-free
    img = cases.nan_image()
    img[50:60, 70:80] = np.nan
    img[55, 66] = -3.0
    img[40:50, 0:10] = np.nan
    wins = [(8, 32, 8, 32), (18, 42, 8, 32), (32, 56, 10, 34), (28, 36, 14, 27), (63, 87, 43, 67), (0, 10, 40, 50), (80, 104, 10, 34),
            (-3, 21, 20, 44), (50, 60, 30, 40)]
    out.append(("chain 60x80", img, wins))
    # an all-NaN window that an earlier, overlapping window's fill brings to life, and one it does not reach
    rng = np.random.RandomState(2)
    img = rng.normal(5, 1, (40, 40)).astype(np.float32)
    img[10:20, 10:40] = np.nan
    out.append(("revived 40x40", img, [(6, 12, 8, 14), (10, 16, 11, 17), (20, 26, 12, 18), (13, 19, 12, 18)]))
    # statistics chunk edges: 1023, 1024, 1025 pixels, not square; infinities beside NaNs (nanmin takes them, zscale does not)
    img = rng.normal(0, 1, (200, 200)).astype(np.float32)
    img[::7, ::5] = np.nan
    img[100, 100] = -np.inf
    img[30, 150] = np.inf
    out.append(("chunks 200x200", img, [(10, 43, 20, 51), (30, 62, 40, 72), (60, 101, 90, 115), (90, 130, 85, 125), (140, 180, 10, 50),
                                        (170, 210, 170, 210)]))
    clean = rng.normal(0, 1, (64, 64)).astype(np.float32)
    out.append(("no NaN 64x64", clean, [(0, 20, 0, 20), (10, 30, 10, 30), (50, 70, 50, 70)]))
    return out


def _host_statement(img, wins):
    """Sequential fits.crop_img over the windows on a copy: (the RGB cut-out or None per window, the plane it leaves)."""
    from caesar_mrcnn_amd import fits
    data = img.copy()
    rgbs = []
    for (xmin, xmax, ymin, ymax) in wins:
        crop = data[ymin:ymax, xmin:xmax] if min(xmin, xmax, ymin, ymax) >= 0 else data[0:0]
        if crop.size == 0 or not np.isfinite(crop).any():
            rgbs.append(None)
            continue
        with warnings.catch_warnings(), np.errstate(all="ignore"):
            warnings.simplefilter("ignore")
            rgbs.append(fits.crop_img(data, (xmin + xmax) / 2, (ymin + ymax) / 2, xmax - xmin, ymax - ymin, True, True, True))
    return rgbs, data


@pytest.mark.parametrize("form", [0, 1])
def test_flags_and_fill_equal_sequential_crop_img(dev, form):
    import torch
    from caesar_mrcnn_amd import ops
    assert 33 * 31 == 1023 and 41 * 25 == 1025
    for tag, img, wins in _fill_scenes():
        ny, nx = img.shape
        want_rgb, want_plane = _host_statement(img, wins)
        plane = torch.from_numpy(img).to(dev)
        flags = ops.catalog_window_flags(plane, wins)
        for k, (xmin, xmax, ymin, ymax) in enumerate(wins):
            crop = img[ymin:ymax, xmin:xmax] if min(xmin, xmax, ymin, ymax) >= 0 else img[0:0]
            assert flags[k].tolist() == [int(np.isfinite(crop).sum()), int(np.isnan(crop).sum())], (tag, k)
        assert np.array_equal(plane.cpu().numpy().view(np.uint32), img.view(np.uint32))          # flags write nothing
        todo = [k for k in range(len(wins)) if flags[k, 1] > 0]
        alive = ops.catalog_nan_fill(plane, [wins[k] for k in todo], form)
        assert alive.tolist() == [want_rgb[k] is not None for k in todo], tag
        got_plane = plane.cpu().numpy()
        assert np.array_equal(got_plane.view(np.uint32), want_plane.view(np.uint32)), tag
        ok = [k for k in range(len(wins)) if want_rgb[k] is not None]
        rects = [(wins[k][0], wins[k][2], min(wins[k][1], nx) - wins[k][0], min(wins[k][3], ny) - wins[k][2]) for k in ok]
        for k, g in zip(ok, ops.fits_tiles_to_rgb(plane, rects)):
            g = g.cpu().numpy()
            assert g.shape == want_rgb[k].shape and np.array_equal(g, want_rgb[k]), (tag, k)
        if "no NaN" in tag:
            assert todo == [] and ops.catalog_nan_fill(plane, [], form).size == 0
        if "revived" in tag:
            assert flags[1].tolist() == [0, 36] and alive.tolist() == [True, True, False, True]
        if "chain" in tag:
            assert [want_rgb[k] is None for k in range(len(wins))] == [False] * 5 + [True] * 3 + [False] and 8 not in todo
            assert (got_plane[15:26, 28:35] == -40).all() and np.isnan(got_plane[40:50, 0:10]).all() and (got_plane[50:60, 70:80] == -3).all()


# ---- end to end ----------------------------------------------------------------------------------------------------------------
NY = NX = 200
SIZE = 40


def _mosaic():
    """Blobs on unit noise, a NaN border of 12 pixels and a NaN strip; the catalogue: one source per blob, three more without one,
    two of them so close to the border that their window has a negative corner or is clipped."""
    rng = np.random.RandomState(7)
    yy, xx = np.mgrid[0:NY, 0:NX]
    img = rng.normal(0.0, 1.0, (NY, NX)).astype(np.float32)
    centres = [(40, 40), (52, 47), (100, 45), (150, 40), (45, 100), (100, 100), (112, 108), (160, 100), (40, 160), (100, 165), (165, 165),
               (172, 150)]
    for cx, cy in centres:
        img += (np.float32(rng.uniform(60, 120)) * np.exp(-0.5 * (((yy - cy) / 3.0) ** 2 + ((xx - cx) / 3.0) ** 2))).astype(np.float32)
    img[:12] = img[-12:] = np.nan
    img[:, :12] = img[:, -12:] = np.nan
    img[90:94, 60:140] = np.nan
    sources = [("S%d" % (k + 1), cx + 0.3, cy - 0.2, cx - 5, cx + 5, cy - 5, cy + 5) for k, (cx, cy) in enumerate(centres)]
    sources += [("edge1", 15.0, 100.0, 10, 20, 95, 105), ("edge2", 185.5, 185.5, 180, 190, 180, 190), ("void", 75.0, 140.0, 70, 80, 135, 145)]
    return img, sources


def _revived():
    """Windows without a finite pixel in the mosaic as it is read: R2's gets some from R1's fill before its turn, R3's from R2's;
    nothing reaches D's."""
    img = np.random.RandomState(8).normal(0.0, 1.0, (120, 120)).astype(np.float32)
    img[30:90, 50:120] = np.nan
    img[95:120, 0:45] = np.nan
    return img, [cases.src("R1", 45, 60, 4), cases.src("R2", 72, 60, 4), cases.src("R3", 100, 60, 4), cases.src("R4", 100, 100, 4),
                 cases.src("D", 20, 115, 4)]


class BytesModel(object):
    """Stand-in for MaskRCNN: the detections of an image are the 4-connected components of image[..., 0] >= 200 that have at least 6
    pixels -- a pure function of the cut-out's bytes -- with a class taken from the component's size.  Host arrays or device
    tensors, any batch length; `raise_on` = the number of the batched (device tensor) call that raises."""

    def __init__(self, config, raise_on=None):
        self.config, self.batches, self.raise_on, self.device_calls = config, [], raise_on, 0

    def detect(self, images, verbose=0):
        from caesar_mrcnn_amd import analyze, utils
        self.batches.append(len(images))
        if hasattr(images[0], "cpu"):
            self.device_calls += 1
            if self.device_calls == self.raise_on:
                raise RuntimeError("planted failure of a batched detect")
        out = []
        for image in images:
            image = image.cpu().numpy() if hasattr(image, "cpu") else np.asarray(image)
            labels, n = analyze.label_components((image[..., 0] >= 200).astype(np.uint8))
            keep = [k for k in range(1, n + 1) if int((labels == k).sum()) >= 6]
            masks = np.stack([labels == k for k in keep], axis=-1) if keep else np.zeros(image.shape[:2] + (0,), bool)
            out.append({"rois": utils.extract_bboxes(masks), "class_ids": np.array([1 + int((labels == k).sum()) % 4 for k in keep], np.int32),
                        "scores": np.array([0.8 + 0.001 * (int((labels == k).sum()) % 100) for k in keep], np.float32), "masks": masks})
        return out


def _config():
    from caesar_mrcnn_amd.config import SDetectorConfig
    cfg = SDetectorConfig()
    cfg.CLASS_NAMES, cfg.NUM_CLASSES = list(cases.CLASS_NAMES), len(cases.CLASS_NAMES)
    return cfg


def _classifier(scene, batch, plan_device, outdir, raise_on=None):
    from caesar_mrcnn_amd import classifier
    from caesar_mrcnn_amd.analyze import Analyzer

    class FailingAnalyzer(Analyzer):                      # the Analyzer step of one cut-out returns -1: known only after planning
        def _accept(self, r, masks_device, bboxes_gt):
            if self.image_id == "S6":
                return -1
            return Analyzer._accept(self, r, masks_device, bboxes_gt)

    class Clf(classifier.SClassifier):
        def _analyzer(self):
            an = classifier.SClassifier._analyzer(self)
            if scene == "analyzer fails":
                an.__class__ = FailingAnalyzer
            return an
    cfg = _config()
    clf = Clf(BytesModel(cfg, raise_on), cfg)
    img, sources = _revived() if scene == "revived" else _mosaic()
    if scene == "no NaN":
        img = np.where(np.isnan(img), np.float32(0.0), img).astype(np.float32)
    cases.setup(clf, dict(sources=sources, image=lambda: img, size=SIZE, iou_thr=0.2, n_max=-1), classifier.SData)
    clf.cutout_batch, clf.plan_device, clf.outdir, clf.image_path = batch, plan_device, outdir, "mosaic.fits"
    return clf


def _outcome(clf):
    assert clf.save() == 0
    return ([bool(s.visited) for s in clf.sources],
            [(i, int(c.class_id), c.class_name, float(c.score), tuple(c.snames)) for i, s in enumerate(clf.sources) for c in s.class_info],
            open(clf.outfile_json).read(), open(clf.outfile_dat).read(), clf.img_data.view(np.uint32).copy())


@pytest.fixture(scope="module")
def sequential(dev, tmp_path_factory):
    out = {}
    for scene in ("plain", "analyzer fails", "no NaN", "revived"):
        clf = _classifier(scene, 0, False, str(tmp_path_factory.mktemp("seq")))
        with warnings.catch_warnings(), np.errstate(all="ignore"):
            warnings.simplefilter("ignore")
            assert clf.classify_all() == 0
        out[scene] = _outcome(clf) + (list(clf.model.batches),)
    return out


@pytest.mark.parametrize("plan_device", [False, True])
@pytest.mark.parametrize("batch", [1, 3, 4])
def test_batched_equals_the_loop(dev, sequential, tmp_path, batch, plan_device):
    """cutout_batch = 1, 3, 4 (a short last group at 3 and 4), plan_device off and on: visited flags, class infos (scores
    included), both catalogue files and the mosaic the run leaves equal the loop's.  Scenes: the mosaic with its NaN border and
    strip (windows with NaNs, a negative corner, a clipped window); a cut-out whose Analyzer step returns -1 after planning (the
    plan is made again); a group whose detect raises (its cut-outs go one at a time); a mosaic without NaN; windows without a
    finite pixel that an earlier cut-out's fill brings to life (the plan is corrected from what the fill found)."""
    import torch
    for scene, raise_on in (("plain", None), ("analyzer fails", None), ("plain", 2), ("no NaN", None), ("revived", None)):
        clf = _classifier(scene, batch, plan_device, str(tmp_path / ("%s_%s" % (scene.replace(" ", "_"), raise_on))), raise_on)
        assert clf._batched()
        with warnings.catch_warnings(), np.errstate(all="ignore"):
            warnings.simplefilter("ignore")
            assert clf.classify_all() == 0
        got = _outcome(clf)
        want = sequential[scene]
        tag = (scene, raise_on, batch, plan_device)
        assert got[0] == want[0], tag
        assert got[1] == want[1], tag
        assert got[2] == want[2] and got[3] == want[3], tag
        assert np.array_equal(got[4], want[4]), tag
        ncut = len(want[5])
        if scene == "plain" and raise_on is None:
            assert clf.model.batches == [batch] * (-(-ncut // batch)), tag                  # every cut-out detected once, in groups
        if raise_on is not None:
            assert 1 in clf.model.batches[1:] and clf.model.device_calls >= 2, tag           # the group that raised went one at a time
        if scene == "analyzer fails":
            assert clf.timing["batched_rounds"] >= 2, tag
        if scene == "revived":
            assert clf.timing["batched_rounds"] == 3, tag                                    # R2, then R3, found alive by the fill
        if plan_device:
            assert clf.member_lists() is not None
    # the scenes are what they claim
    visited, infos = sequential["plain"][0], sequential["plain"][1]
    assert len(infos) >= 8 and not visited[12] and visited[14], (visited, infos)
    assert sequential["revived"][0] == [True, True, True, True, False]
    assert sequential["analyzer fails"][0] != sequential["plain"][0] or sequential["analyzer fails"][1] != sequential["plain"][1]
    img, _ = _mosaic()
    assert not np.array_equal(sequential["plain"][4], img.view(np.uint32))                  # the loop filled NaNs in the mosaic
