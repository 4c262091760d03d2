"""csrc/apmatch.hip (ops.voc_match) against its host statement, exactly; metrics.voc_metrics_device against voc_metrics_host; the
mask overlaps from bit planes against utils.compute_overlaps_masks; ModelTester.compute_mAP on a real model, device against host."""
import contextlib
import io
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import map_cases as cases                                   # noqa: E402
import tester_cases as tcases                               # noqa: E402
from caesar_mrcnn_amd import _hip, analyze, metrics, ops, utils   # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = np.load(cases.GOLDEN)
T10 = tuple(0.5 + 0.05 * k for k in range(10))              # 0.5 ... 0.95
LDS_CAP = 256                                               # APM_GT_CAP of csrc/apmatch.hip


def _device_match(flat, thr, dev):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    got = ops.voc_match(t(flat.det_box), t(flat.det_cls), t(flat.det_score), flat.det_off, t(flat.gt_box), t(flat.gt_cls), flat.gt_off,
                        t(np.asarray(thr, np.float64)))
    return [g.cpu().numpy() for g in got]


def _assert_match(gt, pred, thr, dev, what):
    flat = metrics.Flat(gt, pred)
    want = metrics.voc_match_host(flat, thr)
    got = _device_match(flat, thr, dev)
    for name, a, b in zip(("best_gt", "best_iou", "tp"), got, want):
        assert a.dtype == b.dtype and a.shape == b.shape, (what, name, a.dtype, b.dtype, a.shape, b.shape)
        bad = np.argwhere(a != b)
        assert bad.size == 0, "%s: %s differs at %s: got %r, want %r" % (what, name, bad[:5].tolist(), a[tuple(bad[0])], b[tuple(bad[0])])
    assert metrics.same_metrics(metrics.voc_metrics_device(gt, pred, thr, device=dev), metrics.voc_metrics_host(gt, pred, thr)), what
    return flat, want


@pytest.mark.parametrize("case", cases.golden_cases(GOLDEN))
def test_voc_match_fixture_cases(dev, case):
    """The hand-built cases and the tool's sample files, at the fixture's thresholds and at 0.5 ... 0.95; the device metrics equal
    the tool's recorded answer as well."""
    gt, pred, classes, thr, want = cases.load(GOLDEN, case)
    _assert_match(gt, pred, thr, dev, case)
    _assert_match(gt, pred, T10, dev, case + " T=10")
    cases.assert_record(cases.record(metrics.voc_metrics_device(gt, pred, thr, device=dev)), want, case)


def _crowd(n_det, n_gt, seed, coarse=8, places=3):
    """One image: n_gt ground truths and n_det detections of two classes on a coarse grid (`places` positions and three sizes per
    axis, so that boxes coincide and overlap often), scores from ten values."""
    rng = np.random.default_rng(seed)

    def box():
        y, x = (int(v) * coarse for v in rng.integers(0, places, 2))
        h, w = (int(v) * coarse for v in rng.integers(1, 4, 2))
        return [y, x, y + h - 1, x + w - 1]
    labels = ["galaxy", "source"]
    gt = [box() + [labels[k % 2]] for k in range(n_gt)]
    pred = [box() + [labels[int(rng.integers(0, 2))], float(rng.integers(1, 11)) / 10.0] for _ in range(n_det)]
    return [gt], [pred]


@pytest.mark.parametrize("n_det", [64, 65, 130])
def test_voc_match_more_than_one_pass(dev, n_det):
    """65 and 130 detections on 3 ground truths: a lane takes two and three detections.  The first and the last detection are the
    first ground truth's own box, the last one with the highest score: it takes the ground truth, and the first one -- another
    pass of the wavefront when there is more than one -- loses it at every threshold."""
    gt, pred = _crowd(n_det, 3, 100 + n_det)
    pred[0][0] = gt[0][0][:5] + [0.55]
    pred[0][-1] = gt[0][0][:5] + [1.0]
    flat, (best_gt, best_iou, tp) = _assert_match(gt, pred, T10, dev, "crowd %d" % n_det)
    assert best_gt[0] == best_gt[-1] == 0 and best_iou[0] == best_iou[-1] == 1.0
    assert tp[:, -1].all() and not tp[:, 0].any() and (best_gt >= 0).sum() > 10


@pytest.mark.parametrize("n_gt", [LDS_CAP, LDS_CAP + 1, 300])
def test_voc_match_ground_truths_past_the_lds_cap(dev, n_gt):
    """One image whose ground truths fill the LDS table exactly, and ones that no longer fit: read from global memory.  A second,
    small image follows, so that the rows after the large image are checked too."""
    gt, pred = _crowd(40, n_gt, 7 + n_gt, coarse=4, places=6)
    gt2, pred2 = _crowd(5, 4, 8)
    flat, (best_gt, _, tp) = _assert_match(gt + gt2, pred + pred2, (0.5, 0.75), dev, "cap %d" % n_gt)
    assert best_gt.max() >= n_gt and (best_gt[:40] >= 0).sum() >= 20


def _random_set(n_images, seed):
    rng = np.random.default_rng(seed)
    labels = ["compact", "extended", "galaxy"]
    gt_data, pred_data = [], []

    def box():
        y, x = (int(v) for v in rng.integers(0, 3, 2) * 16)
        h, w = (int(v) for v in rng.integers(1, 3, 2) * 16)
        return [y, x, y + h - 1, x + w - 1]
    for _ in range(n_images):
        gt_data.append([box() + [labels[int(rng.integers(0, 3))]] for _ in range(int(rng.integers(0, 13)))])
        pred_data.append([box() + [labels[int(rng.integers(0, 3))], float(rng.integers(1, 21)) / 20.0] for _ in range(int(rng.integers(0, 13)))])
    return gt_data, pred_data


def test_voc_match_random_images(dev):
    """300 seeded images with 0 - 12 boxes of 3 classes on a 64 x 64 frame, corners on multiples of 16 (a 32 x 16 box inside a 32 x 32 one has IoU 0.5 exactly): equal IoUs, equal scores and
    ground truths chosen by several detections are frequent, empty images occur."""
    gt, pred = _random_set(300, 20260101)
    flat, (best_gt, best_iou, tp) = _assert_match(gt, pred, T10, dev, "random")
    ties = shared = lost = 0
    for i in range(flat.I):
        d0, d1, g0, g1 = flat.det_off[i], flat.det_off[i + 1], flat.gt_off[i], flat.gt_off[i + 1]
        if d1 == d0 or g1 == g0:
            continue
        iou = metrics.box_iou_matrix(flat.det_box[d0:d1], flat.gt_box[g0:g1])
        iou = np.where(flat.det_cls[d0:d1, None] == flat.gt_cls[None, g0:g1], iou, 0.0)
        top = iou.max(axis=1)
        ties += int(((iou == top[:, None]) & (top[:, None] > 0)).sum(axis=1).max() > 1)
        chosen = best_gt[d0:d1][best_gt[d0:d1] >= 0]
        shared += int(chosen.size > np.unique(chosen).size)
        lost += int(((best_iou[d0:d1] >= 0.5) & (tp[0, d0:d1] == 0)).any())
    print("random set: %d detections, %d ground truths; images with a tie for the best IoU %d, with a shared best ground truth %d, "
          "with a detection that lost its ground truth at 0.5 %d" % (flat.D, flat.G, ties, shared, lost))
    assert ties >= 10 and shared >= 10 and lost >= 10
    assert any(len(g) == 0 for g in gt) and any(len(p) == 0 for p in pred)
    assert np.unique(flat.det_score).size < flat.D // 10


def test_voc_match_empty_and_refused(dev, monkeypatch):
    L = _hip.lib()
    t = torch.zeros(64, dtype=torch.float64, device=dev)
    p, s = t.data_ptr(), _hip.current_stream()
    for D, G, I, T in ((0, 1, 1, 1), (1, -1, 1, 1), (1, 1, 0, 1), (1, 1, 1, 0)):
        assert L.mrcnn_voc_match(p, p, p, p, D, p, p, p, G, I, p, T, p, p, p, s) == -1
    assert L.mrcnn_voc_match(p, p, p, p, 1, None, None, p, 1, 1, p, 1, p, p, p, s) == -1
    monkeypatch.setattr(_hip, "lib", lambda: pytest.fail("a launch for an empty request"))
    for gt, pred in (([], []), ([[], []], [[], []]), ([[cases.B10 + ["galaxy"]]], [[]])):
        flat = metrics.Flat(gt, pred)
        best_gt, best_iou, tp = _device_match(flat, (0.5, 0.6), dev)
        assert best_gt.shape == (0,) and best_iou.shape == (0,) and tp.shape == (2, 0)
        assert metrics.same_metrics(metrics.voc_metrics_device(gt, pred, (0.5, 0.6), device=dev), metrics.voc_metrics_host(gt, pred, (0.5, 0.6)))
    monkeypatch.undo()
    flat = metrics.Flat([[]], [[cases.B10 + ["galaxy", 0.5]]])                    # detections, no ground truth anywhere: one launch
    best_gt, best_iou, tp = _device_match(flat, (0.5,), dev)
    assert best_gt.tolist() == [-1] and best_iou.tolist() == [0.0] and tp.tolist() == [[0]]
    flat.det_off = np.array([0, 2])
    with pytest.raises(_hip.HipPathError):
        _device_match(flat, (0.5,), dev)


def test_voc_metrics_selects_by_size(dev, monkeypatch):
    gt, pred = _random_set(40, 5)
    calls = []
    real = ops.voc_match
    monkeypatch.setattr(ops, "voc_match", lambda *a, **k: calls.append(1) or real(*a, **k))
    n = sum(map(len, pred))
    monkeypatch.setattr(metrics, "DEVICE_MIN_DETECTIONS", n + 1)
    a = metrics.voc_metrics(gt, pred, (0.5,))
    assert calls == []
    monkeypatch.setattr(metrics, "DEVICE_MIN_DETECTIONS", n)
    b = metrics.voc_metrics(gt, pred, (0.5,))
    assert calls == [1] and metrics.same_metrics(a, b)


# ---- mask overlaps ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 5, 9])
def test_mask_overlaps_device_equals_host(dev, n):
    """33 x 65 frames (a row is two words and one bit), n detection planes against 9 - n + 1 true ones, an empty plane on either
    side -- and, for n = 5, on both, where 0 / 0 gives the same NaN."""
    H, W = 33, 65
    rng = np.random.default_rng(50 + n)
    a = rng.random((H, W, n)) < 0.3
    b = rng.random((H, W, 10 - n)) < 0.4
    a[:4, :, 0] = True
    b[:4, :, 0] = True
    if n > 1:
        a[:, :, 1] = False
    if b.shape[-1] > 1:
        b[:, :, -1] = False
    with np.errstate(divide="ignore", invalid="ignore"):
        want = utils.compute_overlaps_masks(a, b)
    got = metrics.mask_overlaps_device(torch.from_numpy(a.view(np.uint8)).to(dev), b)
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape == (n, 10 - n)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert torch.equal(torch.from_numpy(np.nan_to_num(got, nan=-1.0)), torch.from_numpy(np.nan_to_num(want, nan=-1.0)))
    assert bool(np.isnan(want).any()) == (n in (2, 5))
    none = metrics.mask_overlaps_device(None, b)
    assert none.shape == (0, 10 - n) and none.dtype == utils.compute_overlaps_masks(a[:, :, :0], b).dtype


@pytest.mark.parametrize("sc", cases.ap_scenes(), ids=lambda s: s["name"])
def test_mask_ap_device_equals_host(dev, sc, monkeypatch):
    gt_box, gt_cls, gt_mask, box, cls, score, mask = cases.ap_inputs(sc, utils.extract_bboxes)
    r = {"rois": box, "class_ids": cls, "scores": score, "masks": mask}
    with np.errstate(divide="ignore", invalid="ignore"):
        want = utils.compute_ap(gt_box, gt_cls, gt_mask, box, cls, score, mask, 0.6)
        masks_dev = torch.from_numpy(np.ascontiguousarray(mask).view(np.uint8)).to(dev) if mask.shape[-1] else None
        if masks_dev is not None:                                             # (without detections nothing lies on the device)
            monkeypatch.setattr(utils, "compute_overlaps_masks", lambda *a: pytest.fail("the full-frame product was formed"))
        got = metrics.mask_ap(gt_box, gt_cls, gt_mask, r, masks_dev, 0.6)
    for a, b in zip(got, want):
        assert np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


# ---- ModelTester.test() with compute_mAP_metrics on a real model -----------------------------------------------------------
class _TwoImages(object):
    """Two images for ModelTester, as SourceDataset presents JSON entries (and load_mask / source_class_ids for load_image_gt)."""

    def __init__(self, images, paths, gt_masks, class_ids, class_names, metadata):
        self.nclasses = self.num_classes = len(class_names)
        self.class_names = list(class_names)
        self.consider_sources_near_mixed_sidelobes = True
        self.image_ids = list(range(len(images)))
        self.source_class_ids = {"": [0], "rg-dataset": list(range(self.nclasses))}
        self.image_info = []
        for k in self.image_ids:
            objs = [{"name": "S%d" % (j + 1), "class": class_names[c], "sidelobe-mixed": 0, "nislands": 1, "border": 0, "snr": 10.0 + j,
                     "maxsize_beam": 2.0 + j, "minsize_beam": 1.0} for j, c in enumerate(class_ids[k])]
            self.image_info.append({"id": "scene%d" % k, "source": "rg-dataset", "path": paths[k], "class_ids": list(class_ids[k]),
                                    "sidelobes_mixed_or_near": [0] * len(class_ids[k]), "objs": objs, "metadata": metadata})
        self._images, self._gt = images, gt_masks

    def load_image(self, image_id):
        return self._images[image_id]

    def load_mask(self, image_id):
        return self._gt[image_id], np.array(self.image_info[image_id]["class_ids"], np.int32)

    def image_uuid(self, image_id):
        return self.image_info[image_id]["id"]

    def image_metadata(self, image_id):
        return self.image_info[image_id]["metadata"]

    def load_gt_masks(self, image_id, binary=True):
        return self._gt[image_id] if binary else self._gt[image_id].astype(int)

    def load_gt_obj_info(self, image_id):
        return self.image_info[image_id]["objs"]


def test_model_tester_compute_map_real_model(dev, tmp_path, monkeypatch):
    """A MaskRCNN with seeded random weights (custom backbone, 128 x 128, score_thr = 0) through ModelTester.test() with
    compute_mAP_metrics: the mask overlaps from the device tensor the model kept and the box matching on the GPU give the APs and
    the VOC result of the host forms."""
    import model_cases as T
    import analyze_post_cases as post
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
        # true objects: the first detections themselves (one under another class), and a block nothing was detected on
        gts.append(np.concatenate([first["masks"][:, :, :n], post.rect((128, 128), 100, 110, 5, 25)[:, :, None]], axis=-1).astype(bool))
        c = [int(v) for v in first["class_ids"][:n]] + [1]
        c[0] = 1 + c[0] % (cfg.NUM_CLASSES - 1)
        ids.append(c)
    monkeypatch.chdir(tmp_path)
    counts = {"voc": 0, "cross": 0}
    real_voc, real_overlaps = ops.voc_match, metrics.mask_overlaps_device
    monkeypatch.setattr(ops, "voc_match", lambda *a, **k: counts.__setitem__("voc", counts["voc"] + 1) or real_voc(*a, **k))
    monkeypatch.setattr(metrics, "mask_overlaps_device", lambda *a, **k: counts.__setitem__("cross", counts["cross"] + 1) or real_overlaps(*a, **k))

    def run(device):
        monkeypatch.setattr(metrics, "DEVICE_MIN_DETECTIONS", 0 if device else 1 << 40)
        monkeypatch.setattr(metrics, "EXACT_PIXELS", (1 << 24) if device else 0)
        ds = _TwoImages(images, paths, gts, ids, cfg.CLASS_NAMES, dict(tcases.META, nx=128, ny=128))
        tester = analyze.ModelTester(model, cfg, ds)
        tester.score_thr, tester.compute_mAP_metrics = 0.0, True
        tester.metrics_outdir = "files_%d" % device
        tester.outfilename_completeness, tester.outfilename_reliability = "c_%d.csv" % device, "r_%d.csv" % device
        out = io.StringIO()
        with contextlib.redirect_stdout(out):
            assert tester.test() == 0
        return tester, out.getvalue()
    t_dev, out_dev = run(True)
    assert counts == {"voc": 1, "cross": 2}
    t_host, out_host = run(False)
    assert counts == {"voc": 1, "cross": 2}
    assert len(t_dev.APs) == 2 and t_dev.APs == t_host.APs and t_dev.mAP == t_host.mAP
    assert metrics.same_metrics(t_dev.voc, t_host.voc) and t_dev.voc["thresholds"] == [0.5, 0.6]
    assert sum(len(c["TP"]) for c in t_dev.voc["results"][0]["classes"].values()) >= 2
    assert max(t_dev.APs) > 0                                                 # the true objects ARE detections: something matches
    assert out_dev == out_host and "== Mean AveragePrecision (mAP) ==\nmAP=%f\n" % t_dev.mAP in out_dev
    assert cases.tree_bytes("files_1") == cases.tree_bytes("files_0") and len(cases.tree_bytes("files_1")) == 8
