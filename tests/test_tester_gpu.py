"""The two kernels of csrc/maskeval.hip against NumPy -- ``mask_cross_stats`` exactly, ``mask_plane_sums`` within the bound of an
n-term float64 sum -- and the Analyzer's device path of compute_performances / compute_det_mask_pars against its host statement,
on the scenarios of tests/tester_cases.py and on a real MaskRCNN.  Frames are at most 128 x 128."""
import numpy as np
import pytest
import torch

import caesar_mrcnn_amd  # noqa: F401
from caesar_mrcnn_amd import analyze, ops

import tester_cases as cases

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52


def _planes(masks_bool, dev):
    """[H, W, n] bool -> MaskPlanes on the device."""
    return ops.mask_planes_pack(torch.from_numpy(np.ascontiguousarray(masks_bool).view(np.uint8)).to(dev))


def _cross_reference(a, b):
    """Brute force: popcount(a_i & b_j) for [H, W, na] and [H, W, nb] bool."""
    na, nb = a.shape[-1], b.shape[-1]
    out = np.zeros((na, nb), np.int32)
    for i in range(na):
        for j in range(nb):
            out[i, j] = int(np.logical_and(a[:, :, i], b[:, :, j]).sum())
    return out


def _blobs(rng, H, W, n):
    m = np.zeros((H, W, n), bool)
    for d in range(n):
        for _ in range(int(rng.integers(1, 3))):
            y, x = int(rng.integers(0, H)), int(rng.integers(0, W))
            m[y:y + int(rng.integers(1, max(2, H))), x:x + int(rng.integers(1, max(2, W))), d] = True
        m[:, :, d] &= rng.uniform(size=(H, W)) < 0.8
    return m


@pytest.mark.parametrize("H", [1, 3, 33])
@pytest.mark.parametrize("W", [1, 31, 32, 33, 65])
def test_mask_cross_stats_shapes(dev, H, W):
    """Every (na, nb) on both sides of the four-cells-per-workgroup boundary; seeded blobs, so that empty and non-empty
    intersections both occur."""
    for na, nb in ((1, 1), (3, 5), (4, 4), (5, 3), (9, 1)):
        rng = np.random.default_rng(10000 * H + 100 * W + 10 * na + nb)
        a, b = _blobs(rng, H, W, na), _blobs(rng, H, W, nb)
        got = ops.mask_cross_stats(_planes(a, dev), _planes(b, dev))
        assert got.dtype == torch.int32 and tuple(got.shape) == (na, nb)
        np.testing.assert_array_equal(got.cpu().numpy(), _cross_reference(a, b), err_msg=str((H, W, na, nb)))


def _constructed(W):
    """Two plane sets on a 9 x W frame, W = 65: every a_i is paired with every b_j by the kernel; the diagonal holds the probes."""
    H = 9
    A, B = [], []

    def rect(*rects):
        m = np.zeros((H, W), bool)
        for y1, y2, x1, x2 in rects:
            m[y1:y2, x1:x2] = True
        return m

    def add(a, b):
        A.append(a); B.append(b)
    add(rect((2, 4, 50, W)), rect((3, 5, W - 1, W)))                               # overlap only in the last word of a row
    add(rect((4, 5, 20, 33)), rect((4, 5, 31, 40)) & ~rect((4, 5, 33, 40)))        # overlap = bit 31 of word 0 and bit 0 of word 1 ...
    add(rect((5, 6, 31, 32), (5, 6, 32, 33)), rect((5, 6, 31, 33)))                # ... and exactly those two bits, both set alone
    add(rect((0, 3, 5, 9)), rect((0, 1, 0, W)))                                    # overlap only in the first row
    add(rect((6, H, 40, 44)), rect((H - 1, H, 0, W)))                              # overlap only in the last row
    add(rect((0, H, 0, W)), rect((3, 6, 8, 30)))                                   # nested boxes
    add(rect((3, 6, 8, 30)), rect((3, 6, 8, 30)))                                  # identical boxes
    add(rect((0, 2, 0, 5)), rect((7, 9, 60, W)))                                   # disjoint boxes
    add(rect((1, 8, 1, 2), (1, 8, 31, 32), (1, 2, 1, 32), (7, 8, 1, 32)), rect((3, 6, 8, 30)))     # boxes nested, pixels apart
    add(rect(), rect((0, H, 0, W)))                                                # an empty plane on the a side
    add(rect((0, H, 0, W)), rect())                                                # ... and on the b side
    return np.stack(A, axis=-1), np.stack(B, axis=-1)


def test_mask_cross_stats_constructed(dev):
    a, b = _constructed(65)
    want = _cross_reference(a, b)
    diag = np.diag(want).tolist()
    assert diag[:5] == [1, 2, 2, 4, 4] and diag[5:] == [66, 66, 0, 0, 0, 0], diag
    pa, pb = _planes(a, dev), _planes(b, dev)
    np.testing.assert_array_equal(ops.mask_cross_stats(pa, pb).cpu().numpy(), want)
    np.testing.assert_array_equal(ops.mask_cross_stats(pb, pa).cpu().numpy(), want.T)
    # the same buffer as both sets: a symmetric matrix with the counts on its diagonal
    same = ops.mask_cross_stats(pa, pa).cpu().numpy()
    np.testing.assert_array_equal(same, _cross_reference(a, a))
    np.testing.assert_array_equal(np.diag(same), pa.count.cpu().numpy())


def test_mask_eval_entry_points_reject_empty_requests(dev):
    from caesar_mrcnn_amd import _hip
    L = _hip.lib()
    t = torch.zeros(64, dtype=torch.int32, device=dev)
    p, s = t.data_ptr(), _hip.current_stream()
    for na, nb, H, W in ((0, 1, 4, 4), (1, 0, 4, 4), (1, 1, 0, 4), (1, 1, 4, 0), (-1, 1, 4, 4)):
        assert L.mrcnn_mask_cross_stats(p, p, na, p, p, nb, H, W, p, s) == -1
    for n, H, W in ((0, 4, 4), (1, 0, 4), (1, 4, 0), (-2, 4, 4)):
        assert L.mrcnn_mask_plane_sums(p, 0, p, p, n, H, W, p, s) == -1
    full = _planes(np.ones((4, 4, 2), bool), dev)
    none = ops.MaskPlanes(full.words[:0], full.count[:0], full.box[:0], 4)
    assert tuple(ops.mask_cross_stats(none, full).shape) == (0, 2) and tuple(ops.mask_cross_stats(full, none).shape) == (2, 0)
    assert tuple(ops.mask_plane_sums(torch.zeros((4, 4), device=dev), none).shape) == (0,)


def _sum_case(W, seed):
    """A seeded image with a NaN strip and one +inf, and planes over it: blobs, one plane that holds the infinity, one that lies in
    the NaN strip only, an empty one and the full frame."""
    H = 33
    rng = np.random.default_rng(seed)
    img = (rng.normal(size=(H, W)) * 10 ** rng.uniform(-3, 3, size=(H, W))).astype(np.float32)
    img[10:13, :] = np.nan
    img[20, W - 1] = np.inf
    m = _blobs(rng, H, W, 7)
    m[20, W - 1, :] = False
    m[:, :, 1] = False
    m[18:23, W - 3:, 1] = True                                                      # holds the +inf
    m[:, :, 2] = False
    m[10:13, 2:W - 1, 2] = True                                                     # NaN only: nansum = 0
    m[:, :, 3] = False                                                              # empty
    m[:, :, 4] = True                                                               # the whole frame
    m[20, W - 1, 4] = False
    return img, m


@pytest.mark.parametrize("W", [33, 65])
def test_mask_plane_sums(dev, W):
    """Against np.nansum of the float64-cast values, within n * 2^-52 * sum|x|: an n-term float64 sum in any order differs from
    the exact sum by at most (n - 1) * 2^-53 * sum|x| (first order), so two such sums differ by at most twice that."""
    img, m = _sum_case(W, 77 + W)
    planes = _planes(m, dev)
    got_t = ops.mask_plane_sums(torch.from_numpy(img).to(dev), planes)
    got = got_t.cpu().numpy()
    assert got.dtype == np.float64
    x64 = img.astype(np.float64)
    for p in range(m.shape[-1]):
        vals = x64[m[:, :, p]]
        want = np.nansum(vals)
        if p == 1:
            assert want == np.inf and got[p] == np.inf
            continue
        finite = vals[~np.isnan(vals)]
        bound = finite.size * EPS * np.abs(finite).sum()
        print("W %d plane %d: n %d, |got - want| %.3e, bound %.3e" % (W, p, finite.size, abs(got[p] - want), bound))
        assert abs(got[p] - want) <= bound, (p, got[p], want, bound)
    assert got[2] == 0.0 and got[3] == 0.0 and m[:, :, 2].any()
    # the file's big-endian bytes give the same bits, and so does a second call
    be = torch.from_numpy(np.ascontiguousarray(img.astype(">f4")).view(np.uint8).reshape(img.shape + (4,))).to(dev)
    again = ops.mask_plane_sums(be, planes, big_endian=True).cpu().numpy()
    np.testing.assert_array_equal(again.view(np.int64), got.view(np.int64))
    twice = ops.mask_plane_sums(torch.from_numpy(img).to(dev), planes).cpu().numpy()
    np.testing.assert_array_equal(twice.view(np.int64), got.view(np.int64))


# ---- the Analyzer's device path against its host statement ---------------------------------------------------------
def _drive(sc, device, path):
    import contextlib
    import io
    from caesar_mrcnn_amd.utils import extract_bboxes
    an = analyze.Analyzer(None, cases.cfg(), cases.StubDataset(sc["consider"]), [], [])
    an.eval_device, an.eval_device_min_pairs = device, 0
    with contextlib.redirect_stdout(io.StringIO()):
        cases.drive(an, sc, extract_bboxes)
        an.image_path = path
        assert an.compute_det_mask_pars() == 0
    return an


def _scene_image(shape, path):
    from caesar_mrcnn_amd import fits
    rng = np.random.default_rng(shape[0] + shape[1])
    img = (rng.normal(size=shape) * 10 ** rng.uniform(-4, 0, size=shape)).astype(np.float32)
    fits.write_fits(path, img)
    return img


def _assert_pars(dev_pars, host_pars, masks, img, rms, what):
    """Every entry equal but Stot, within n * 2^-52 * sum|x| (see test_mask_plane_sums), and snr = (Stot - bkg * n) / (rms * sqrt(n)),
    within that bound divided by rms * sqrt(n) plus four roundings of the result (the subtraction, the product, the root, the
    division)."""
    assert len(dev_pars) == len(host_pars) == len(masks)
    x = np.abs(img.astype(np.float64))
    for a, b, m in zip(dev_pars, host_pars, masks):
        assert (a == {}) == (b == {})
        if not b:
            continue
        n = b["npix"]
        bound = n * EPS * float(x[np.asarray(m) != 0].sum())
        print("%s: npix %d, |dStot| %.3e (bound %.3e), |dsnr| %.3e" % (what, n, abs(a["Stot"] - b["Stot"]), bound, abs(a["snr"] - b["snr"])))
        assert abs(a["Stot"] - b["Stot"]) <= bound, (what, a["Stot"], b["Stot"], bound)
        assert abs(a["snr"] - b["snr"]) <= bound / (rms * np.sqrt(n)) + 4 * EPS * abs(b["snr"]), (what, a["snr"], b["snr"])
        assert {k: v for k, v in a.items() if k not in ("Stot", "snr")} == {k: v for k, v in b.items() if k not in ("Stot", "snr")}, what


@pytest.mark.parametrize("sc", cases.scenarios(), ids=lambda s: s["name"])
def test_analyzer_device_equals_host(dev, sc, tmp_path):
    path = str(tmp_path / "img.fits")
    img = _scene_image(sc["shape"], path)
    got, ref = _drive(sc, True, path), _drive(sc, False, path)
    if len(ref.masks_gt_merged) * len(ref.masks_final) > 0:
        assert got.eval_timing["mask_uploads"] == 2 and "performances_ms" in got.eval_timing and "det_mask_pars_ms" in got.eval_timing
    assert ref.eval_timing == {}
    a, b = cases.analyzer_record(got, sc["shape"]), cases.analyzer_record(ref, sc["shape"])
    assert sorted(a) == sorted(b)
    for k in a:
        assert a[k].shape == b[k].shape and bool(np.all(a[k] == b[k])), (sc["name"], k)
    _assert_pars(got.det_obj_pars, ref.det_obj_pars, ref.masks_final, img, cases.META["rms"], sc["name"])


class _OneImage(object):
    """A dataset of one image for ModelTester, as SourceDataset presents a JSON entry."""

    def __init__(self, image, path, gt_masks, class_ids, class_names, objs, metadata):
        self.nclasses, self.class_names = len(class_names), list(class_names)
        self.consider_sources_near_mixed_sidelobes = True
        self.image_ids = [0]
        self.image_info = [{"id": "scene", "path": path, "class_ids": list(class_ids), "sidelobes_mixed_or_near": [0] * len(class_ids),
                            "objs": objs, "metadata": metadata}]
        self._image, self._gt = image, gt_masks

    def load_image(self, image_id):
        return self._image

    def image_uuid(self, image_id):
        return "scene"

    def image_metadata(self, image_id):
        return self.image_info[0]["metadata"]

    def load_gt_masks(self, image_id, binary=True):
        return self._gt if binary else self._gt.astype(int)

    def load_gt_obj_info(self, image_id):
        return self.image_info[0]["objs"]


def test_model_tester_real_model(dev, tmp_path, monkeypatch):
    """A MaskRCNN with seeded random weights (custom backbone, 128 x 128, score_thr = 0) through ModelTester, the pixel steps on
    the device and on the host: the same two tables in every column but snr, and snr within the bound of the float64 sum."""
    import csv
    import model_cases as T
    import analyze_post_cases as post
    from caesar_mrcnn_amd import fits
    from caesar_mrcnn_amd.model import MaskRCNN
    cfg = T._small_cfg("custom", 128, mode="inference")
    cfg.CLASS_NAMES = list(post.CLASS_NAMES)
    model = MaskRCNN("inference", cfg, "/tmp/mrcnn_logs", device=dev, weights=T._weights(cfg, 3))
    image = T._scene(cfg, 1, 7)[0][0].astype(np.float32)
    path = str(tmp_path / "scene.fits")
    raw = _scene_image((128, 128), path)
    first = model.detect([image], verbose=0)[0]
    n = first["masks"].shape[-1]
    assert n >= 1
    # true objects: the first detections themselves (so that something matches), one of them under another class, and a block
    k = min(n, 3)
    gt = np.concatenate([first["masks"][:, :, :k], post.rect((128, 128), 100, 110, 5, 25)[:, :, None]], axis=-1).astype(bool)
    ids = [int(c) for c in first["class_ids"][:k]] + [1]
    ids[0] = 1 + ids[0] % (cfg.NUM_CLASSES - 1)
    objs = [{"name": "S%d" % (j + 1), "class": cfg.CLASS_NAMES[c], "sidelobe-mixed": 0, "nislands": 1, "border": 0, "snr": 10.0 + j,
             "maxsize_beam": 2.0 + j, "minsize_beam": 1.0} for j, c in enumerate(ids)]
    meta = dict(cases.META, nx=128, ny=128)
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(analyze.Analyzer, "EVAL_DEVICE_MIN_PAIRS", 1)         # the device path whatever the number of pairs

    def run(device):
        ds = _OneImage(image, path, gt, ids, cfg.CLASS_NAMES, objs, meta)
        tester = analyze.ModelTester(model, cfg, ds)
        tester.score_thr, tester.eval_device = 0.0, device
        tester.outfilename_completeness, tester.outfilename_reliability = "c_%d.csv" % device, "r_%d.csv" % device
        kept = {}
        update = tester.update_performances

        def spy(an):
            kept["an"] = an
            return update(an)
        tester.update_performances = spy
        import contextlib
        import io
        with contextlib.redirect_stdout(io.StringIO()):
            assert tester.test() == 0
        tables = []
        for fn in (tester.outfilename_completeness, tester.outfilename_reliability):
            with open(fn) as fp:
                assert fp.read(2) == "# "
                tables.append(list(csv.DictReader(fp)))
        return tester, kept["an"], tables
    t_dev, an_dev, (c_dev, r_dev) = run(True)
    t_host, an_host, (c_host, r_host) = run(False)
    assert an_dev.eval_timing.get("performances_ms") is not None and an_host.eval_timing == {}
    assert len(c_host) == len(ids) and len(r_host) == len(an_host.masks_final) >= 1 and sum(int(r["detected"]) for r in c_host) >= 1
    assert c_dev == c_host                                                   # completeness: its snr is the object info's
    assert len(r_dev) == len(r_host)
    for a, b in zip(r_dev, r_host):
        assert {k: v for k, v in a.items() if k != "snr"} == {k: v for k, v in b.items() if k != "snr"}
    _assert_pars(an_dev.det_obj_pars, an_host.det_obj_pars, an_host.masks_final, raw, meta["rms"], "real model")
    for a, b in zip(r_dev, an_dev.det_obj_pars):
        assert float(a["snr"]) == b["snr"]
    for k in ("classification_matrix", "nobjs_true", "nobjs_det", "nobjs_det_right", "purity"):
        assert np.array_equal(getattr(t_dev, k), getattr(t_host, k)), k
    assert t_dev.detobj_ious == t_host.detobj_ious and t_dev.detobj_scores == t_host.detobj_scores
