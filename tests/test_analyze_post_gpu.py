"""The bit-plane kernels of csrc/maskgraph.hip against NumPy, and Analyzer's device path against its host statement: exact
equality throughout.  Frames are at most 132 x 132 with at most 24 masks (the pack test's n = 100 runs at 3 x 33)."""
import numpy as np
import pytest
import torch

import caesar_mrcnn_amd  # noqa: F401
from caesar_mrcnn_amd import analyze, ops
from caesar_mrcnn_amd.utils import extract_bboxes

import analyze_post_cases as cases

pytestmark = pytest.mark.gpu


def _upload(masks, dev):
    return torch.from_numpy(np.ascontiguousarray(masks).view(np.uint8) if masks.dtype == np.bool_ else np.ascontiguousarray(masks)).to(dev)


def _check_planes(planes, masks_bool):
    """MaskPlanes against the NumPy statement for [H, W, n] bool masks."""
    H, W, n = masks_bool.shape
    assert (planes.n, planes.H, planes.wpr, planes.W) == (n, H, (W + 31) // 32, W)
    np.testing.assert_array_equal(planes.words.cpu().numpy().view(np.uint32), analyze.pack_mask_planes(masks_bool))
    np.testing.assert_array_equal(planes.count.cpu().numpy(), masks_bool.reshape(-1, n).sum(0).astype(np.int32))
    box = planes.box.cpu().numpy()
    assert box.dtype == np.int32
    np.testing.assert_array_equal(box, extract_bboxes(masks_bool))


def _pack_input(H, W, n, seed):
    rng = np.random.default_rng(seed)
    m = (rng.uniform(size=(H, W, n)) < rng.uniform(0.05, 0.7, size=n)).astype(np.uint8)
    m[m != 0] = rng.integers(1, 256, size=int((m != 0).sum()), dtype=np.uint8)       # any nonzero byte is "set"
    special = [np.zeros((H, W), np.uint8), np.full((H, W), 255, np.uint8)]          # an empty plane, a full plane of 255s
    for y, x in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)):                     # one pixel in each corner
        p = np.zeros((H, W), np.uint8)
        p[y, x] = 255
        special.append(p)
    for k, p in enumerate(special[:n]):                                               # spread over the planes (n >= 6: all six)
        m[:, :, k * max(n // 6, 1)] = p
    return m


@pytest.mark.parametrize("H", [1, 3, 132])
@pytest.mark.parametrize("W", [1, 31, 32, 33, 65, 132])
def test_mask_planes_pack(dev, H, W):
    for n in (1, 7, 8, 9) + ((100,) if (H, W) == (3, 33) else ()):
        if n == 1:                                                                     # one plane at a time: each special plane alone
            full = _pack_input(H, W, 6, 100 * H + W)
            for k in range(6):
                m = np.ascontiguousarray(full[:, :, k:k + 1])
                _check_planes(ops.mask_planes_pack(_upload(m, dev)), m != 0)
            continue
        m = _pack_input(H, W, n, 1000 * n + 10 * H + W)
        _check_planes(ops.mask_planes_pack(_upload(m, dev)), m != 0)
    b = _pack_input(H, W, 7, 5) != 0                                                  # a bool tensor is taken as it is
    _check_planes(ops.mask_planes_pack(torch.from_numpy(b).to(dev)), b)


def test_mask_entry_points_reject_empty_requests(dev):
    from caesar_mrcnn_amd import _hip
    L = _hip.lib()
    t = torch.zeros(64, dtype=torch.int32, device=dev)
    p, s = t.data_ptr(), _hip.current_stream()
    for n, H, W in ((0, 4, 4), (4, 0, 4), (4, 4, 0), (-1, 4, 4)):
        assert L.mrcnn_mask_planes_pack(p, H, W, n, p, p, p, s) == -1
        assert L.mrcnn_mask_pair_stats(p, p, n, H, W, p, 1, p, p, s) == -1
        assert L.mrcnn_mask_union(p, n, H, W, p, p, 1, 1, p, p, p, s) == -1
    assert L.mrcnn_mask_pair_stats(p, p, 1, 4, 4, p, 0, p, p, s) == 0 and L.mrcnn_mask_pair_stats(p, p, 1, 4, 4, p, -1, p, p, s) == -1
    with pytest.raises(_hip.HipPathError):
        ops.mask_planes_pack(torch.zeros((4, 4, 0), dtype=torch.uint8, device=dev))


def _pair_reference(masks_bool, pairs):
    n = masks_bool.shape[-1]
    inter, touch = [], []
    for i, j in pairs:
        if not (0 <= i < n and 0 <= j < n):
            inter.append(0); touch.append(0)
            continue
        a, b = masks_bool[:, :, i], masks_bool[:, :, j]
        inter.append(int(np.logical_and(a, b).sum()))
        touch.append(int(analyze.masks_touch4(a, b)))
    return np.array(inter, np.int32), np.array(touch, np.int32)


def _constructed_planes(W):
    """Planes on a 9 x W frame (W = 33 or 65: the last word holds one pixel) and the pairs that probe them."""
    H = 9
    planes, pairs = [], []

    def add(*rects):
        m = np.zeros((H, W), bool)
        for y1, y2, x1, x2 in rects:
            m[y1:y2, x1:x2] = True
        planes.append(m)
        return len(planes) - 1
    a = add((2, 3, 28, 32)); b = add((2, 3, 32, 33))                                 # contact only across x = 31 | 32 ...
    pairs += [(a, b), (b, a)]                                                         # ... in both directions
    c = add((4, 5, 10, 14)); d = add((5, 6, 12, 20))                                  # contact only between rows 4 / 5
    pairs += [(c, d), (d, c)]
    e = add((6, 7, 30, 32)); f = add((7, 8, 32, 33))                                  # diagonal only, across the word boundary: 0
    g = add((7, 8, 5, 6)); h = add((8, 9, 6, 7))                                      # diagonal only, inside a word: 0
    pairs += [(e, f), (f, e), (g, h), (h, g)]
    r0 = add((0, 1, 0, 3)); r0b = add((0, 1, 3, 5))                                   # first row / first column
    c0 = add((1, 4, 0, 1)); last = add((H - 1, H, W - 1, W)); lastb = add((H - 2, H - 1, W - 1, W))       # last row / last column
    pairs += [(r0, r0b), (r0, c0), (c0, r0), (last, lastb), (lastb, last), (r0, last)]
    p = add((2, 3, 2, 3)); q = add((2, 3, 4, 5)); q2 = add((4, 5, 2, 3))              # distance 2
    pairs += [(p, q), (q, p), (p, q2), (q2, p)]
    big = add((0, H, 0, W)); inner = add((3, 6, 8, 30)); same = add((3, 6, 8, 30))    # nested and identical boxes
    ring = add((1, 8, 1, 2), (1, 8, 31, 32), (1, 2, 1, 32), (7, 8, 1, 32))            # boxes nested, pixels apart
    pairs += [(big, inner), (inner, big), (inner, same), (ring, inner), (inner, ring), (big, last)]
    empty = add()
    pairs += [(empty, big), (big, empty), (empty, empty), (big, big), (a, a)]         # one empty plane; the same plane twice
    pairs += [(a, len(planes)), (-1, a), (len(planes) + 5, -3)]                       # out of range
    if W > 64:
        x = add((1, 2, 60, 64)); y = add((1, 2, 64, 65)); z = add((2, 3, 64, 65))      # x = 63 | 64, straight and diagonal
        pairs += [(x, y), (y, x), (x, z), (z, x), (y, z)]
    return np.stack(planes, axis=-1), np.array(pairs, np.int32)


@pytest.mark.parametrize("W", [33, 65])
def test_mask_pair_stats_constructed(dev, W):
    masks, pairs = _constructed_planes(W)
    want_inter, want_touch = _pair_reference(masks, pairs)
    assert masks.shape[-1] <= 24 and want_touch.tolist()[:8] == [1, 1, 1, 1, 0, 0, 0, 0]      # straight contact 1, diagonal contact 0
    planes = ops.mask_planes_pack(_upload(masks, dev))
    inter, touch = ops.mask_pair_stats(planes, pairs)
    np.testing.assert_array_equal(inter.cpu().numpy(), want_inter)
    np.testing.assert_array_equal(touch.cpu().numpy(), want_touch)
    # on the planes of mask_union (every plane its own component) as well, with the pairs already on the device
    n = masks.shape[-1]
    again = ops.mask_union(planes, np.arange(n + 1), np.arange(n))
    inter, touch = ops.mask_pair_stats(again, torch.from_numpy(pairs).to(dev))
    np.testing.assert_array_equal(inter.cpu().numpy(), want_inter)
    np.testing.assert_array_equal(touch.cpu().numpy(), want_touch)


def test_mask_pair_stats_random(dev):
    """300 seeded pairs among 24 planes on a 40 x 70 frame: sparse blobs, so that touching, overlapping and apart all occur."""
    rng = np.random.default_rng(12)
    H, W, n = 40, 70, 24
    masks = np.zeros((H, W, n), bool)
    for d in range(n):
        for _ in range(int(rng.integers(1, 4))):
            y, x = int(rng.integers(0, H)), int(rng.integers(0, W))
            masks[y:y + int(rng.integers(1, 12)), x:x + int(rng.integers(1, 20)), d] = True
        masks[:, :, d] &= rng.uniform(size=(H, W)) < 0.8
    pairs = rng.integers(0, n, size=(300, 2)).astype(np.int32)
    want_inter, want_touch = _pair_reference(masks, pairs)
    assert 60 < int(want_touch.sum()) < 240 and int((want_inter > 0).sum()) > 30 and int(((want_inter == 0) & (want_touch == 1)).sum()) > 5
    planes = ops.mask_planes_pack(_upload(masks, dev))
    inter, touch = ops.mask_pair_stats(planes, pairs)
    np.testing.assert_array_equal(inter.cpu().numpy(), want_inter)
    np.testing.assert_array_equal(touch.cpu().numpy(), want_touch)


@pytest.mark.parametrize("H,W", [(1, 1), (9, 33), (40, 70), (132, 132)])
def test_mask_union(dev, H, W):
    rng = np.random.default_rng(H + W)
    n = 9
    masks = rng.uniform(size=(H, W, n)) < rng.uniform(0.02, 0.3, size=n)
    masks[:, :, 4] = False
    comps = [[0], [1, 1, 1], [2, 3], [], [5, 0, 5, 7], [4], [4, 8], list(range(n)), [8]]        # single, repeated, several, empty
    if H >= 9 and W >= 33:
        masks[:, :, 2] = cases.rect((H, W), 0, 2, 0, 3)
        masks[:, :, 3] = cases.rect((H, W), H - 2, H, W - 3, W)                                  # disjoint members
    planes = ops.mask_planes_pack(_upload(masks, dev))
    offsets = np.concatenate([[0], np.cumsum([len(c) for c in comps])])
    got = ops.mask_union(planes, offsets, [k for c in comps for k in c])
    want = np.zeros((H, W, len(comps)), bool)
    for c, members in enumerate(comps):
        for k in members:
            want[:, :, c] |= masks[:, :, k]
    _check_planes(got, want)
    assert int(got.count[3]) == 0 and got.box[3].tolist() == [0, 0, 0, 0]
    none = ops.mask_union(planes, [0], [])
    assert tuple(none.words.shape) == (0, H, (W + 31) // 32)


@pytest.mark.parametrize("case", cases.scenarios(), ids=lambda c: c[0])
def test_analyzer_device_equals_host(dev, case):
    name, shape, objs, settings = case
    got = cases.run(cases.analyzer(objs, shape, settings, device=True), shape)
    assert got.postprocess_timing["masks"] == len(objs)                             # the device path ran ...
    n_above = sum(1 for o in objs if np.float32(o[2]) >= 0.7)
    assert got.postprocess_timing["mask_uploads"] == (1 if n_above else 0)         # ... on one upload of the stand-in's masks
    ref = cases.run(cases.analyzer(objs, shape, settings, device=False), shape)
    cases.assert_same(got, ref, name)


def test_analyzer_switch(dev):
    """Off until it has been timed against the host statement on the target; has_gpu is what turns it on."""
    name, shape, objs, settings = cases.scenarios()[0]
    an = analyze.Analyzer(cases.StubModel(cases.result(shape, objs)), cases.cfg())
    assert an.postprocess_device is False and an.postprocess_device_min_masks == analyze.Analyzer.POSTPROCESS_DEVICE_MIN_MASKS
    assert analyze.Analyzer.has_gpu(an.model) is True and analyze.Analyzer.has_gpu(None) is True


def test_analyzer_real_model_uses_the_kept_device_tensor(dev):
    """A MaskRCNN with seeded random weights at the suite's smallest configuration: predict() through the device path equals the
    host path on the same detect() output, and works on the tensor the model kept -- no mask is uploaded."""
    import model_cases as T
    from caesar_mrcnn_amd.model import MaskRCNN
    cfg = T._small_cfg("custom", 128, mode="inference")
    cfg.CLASS_NAMES = list(cases.CLASS_NAMES)
    model = MaskRCNN("inference", cfg, "/tmp/mrcnn_logs", device=dev, weights=T._weights(cfg, 3))
    image = T._scene(cfg, 1, 7)[0][0].astype(np.float32)

    def run(device):
        an = analyze.Analyzer(model, cfg)
        an.write_to_json = an.write_to_ds9 = False
        an.score_thr = 0.0                                                            # random weights: keep every detection
        an.postprocess_device = device
        assert an.predict(image, image_id="scene") == 0
        return an
    got, ref = run(True), run(False)
    n = ref.masks.shape[-1]
    assert n >= 1 and np.array_equal(got.masks, ref.masks) and np.array_equal(got.scores, ref.scores)
    kept = model.last_masks_device
    assert len(kept) == 1 and kept[0].is_cuda and tuple(kept[0].shape) == ref.masks.shape
    assert np.array_equal(kept[0].cpu().numpy().view(np.bool_), ref.masks)
    assert got.postprocess_timing["masks"] == n and got.postprocess_timing["mask_uploads"] == 0
    assert ref.postprocess_timing == {}
    assert len(ref.masks_final) >= 1
    cases.assert_same(got, ref, "real model")
    got.masks = got.masks.copy()                                                      # masks assigned by hand: the kept tensor is not
    got.extract_det_masks()                                                           # theirs -> one upload, same lists
    assert got.postprocess_timing["mask_uploads"] == 1
    got.make_json_results()
    got.make_ds9_regions(got.use_polygon_regions)
    cases.assert_same(got, ref, "real model, uploaded")
