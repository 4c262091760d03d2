"""The reference's training augmentation (caesar_mrcnn_amd.augment): sampler, the float64 host statement against a second
source (scipy.ndimage.map_coordinates), exact cases, masks, the path through load_image_gt and the CLI flag.  No GPU."""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _aug():
    from caesar_mrcnn_amd import augment
    return augment


def _coords(m, H, W):
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    return m[0, 0] * xs + m[0, 1] * ys + m[0, 2], m[1, 0] * xs + m[1, 1] * ys + m[1, 2]


# ---- 1. sampler -----------------------------------------------------------------------------------------------------------
def test_sampler_distribution_and_ranges():
    A = _aug()
    rng = np.random.RandomState(0)
    plans = [A.ReferenceAugmenter.draw(rng) for _ in range(30000)]
    counts = np.bincount([len(p) for p in plans], minlength=3)
    assert counts.sum() == 30000 and len(counts) == 3
    assert np.all(np.abs(counts / 30000.0 - 1.0 / 3.0) < 0.02), counts
    pairs = set()
    for p in plans:
        kinds = [s[0] for s in p]
        assert len(set(kinds)) == len(kinds) and set(kinds) <= set(A.STAGES)
        if len(kinds) == 2:
            pairs.add(tuple(kinds))
        for s in p:
            if s[0] == "rotate":
                assert len(s) == 2 and -90.0 <= s[1] <= 90.0
            elif s[0] == "translate":
                assert len(s) == 3 and -0.3 <= s[1] <= 0.3 and -0.3 <= s[2] <= 0.3
            else:
                assert len(s) == 1
    assert pairs == {(a, b) for a in A.STAGES for b in A.STAGES if a != b}      # both orders of every pair
    again = [A.ReferenceAugmenter.draw(np.random.RandomState(0)) for _ in range(1)]
    assert again[0] == plans[0]
    r1, r2 = np.random.RandomState(7), np.random.RandomState(7)
    assert [A.ReferenceAugmenter.draw(r1) for _ in range(200)] == [A.ReferenceAugmenter.draw(r2) for _ in range(200)]
    a1, a2 = A.ReferenceAugmenter(seed=3), A.ReferenceAugmenter(seed=3)
    assert [a1.draw(a1._rng) for _ in range(50)] == [a2.draw(a2._rng) for _ in range(50)]


# ---- 2. second source -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(256, 256, 3), (37, 53, 3)])
def test_warp_host_matches_map_coordinates(shape):
    import scipy.ndimage as ndi
    A = _aug()
    H, W, C = shape
    img = np.random.RandomState(H).randint(0, 256, shape).astype(np.uint8)
    stages = [("rotate", d) for d in (37.3, -37.3, 89.9, -89.9, 0.001)] + \
             [("translate", 0.3, 0.0), ("translate", -0.3, 0.0), ("translate", 0.0, 0.3), ("translate", 0.0, -0.3),
              ("translate", 0.3, -0.3)]
    for st in stages:
        m = A.stage_matrix(st, H, W)
        sx, sy = _coords(m, H, W)
        ref = np.stack([ndi.map_coordinates(img[..., c].astype(np.float64), [sy, sx], order=1, mode="grid-constant", cval=0.0)
                        for c in range(C)], axis=-1)
        got = A.warp_host(img.astype(np.float64), m, "image")
        assert got.dtype == np.float64 and got.shape == shape
        np.testing.assert_allclose(got, ref, rtol=0, atol=1e-9, err_msg=str(st))
        u8 = A.warp_host(img, m, "image")
        assert u8.dtype == np.uint8 and u8.shape == shape
        # exact wherever the value is not a rounding tie.  At a tie (k + 0.5 within 1e-9: common with a 0.1-pixel shift, whose
        # weights 0.9 / 0.1 make 9 a + b = 10 k + 5 a tie) the two sources differ in the last bits and may round apart.
        clear = np.abs(ref - np.floor(ref) - 0.5) > 1e-9
        assert clear.mean() > 0.8, st
        assert np.array_equal(u8[clear], np.rint(ref[clear]).astype(np.uint8)), st
        assert np.all(np.abs(u8[~clear].astype(int) - ref[~clear]) <= 0.5 + 1e-9), st


# ---- 3. exact cases -------------------------------------------------------------------------------------------------------
def test_exact_cases():
    A = _aug()
    sq = np.random.RandomState(1).randint(0, 256, (64, 64, 3)).astype(np.uint8)
    mk = np.random.RandomState(2).rand(64, 64, 5) > 0.7
    H, W = 64, 64

    def both(st):
        m = A.stage_matrix(st, H, W)
        return A.warp_host(sq, m, "image"), A.warp_host(mk, m, "mask")
    ident = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
    assert np.array_equal(A.warp_host(sq, ident, "image"), sq) and np.array_equal(A.warp_host(mk, ident, "mask"), mk)
    i, m = both(("fliplr",))
    assert np.array_equal(i, np.fliplr(sq)) and np.array_equal(m, np.fliplr(mk))
    i, m = both(("flipud",))
    assert np.array_equal(i, np.flipud(sq)) and np.array_equal(m, np.flipud(mk))
    i, m = both(("rotate", 90.0))
    assert np.array_equal(i, np.rot90(sq, -1)) and np.array_equal(m, np.rot90(mk, -1))
    i, m = both(("rotate", -90.0))
    assert np.array_equal(i, np.rot90(sq, 1)) and np.array_equal(m, np.rot90(mk, 1))
    # whole-pixel translation: (tx, ty) = (16, -8) -> out[y, x] = src[y + 8, x - 16], zero fill
    i, m = both(("translate", 0.25, -0.125))
    want = np.zeros_like(sq)
    want[:H - 8, 16:] = sq[8:, :W - 16]
    wantm = np.zeros_like(mk)
    wantm[:H - 8, 16:] = mk[8:, :W - 16]
    assert np.array_equal(i, want) and np.array_equal(m, wantm)
    # a non-square image keeps its shape (and a float image its dtype)
    ns = np.random.RandomState(3).randint(0, 256, (37, 53, 3)).astype(np.uint8)
    for st in (("rotate", 90.0), ("rotate", 37.3), ("translate", 0.3, -0.3), ("fliplr",), ("flipud",)):
        m = A.stage_matrix(st, 37, 53)
        assert A.warp_host(ns, m, "image").shape == (37, 53, 3)
        assert A.warp_host(ns[..., 0], m, "image").shape == (37, 53)
        assert A.warp_host(ns.astype(np.float32), m, "image").dtype == np.float32
    aug = A.ReferenceAugmenter()
    i, m = aug.apply(ns, np.zeros((37, 53, 2), bool), [("rotate", 90.0), ("translate", 0.1, 0.2)])
    assert i.shape == (37, 53, 3) and m.shape == (37, 53, 2)


# ---- 4. masks -------------------------------------------------------------------------------------------------------------
def test_mask_half_pixel_tie_and_rounding_between_stages():
    A = _aug()
    H, W = 32, 40
    mk = np.zeros((H, W, 1), bool)
    mk[10, 10, 0] = True
    m = A.stage_matrix(("translate", 0.5 / W, 0.0), H, W)
    v = A.warp_host(mk.astype(np.float64), m, "image")
    assert v[10, 10, 0] == 0.5 and v[10, 11, 0] == 0.5 and v.sum() == 1.0          # both neighbours exactly 0.5 ...
    assert not A.warp_host(mk, m, "mask").any()                                      # ... so neither is set
    # two half-pixel stages: rounded in between (the reference's order) the instance is gone; one composed 1-pixel shift
    # would keep it
    aug = A.ReferenceAugmenter()
    img = np.zeros((H, W, 3), np.uint8)
    img[10, 10] = 201
    stages = [("translate", 0.5 / W, 0.0), ("translate", 0.5 / W, 0.0)]
    i2, m2 = aug.apply(img, mk, stages)
    m1, mb = (np.vstack([x, [0, 0, 1]]) for x in A.ReferenceAugmenter.matrices(stages, H, W))
    composed = (m1 @ mb)[:2]                          # output -> stage-2 source -> stage-1 source
    assert np.array_equal(composed, [[1, 0, -1.0], [0, 1, 0]])
    want_i, want_m = img, mk
    for mm in A.ReferenceAugmenter.matrices(stages, H, W):
        want_i, want_m = A.warp_host(want_i, mm, "image"), A.warp_host(want_m, mm, "mask")
    assert np.array_equal(i2, want_i) and np.array_equal(m2, want_m)
    assert not m2.any() and A.warp_host(mk, composed, "mask")[10, 11, 0]
    # image: 201 -> 100.5 / 100.5 -> rint 100 / 100 -> 50 / 100 / 50; the composed shift moves 201 whole
    assert list(i2[10, 9:13, 0]) == [0, 50, 100, 50] and A.warp_host(img, composed, "image")[10, 11, 0] == 201
    # a rotation + translation on random masks: bool in, bool out, equal to the per-plane host statement of a float image
    rng = np.random.RandomState(4)
    big = rng.rand(24, 28, 40) > 0.6
    for mm in A.ReferenceAugmenter.matrices([("rotate", 33.0), ("translate", 0.13, -0.21)], 24, 28):
        got = A.warp_host(big, mm, "mask")
        assert got.dtype == bool and np.array_equal(got, A.warp_host(big.astype(np.float64), mm, "image") > 0.5)
        big = got


# ---- 5. through load_image_gt ---------------------------------------------------------------------------------------------
class _Toy(object):
    """Duck-typed like mrcnn.utils.Dataset as load_image_gt uses it: one 128 x 128 image, an instance near the left edge
    (class 1) and one in the middle (class 2)."""
    image_ids = np.arange(1)
    image_info = [{"source": "toy", "id": 0}]
    num_classes = 3
    source_class_ids = {"toy": [0, 1, 2]}

    def load_image(self, i):
        img = np.random.RandomState(5).randint(0, 40, (128, 128, 3)).astype(np.uint8)
        img[40:60, 4:24] = 220
        img[50:80, 60:90] = 180
        return img

    def load_mask(self, i):
        mk = np.zeros((128, 128, 2), bool)
        mk[40:60, 4:24, 0] = True
        mk[50:80, 60:90, 1] = True
        return mk, np.array([1, 2], np.int32)


def _gen_cfg():
    from caesar_mrcnn_amd.config import run_py_config
    cfg = run_py_config(backbone="custom", imgsize=128)
    cfg.MAX_GT_INSTANCES = 10
    return cfg


def test_load_image_gt_drops_instances_pushed_out_of_frame():
    from caesar_mrcnn_amd import utils
    from caesar_mrcnn_amd.datagen import load_image_gt
    A = _aug()
    aug = A.ReferenceAugmenter()
    plan = [("translate", -0.3, 0.0), ("rotate", 10.0)]          # 38.4 px to the left: the left instance leaves the frame

    def fixed(image, mask):
        return aug.apply(image, mask, plan)
    img, meta, ids, boxes, masks = load_image_gt(_Toy(), _gen_cfg(), 0, augmentation=fixed)
    assert img.shape == (128, 128, 3) and img.dtype == np.uint8
    assert list(ids) == [2] and masks.shape == (128, 128, 1) and masks.dtype == bool
    assert np.array_equal(boxes, utils.extract_bboxes(masks))
    want_i, _, _, _, raw = load_image_gt(_Toy(), _gen_cfg(), 0)
    want_m = raw
    for m in aug.matrices(plan, 128, 128):
        want_i, want_m = A.warp_host(want_i, m, "image"), A.warp_host(want_m, m, "mask")
    assert np.array_equal(img, want_i) and np.array_equal(masks[..., 0], want_m[..., 1]) and not want_m[..., 0].any()
    # the shared callable: draws its own plans, keeps shapes, boxes follow the masks
    aug = A.ReferenceAugmenter(seed=0)
    for _ in range(6):
        img, meta, ids, boxes, masks = load_image_gt(_Toy(), _gen_cfg(), 0, augmentation=aug)
        assert img.shape == (128, 128, 3) and masks.shape[:2] == (128, 128) and len(ids) == masks.shape[2]
        assert np.array_equal(boxes, utils.extract_bboxes(masks)) and masks.any(axis=(0, 1)).all()
    assert aug.device_calls == 0


# ---- 6. CLI ---------------------------------------------------------------------------------------------------------------
def _run_module():
    spec = importlib.util.spec_from_file_location("_mrcnn_run_cli", os.path.join(ROOT, "scripts", "run.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_cli_reference_augmentation_flag():
    run = _run_module()
    A = _aug()
    args = run.parse_args(["train"])
    assert args.reference_augmentation is False and args.use_augmentation is True
    default = run.build_augmentation(args)
    assert callable(default) and not isinstance(default, A.ReferenceAugmenter)
    img = np.random.RandomState(6).randint(0, 256, (16, 16, 3)).astype(np.uint8)
    mk = np.random.RandomState(7).rand(16, 16, 2) > 0.5
    dihedral = [np.rot90(f, k) for f in (img, np.fliplr(img)) for k in range(4)]
    for _ in range(8):                                       # the flips / rot90 callable: always one of the 8 symmetries
        i, m = default(img, mk)
        assert any(np.array_equal(i, d) for d in dihedral) and m.shape == mk.shape
    ref = run.build_augmentation(run.parse_args(["train", "--reference_augmentation"]))
    assert isinstance(ref, A.ReferenceAugmenter) and ref.device is None
    assert run.build_augmentation(run.parse_args(["train", "--reference_augmentation", "--no_augmentation"])) is None
    assert run.build_augmentation(run.parse_args(["train", "--no_augmentation"])) is None
