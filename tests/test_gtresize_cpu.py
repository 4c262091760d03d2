"""Scaled training samples without a GPU: scipy's nearest-neighbour mask zoom as two index tables
(gtprep.zoom_index_tables) and its statement on the bit-packed layout (gtprep.mask_bits_zoom_host) against utils.resize_mask on
unpacked masks; the sampler's table cache and its hand-over to the host; the library's entry points and the wrappers' refusals;
the switch without device_samples."""
import logging
import os
import sys

import numpy as np
import pytest

from caesar_mrcnn_amd import _hip, gtprep, utils

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_ARG, ERR_WORKSPACE, ERR_UNSUPPORTED = 0, -1, -3, -4
MAX_SIDE, MAX_INSTANCES = 8192, 4096
NEW_SYMBOLS = ("mrcnn_mask_bits_zoom_check", "mrcnn_mask_bits_zoom", "mrcnn_resize_image_u8")
COUNTS = (1, 32, 33, 70)                                   # nb = 4, 4, 8, 12
PADS = (((0, 0), (0, 0)), ((0, 3), (0, 2)), ((2, 0), (5, 0)), ((2, 3), (4, 1)))      # none, one side (after / before), both sides


def _cases():
    """The fixed (h, w, scale) and 50 seeded random ones: 1 <= h, w < 90, scales from 0.5 to the one that brings the short side to
    64, every zoomed side at least one pixel."""
    cases = [(32, 32, 1.5), (28, 30, 0.5), (90, 60, 64 / 90), (1, 7, 3.0), (29, 61, 1.5), (255, 40, 1.37)]
    r = np.random.RandomState(2024)
    while len(cases) < 56:
        h, w = (int(v) for v in r.randint(1, 90, 2))
        scale = [0.5, 0.75, 0.9, 1.37, 1.5, 2.0, 64 / min(h, w)][r.randint(7)]
        if scale != 1 and round(h * scale) >= 1 and round(w * scale) >= 1:
            cases.append((h, w, scale))
    return cases


CASES = _cases()


def _unpacked(packed, n):
    bits = np.unpackbits(packed, axis=-1, bitorder="little")
    assert not bits[:, :, n:].any()                       # the padding bits stay clear
    return bits[:, :, :n].astype(bool)


def test_tables_and_packed_zoom_equal_resize_mask():
    constants = 0
    for k, (h, w, scale) in enumerate(CASES):
        iy, ix = gtprep.zoom_index_tables(h, w, scale)
        assert iy.dtype == np.int32 and ix.dtype == np.int32 and iy.ndim == 1 and ix.ndim == 1
        assert (iy.size, ix.size) == (round(h * scale), round(w * scale)), (h, w, scale)
        assert iy.min() >= -1 and iy.max() < h and ix.min() >= -1 and ix.max() < w
        constants += int((iy < 0).sum() + (ix < 0).sum())
        counts = COUNTS if k < 6 else (COUNTS[k % 4],)
        for n in counts:
            mask = np.random.RandomState(1000 * k + n).rand(h, w, n) > 0.5
            packed = gtprep.mask_bits_pack(mask)
            assert packed.shape[2] == {1: 4, 32: 4, 33: 8, 70: 12}[n]
            for (top, bottom), (left, right) in (PADS if k < 6 else (PADS[k % 4],)):
                want = utils.resize_mask(mask, scale, [(top, bottom), (left, right), (0, 0)])
                OH, OW = iy.size + top + bottom, ix.size + left + right
                assert want.shape == (OH, OW, n), (h, w, scale)
                got = gtprep.mask_bits_zoom_host(packed, iy, ix, top, left, OH, OW)
                assert got.dtype == np.uint8 and got.shape == (OH, OW, packed.shape[2])
                assert np.array_equal(_unpacked(got, n), want), (h, w, scale, n, top, left)
    assert constants > 0                                   # the set reaches scipy's constant: (28, 30, 0.5) ends in one


def test_a_constant_entry_is_where_scipy_writes_zero():
    iy, ix = gtprep.zoom_index_tables(28, 30, 0.5)
    assert iy[-1] == -1 and (iy[:-1] >= 0).all()
    ones = utils.resize_mask(np.ones((28, 30, 1), bool), 0.5, [(0, 0), (0, 0), (0, 0)])
    assert not ones[-1].any() and ones[:-1][:, ix >= 0].all()


def test_zoom_host_refuses_malformed_requests():
    packed = gtprep.mask_bits_pack(np.ones((4, 5, 3), bool))
    for iy, ix, top, left, OH, OW in (([4], [0], 0, 0, 1, 1), ([0], [-2], 0, 0, 1, 1), ([], [0], 0, 0, 1, 1), ([0, 1], [0], 0, 0, 1, 1),
                                      ([0], [0], 1, 0, 1, 1), ([0], [0], 0, -1, 2, 2)):
        with pytest.raises(ValueError):
            gtprep.mask_bits_zoom_host(packed, iy, ix, top, left, OH, OW)
    with pytest.raises(ValueError):
        gtprep.mask_bits_zoom_host(packed.astype(np.int32), [0], [0], 0, 0, 1, 1)


def test_library_exports_the_entry_points_and_the_header_names_them():
    assert set(NEW_SYMBOLS) <= set(_hip.exported_symbols())
    L = _hip.lib()
    header = open(os.path.join(os.path.dirname(_hip.PKG_DIR), "include", "mrcnn_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert callable(getattr(L, name)) and name + "(" in header


def test_check_entry_at_the_caps():
    L = _hip.lib()
    zc = L.mrcnn_mask_bits_zoom_check                      # (h, w, nb, oh, ow, top, left, OH, OW)
    assert zc(32, 32, 4, 48, 48, 8, 8, 64, 64) == OK and zc(1, 1, 4, 1, 1, 0, 0, 1, 1) == OK
    assert zc(MAX_SIDE, MAX_SIDE, MAX_INSTANCES // 8, MAX_SIDE, MAX_SIDE, 0, 0, MAX_SIDE, MAX_SIDE) == OK
    for bad in ((0, 32, 4, 48, 48, 8, 8, 64, 64), (32, 32, 3, 48, 48, 8, 8, 64, 64), (32, 32, 0, 48, 48, 8, 8, 64, 64),
                (32, 32, 4, 0, 48, 8, 8, 64, 64), (32, 32, 4, 48, 48, -1, 8, 64, 64), (32, 32, 4, 48, 48, 17, 8, 64, 64),
                (32, 32, 4, 48, 57, 8, 8, 64, 64), (32, 32, 4, 48, 48, 8, 8, 64, 0), (32, 32, 4, 48, 48, 2 ** 31 - 1, 8, 64, 64)):
        assert zc(*bad) == ERR_ARG, bad
    assert zc(MAX_SIDE + 1, 32, 4, 48, 48, 8, 8, 64, 64) == ERR_UNSUPPORTED
    assert zc(32, 32, 4, 48, 48, 8, 8, 64, MAX_SIDE + 1) == ERR_UNSUPPORTED
    assert zc(32, 32, MAX_INSTANCES // 8 + 4, 48, 48, 8, 8, 64, 64) == ERR_UNSUPPORTED
    # the launching entries refuse the same requests before they touch anything (no device here: null pointers are enough)
    assert L.mrcnn_mask_bits_zoom(None, MAX_SIDE + 1, 32, 4, None, 48, None, 48, 8, 8, 64, 64, None, None) == ERR_UNSUPPORTED
    assert L.mrcnn_mask_bits_zoom(None, 32, 32, 4, None, 48, None, 48, 8, 8, 64, 64, None, None) == ERR_ARG
    assert L.mrcnn_resize_image_u8(None, 32, 32, 3, 48, 48, 8, 8, 64, 64, None, None, 0, None) == ERR_ARG


def test_wrappers_refuse_before_they_need_a_device():
    import torch
    from caesar_mrcnn_amd import ops
    good = torch.zeros((4, 4, 4), dtype=torch.uint8)
    iy = ix = np.zeros(6, np.int32)
    for bad in (np.zeros((4, 4, 4), np.uint8), good.to(torch.int32), good[0], torch.zeros((4, 4, 3), dtype=torch.uint8)):
        with pytest.raises(ValueError):
            ops.mask_bits_zoom(bad, iy, ix, (1, 1), (8, 8))
    for t in ([4] * 6, [-2] * 6, [], [[0]], [0.5], torch.zeros(6, dtype=torch.int64), torch.zeros((2, 3), dtype=torch.int32)):
        with pytest.raises(ValueError):
            ops.mask_bits_zoom(good, t, ix, (1, 1), (8, 8))
        with pytest.raises(ValueError):
            ops.mask_bits_zoom(good, iy, t, (1, 1), (8, 8))
    for pad_tl, canvas in (((-1, 0), (8, 8)), ((3, 0), (8, 8)), ((0, 0), (8, 5)), ((0, 0), (0, 8)), (0, (8, 8)), ((0, 0), (8, 8, 8))):
        with pytest.raises(ValueError):
            ops.mask_bits_zoom(good, iy, ix, pad_tl, canvas)
    with pytest.raises(ValueError):
        ops.mask_bits_zoom(good, iy, ix, (1, 1), (8, 8), out=torch.zeros((8, 8, 8), dtype=torch.uint8))
    with pytest.raises(ops.GtPrepUnsupported):
        ops.mask_bits_zoom(torch.zeros((1, MAX_SIDE + 1, 4), dtype=torch.uint8), [0], [0], (0, 0), (1, 1))
    with pytest.raises(ops.GtPrepUnsupported):
        ops.mask_bits_zoom(good, [0], [0], (0, 0), (1, MAX_SIDE + 1))
    with pytest.raises(ops.GtPrepUnsupported):
        ops.gtprep_zoom_check(4, 4, 4, 1, 1, 0, 0, MAX_SIDE + 1, 1)
    ops.gtprep_zoom_check(32, 32, 4, 48, 48, 8, 8, 64, 64)
    img = torch.zeros((4, 4, 3), dtype=torch.uint8)
    for bad in (np.zeros((4, 4, 3), np.uint8), img.to(torch.float32), img[0], torch.zeros((4, 4, 5), dtype=torch.uint8),
                img.permute(1, 0, 2)[:, :2]):
        with pytest.raises(ValueError):
            ops.resize_image_u8(bad, (6, 6), (1, 1), (8, 8))
    for out_hw, pad_tl, canvas in (((0, 6), (1, 1), (8, 8)), ((6, 6), (-1, 1), (8, 8)), ((6, 6), (3, 1), (8, 8)), ((6, 6), (1, 1), (8, 6)),
                                   (6, (1, 1), (8, 8)), ((6, 6), (1, 1), (8,))):
        with pytest.raises(ValueError):
            ops.resize_image_u8(img, out_hw, pad_tl, canvas)
    with pytest.raises(ValueError):
        ops.resize_image_u8(img, (6, 6), (1, 1), (8, 8), out=torch.zeros((8, 8, 4), dtype=torch.uint8))
    # well-formed requests get as far as asking for a device tensor
    with pytest.raises(_hip.HipPathError):
        ops.mask_bits_zoom(good, iy, ix, (1, 1), (8, 8))
    with pytest.raises(_hip.HipPathError):
        ops.resize_image_u8(img, (6, 6), (1, 1), (8, 8))


# ---- the sampler and the generator ---------------------------------------------------------------------------------
class _Toy(object):
    """Duck-typed like mrcnn.utils.Dataset as load_image_gt uses it: 32 x 32 images, which IMAGE_MIN_DIM = 48 scales by 1.5."""

    def __init__(self, n=5, size=32):
        self.image_ids = np.arange(n)
        self.image_info = [{"source": "toy", "id": i} for i in range(n)]
        self.num_classes = 4
        self.source_class_ids = {"toy": [0, 1, 2, 3]}
        self.size = size

    def _make(self, i):
        r = np.random.RandomState(300 + i)
        img = r.randint(0, 255, (self.size, self.size, 3)).astype(np.uint8)
        k = r.randint(1, 6)
        mask = np.zeros((self.size, self.size, k), bool)
        for g in range(k):
            y, x = r.randint(0, self.size - 12, 2)
            mask[y:y + r.randint(2, 12), x:x + r.randint(2, 12), g] = True
        return img, mask, r.randint(1, 4, k).astype(np.int32)

    def load_image(self, i):
        return self._make(i)[0]

    def load_mask(self, i):
        return self._make(i)[1], self._make(i)[2]


def _cfg():
    from caesar_mrcnn_amd.config import run_py_config
    cfg = run_py_config(backbone="custom", imgsize=64)
    cfg.IMAGE_MIN_DIM = 48
    cfg.MAX_GT_INSTANCES = 8
    return cfg


def test_the_table_cache_is_bounded_and_drops_the_oldest():
    sampler = gtprep.DeviceSampler(_cfg(), "cuda:0", resize=True)
    first = sampler.zoom_tables(5, 6, 1.5)
    assert sampler.zoom_tables(5, 6, 1.5) is first        # datasets repeat their sizes
    assert np.array_equal(first[0], gtprep.zoom_index_tables(5, 6, 1.5)[0]) and np.array_equal(first[1], gtprep.zoom_index_tables(5, 6, 1.5)[1])
    assert 16 <= gtprep.ZOOM_CACHE_ENTRIES <= 1000
    for k in range(gtprep.ZOOM_CACHE_ENTRIES + 9):
        sampler.zoom_tables(2 + k % 7, 3 + k // 7, 2.0)
        assert len(sampler._zoom) <= gtprep.ZOOM_CACHE_ENTRIES
    assert len(sampler._zoom) == gtprep.ZOOM_CACHE_ENTRIES
    assert (5, 6, 1.5) not in sampler._zoom and (2, 3, 2.0) not in sampler._zoom
    last = gtprep.ZOOM_CACHE_ENTRIES + 8
    assert (2 + last % 7, 3 + last // 7, 2.0) in sampler._zoom
    assert sampler.zoom_tables(5, 6, 1.5) is not first    # rebuilt after it was dropped


def test_table_length_mismatch_sends_the_sample_to_the_host(monkeypatch):
    ds, cfg = _Toy(), _cfg()
    asked = []

    def short_tables(h, w, scale):
        asked.append((h, w, scale))
        return np.zeros(47, np.int32), np.zeros(48, np.int32)
    monkeypatch.setattr(gtprep, "zoom_index_tables", short_tables)
    got = gtprep.DeviceSampler(cfg, "cuda:0", resize=True).load(ds, 0, None)
    assert asked == [(32, 32, 1.5)]
    assert got[0] == "host" and np.array_equal(got[1], ds.load_image(0)) and np.array_equal(got[2], ds.load_mask(0)[0])
    # without the switch the scaled image is the host's before any table is asked for
    got = gtprep.DeviceSampler(cfg, "cuda:0").load(ds, 0, None)
    assert got[0] == "host" and asked == [(32, 32, 1.5)]


@pytest.mark.parametrize("device_targets", [False, True])
def test_the_switch_is_ignored_without_device_samples(device_targets, caplog):
    from caesar_mrcnn_amd.augment import ReferenceAugmenter
    from caesar_mrcnn_amd.config import Config
    from caesar_mrcnn_amd.datagen import data_generator
    ds, cfg = _Toy(), _cfg()
    assert cfg.DEVICE_SAMPLE_RESIZE is False and Config.DEVICE_SAMPLE_RESIZE is False
    assert set(gtprep.counters) == {"device", "host", "scaled"}

    def run(**kw):
        np.random.seed(5)
        gen = data_generator(ds, cfg, shuffle=True, augmentation=ReferenceAugmenter(seed=2), batch_size=2, seed=7,
                             device_targets=device_targets, **kw)
        return [next(gen)[0] for _ in range(3)]
    before = dict(gtprep.counters)
    want = run()
    with caplog.at_level(logging.INFO, logger="mrcnn"):
        got = run(device_resize=True)
    said = [r.getMessage() for r in caplog.records if "device_resize" in r.getMessage()]
    assert len(said) == 1 and "ignored" in said[0]
    assert gtprep.counters == before
    for bw, bg in zip(want, got):
        assert type(bg) is list and len(bg) == 7
        for w, g in zip(bw, bg):
            assert (w is None and g is None) or (isinstance(g, np.ndarray) and g.dtype == w.dtype and np.array_equal(g, w))


def test_run_py_flag_implies_nothing_by_itself(caplog):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import run
    finally:
        sys.path.pop(0)
    with caplog.at_level(logging.INFO, logger="mrcnn"):
        alone = run.build_config(run.parse_args(["train", "--device_sample_resize"]), {"sidelobe": 1, "source": 2, "galaxy": 3})
    said = [r.getMessage() for r in caplog.records if "device_sample_resize" in r.getMessage()]
    assert len(said) == 1 and "ignored" in said[0]
    assert alone.DEVICE_SAMPLES is False and alone.DEVICE_SAMPLE_RESIZE is False
    caplog.clear()
    with caplog.at_level(logging.INFO, logger="mrcnn"):
        both = run.build_config(run.parse_args(["train", "--device_samples", "--device_sample_resize"]), {"sidelobe": 1, "source": 2, "galaxy": 3})
        plain = run.build_config(run.parse_args(["train", "--device_samples"]), {"sidelobe": 1, "source": 2, "galaxy": 3})
    assert not [r for r in caplog.records if "device_sample_resize" in r.getMessage()]
    assert both.DEVICE_SAMPLES is True and both.DEVICE_SAMPLE_RESIZE is True
    assert plain.DEVICE_SAMPLES is True and plain.DEVICE_SAMPLE_RESIZE is False
