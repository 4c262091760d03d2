"""Ground-truth preparation on bit-packed masks without a GPU: the NumPy statements the kernels are held to
(gtprep.mask_bits_stats_host / mask_bits_gather_host) against np.sum, utils.extract_bboxes and fancy indexing; the library's
entry points and their refusals; data_generator(device_samples=True) without a device is the host generator."""
import logging

import numpy as np
import pytest

from caesar_mrcnn_amd import _hip, gtprep, utils

OK, ERR_ARG, ERR_WORKSPACE, ERR_UNSUPPORTED = 0, -1, -3, -4
MAX_SIDE, MAX_INSTANCES = 8192, 4096
NEW_SYMBOLS = ("mrcnn_mask_bits_stats_check", "mrcnn_mask_bits_stats_workspace", "mrcnn_mask_bits_stats",
               "mrcnn_mask_bits_gather_check", "mrcnn_mask_bits_gather")


def _masks(H, W, n, seed):
    r = np.random.RandomState(seed)
    m = r.rand(H, W, n) > 0.7
    m[:, :, r.randint(n)] = False                         # an empty instance
    return m


@pytest.mark.parametrize("shape", [(1, 1, 1), (5, 7, 9), (33, 65, 31), (20, 12, 70)])
def test_stats_statement_is_sum_and_extract_bboxes(shape):
    H, W, n = shape
    m = _masks(H, W, n, n)
    packed = gtprep.mask_bits_pack(m)
    assert packed.dtype == np.uint8 and packed.shape == (H, W, 4 * -(-n // 32)) and packed.flags.c_contiguous
    assert np.array_equal(packed[:, :, :(n + 7) // 8], np.packbits(m, axis=-1, bitorder="little"))
    count, box = gtprep.mask_bits_stats_host(packed, n)
    assert count.dtype == np.int32 and box.dtype == np.int32
    assert np.array_equal(count, np.sum(m, axis=(0, 1)))
    assert np.array_equal(box, utils.extract_bboxes(m))
    # the padding bits do not count, whatever they hold
    bits = np.unpackbits(packed, axis=-1, bitorder="little")
    bits[:, :, n:] = 1
    dirty = np.packbits(bits, axis=-1, bitorder="little")
    assert dirty.shape == packed.shape and not np.array_equal(dirty, packed)
    c2, b2 = gtprep.mask_bits_stats_host(dirty, n)
    assert np.array_equal(c2, count) and np.array_equal(b2, box)
    # uint8 masks pack as != 0
    assert np.array_equal(gtprep.mask_bits_pack(m.astype(np.uint8) * 7), packed)


def test_gather_statement_is_fancy_indexing_and_padding():
    H, W, n = 9, 11, 37
    m = _masks(H, W, n, 3)
    packed = gtprep.mask_bits_pack(m)
    r = np.random.RandomState(0)
    for sel, G in (([], 8), (np.arange(n), 40), (r.permutation(n)[:10], 10), (r.permutation(n)[:5], 300)):
        sel = np.asarray(sel, dtype=np.int64)
        want = np.pad(m[:, :, sel].astype(np.uint8), ((0, 0), (0, 0), (0, G - sel.size)))
        got = gtprep.mask_bits_gather_host(packed, sel, G)
        assert got.dtype == np.uint8 and np.array_equal(got, want)
    with pytest.raises(ValueError):
        gtprep.mask_bits_gather_host(packed, [0, 1, 2], 2)
    with pytest.raises(ValueError):
        gtprep.mask_bits_gather_host(packed, [8 * packed.shape[2]], 8)
    with pytest.raises(ValueError):
        gtprep.mask_bits_stats_host(packed, 8 * packed.shape[2] + 1)


def test_library_exports_the_entry_points_and_the_header_names_them():
    import os
    assert set(NEW_SYMBOLS) <= set(_hip.exported_symbols())
    L = _hip.lib()
    for name in NEW_SYMBOLS:
        assert callable(getattr(L, name))
    header = open(os.path.join(os.path.dirname(_hip.PKG_DIR), "include", "mrcnn_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert name + "(" in header
    assert "#define MRCNN_GTPREP_MAX_SIDE %d" % MAX_SIDE in header and "#define MRCNN_GTPREP_MAX_INSTANCES %d" % MAX_INSTANCES in header
    from caesar_mrcnn_amd import ops
    assert issubclass(ops.GtPrepUnsupported, _hip.HipPathError)
    assert (ops.GTPREP_MAX_SIDE, ops.GTPREP_MAX_INSTANCES) == (MAX_SIDE, MAX_INSTANCES)


def test_check_entries_at_the_caps():
    L = _hip.lib()
    st, ga = L.mrcnn_mask_bits_stats_check, L.mrcnn_mask_bits_gather_check
    assert st(1, 1, 4, 1) == OK and st(256, 256, 40, 300) == OK
    for H, W, nb, n in ((0, 8, 4, 1), (8, 0, 4, 1), (8, 8, 0, 1), (8, 8, 3, 1), (8, 8, 6, 1), (8, 8, 4, 0), (8, 8, 4, -1), (8, 8, 4, 33)):
        assert st(H, W, nb, n) == ERR_ARG, (H, W, nb, n)
    assert st(MAX_SIDE, MAX_SIDE, MAX_INSTANCES // 8, MAX_INSTANCES) == OK
    assert st(MAX_SIDE + 1, 8, 4, 1) == ERR_UNSUPPORTED and st(8, MAX_SIDE + 1, 4, 1) == ERR_UNSUPPORTED
    assert st(8, 8, MAX_INSTANCES // 8 + 4, MAX_INSTANCES + 1) == ERR_UNSUPPORTED
    assert st(8, 8, MAX_INSTANCES // 8 + 4, 5) == ERR_UNSUPPORTED
    assert L.mrcnn_mask_bits_stats_workspace(4) == 32 * 20 and L.mrcnn_mask_bits_stats_workspace(40) == 320 * 20
    assert L.mrcnn_mask_bits_stats_workspace(3) == 0 and L.mrcnn_mask_bits_stats_workspace(MAX_INSTANCES // 8 + 4) == 0
    assert ga(1, 1, 4, 0, 1) == OK and ga(256, 256, 40, 300, 300) == OK
    for H, W, nb, k, G in ((0, 8, 4, 1, 8), (8, 0, 4, 1, 8), (8, 8, 5, 1, 8), (8, 8, 4, -1, 8), (8, 8, 4, 9, 8), (8, 8, 4, 0, 0)):
        assert ga(H, W, nb, k, G) == ERR_ARG, (H, W, nb, k, G)
    assert ga(MAX_SIDE, MAX_SIDE, MAX_INSTANCES // 8, MAX_INSTANCES, MAX_INSTANCES) == OK
    assert ga(MAX_SIDE + 1, 8, 4, 1, 8) == ERR_UNSUPPORTED and ga(8, MAX_SIDE + 1, 4, 1, 8) == ERR_UNSUPPORTED
    assert ga(8, 8, 4, 1, MAX_INSTANCES + 1) == ERR_UNSUPPORTED and ga(8, 8, MAX_INSTANCES // 8 + 4, 1, 8) == ERR_UNSUPPORTED
    # the launching entries refuse the same requests before they touch anything (no device here: null pointers are enough)
    assert L.mrcnn_mask_bits_stats(None, MAX_SIDE + 1, 8, 4, 1, None, None, None, 0, None) == ERR_UNSUPPORTED
    assert L.mrcnn_mask_bits_stats(None, 8, 8, 4, 1, None, None, None, 0, None) == ERR_ARG
    assert L.mrcnn_mask_bits_gather(None, 8, 8, 4, None, 1, MAX_INSTANCES + 1, None, None) == ERR_UNSUPPORTED
    assert L.mrcnn_mask_bits_gather(None, 8, 8, 4, None, 0, 8, None, None) == ERR_ARG


def test_wrappers_refuse_before_they_need_a_device():
    import torch
    from caesar_mrcnn_amd import ops
    good = torch.zeros((4, 4, 4), dtype=torch.uint8)
    for bad in (np.zeros((4, 4, 4), np.uint8), good.to(torch.int32), good[0], torch.zeros((4, 4, 3), dtype=torch.uint8)):
        with pytest.raises(ValueError):
            ops.mask_bits_stats(bad, 1)
        with pytest.raises(ValueError):
            ops.mask_bits_gather(bad, [0], 8)
    for n in (0, 33):
        with pytest.raises(ValueError):
            ops.mask_bits_stats(good, n)
    for sel, G in (([32], 8), ([-1], 8), ([0, 1, 2], 2), ([[0]], 8), ([0.5], 8), ([0], 0)):
        with pytest.raises(ValueError):
            ops.mask_bits_gather(good, sel, G)
    with pytest.raises(ValueError):
        ops.mask_bits_gather(good, [0], 8, out=torch.zeros((4, 4, 9), dtype=torch.uint8))
    wide = torch.zeros((1, MAX_SIDE + 1, 4), dtype=torch.uint8)
    with pytest.raises(ops.GtPrepUnsupported):
        ops.mask_bits_stats(wide, 1)
    with pytest.raises(ops.GtPrepUnsupported):
        ops.mask_bits_gather(wide, [0], 8)
    with pytest.raises(ops.GtPrepUnsupported):
        ops.mask_bits_gather(good, [0], MAX_INSTANCES + 1)
    with pytest.raises(ops.GtPrepUnsupported):
        ops.gtprep_check(8, 8, 4, 1, MAX_INSTANCES + 1)
    ops.gtprep_check(256, 256, 40, 300, 300)


class _Toy(object):
    """Duck-typed like mrcnn.utils.Dataset as load_image_gt uses it."""

    def __init__(self, n=5, size=64):
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


def _cfg(size=64):
    from caesar_mrcnn_amd.config import run_py_config
    cfg = run_py_config(backbone="custom", imgsize=size)
    cfg.MAX_GT_INSTANCES = 8
    return cfg


@pytest.mark.parametrize("device_targets", [False, True])
def test_device_samples_without_a_device_is_the_host_generator(device_targets, caplog):
    from caesar_mrcnn_amd.augment import ReferenceAugmenter
    from caesar_mrcnn_amd.datagen import data_generator
    ds, cfg = _Toy(), _cfg()
    assert cfg.DEVICE_SAMPLES is False

    def run(**kw):
        np.random.seed(5)
        gen = data_generator(ds, cfg, shuffle=True, augmentation=ReferenceAugmenter(seed=2), batch_size=2, seed=7,
                             device_targets=device_targets, **kw)
        return [next(gen)[0] for _ in range(3)]
    want = run()
    with caplog.at_level(logging.INFO, logger="mrcnn"):
        got = run(device_samples=True)
    said = [r for r in caplog.records if "device_samples" in r.getMessage()]
    assert len(said) == 1 and "no GPU" in said[0].getMessage()
    for bw, bg in zip(want, got):
        assert type(bg) is list and len(bg) == 7
        for w, g in zip(bw, bg):
            assert (w is None and g is None) or (isinstance(g, np.ndarray) and g.dtype == w.dtype and np.array_equal(g, w))


def test_whole_generator_refusals_name_their_reason():
    from caesar_mrcnn_amd.augment import ReferenceAugmenter
    cfg = _cfg()
    assert "no GPU" in gtprep.generator_refusal(cfg, None, False, None)
    assert "no GPU" in gtprep.generator_refusal(cfg, "cpu", False, None)
    try:
        import torch
        has_gpu = torch.cuda.is_available()
    except Exception:
        has_gpu = False
    if has_gpu:
        assert gtprep.generator_refusal(cfg, "cuda:0", False, None) is None
        assert gtprep.generator_refusal(cfg, "cuda:0", False, ReferenceAugmenter()) is None
        assert "augment=True" in gtprep.generator_refusal(cfg, "cuda:0", True, None)
        assert "ReferenceAugmenter" in gtprep.generator_refusal(cfg, "cuda:0", False, lambda i, m: (i, m))
        cfg.USE_MINI_MASK = True
        assert "USE_MINI_MASK" in gtprep.generator_refusal(cfg, "cuda:0", False, None)
        cfg.USE_MINI_MASK, cfg.IMAGE_RESIZE_MODE = False, "crop"
        assert "crop" in gtprep.generator_refusal(cfg, "cuda:0", False, None)
