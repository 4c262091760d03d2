"""Training samples assembled on the device (csrc/gtprep.hip through ops / gtprep.DeviceSampler / data_generator(device_samples=True)):
the two kernels against their NumPy statements, exactly; the generator against the host generator, item by item and through
MaskRCNN._to_device; four loader threads; MaskRCNN.train() and `run.py train --device_samples`."""
import glob
import logging
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FRAMES = [(1, 1), (5, 7), (33, 65), (64, 130)]          # rows shorter than, equal to (with x = 64 unused) and crossing a 64-lane segment
COUNTS = [1, 7, 8, 9, 31, 32, 33, 70]                   # byte and word boundaries, more than two words
SENTINEL = 0xAB


def _planted(H, W, n, off):
    """Instance i by (i + off) % 5: empty, the full frame, one pixel in each corner, one whole row (row i % H), one pixel."""
    r = np.random.RandomState(H * 1000 + n * 10 + off)
    m = np.zeros((H, W, n), bool)
    for i in range(n):
        kind = (i + off) % 5
        if kind == 1:
            m[:, :, i] = True
        elif kind == 2:
            m[0, 0, i] = m[0, W - 1, i] = m[H - 1, 0, i] = m[H - 1, W - 1, i] = True
        elif kind == 3:
            m[i % H, :, i] = True
        elif kind == 4:
            m[r.randint(H), r.randint(W), i] = True
    return m


def _scenes(H, W, n):
    r = np.random.RandomState(H + 7 * n)
    yield r.rand(H, W, n) > 0.8
    for off in range(5):
        yield _planted(H, W, n, off)


def _pack_dirty(m):
    """The loader's layout with every padding bit >= n set: none may leak into a result."""
    from caesar_mrcnn_amd import gtprep
    bits = np.unpackbits(gtprep.mask_bits_pack(m), axis=-1, bitorder="little")
    bits[:, :, m.shape[2]:] = 1
    return np.packbits(bits, axis=-1, bitorder="little")


@pytest.mark.parametrize("frame", FRAMES)
def test_stats_equal_the_host_statement(dev, frame):
    from caesar_mrcnn_amd import gtprep, ops, utils
    H, W = frame
    for n in COUNTS:
        for m in _scenes(H, W, n):
            packed = _pack_dirty(m)
            count, box = ops.mask_bits_stats(torch.from_numpy(packed).to(dev), n)
            assert count.dtype == torch.int32 and tuple(count.shape) == (n,) and box.dtype == torch.int32 and tuple(box.shape) == (n, 4)
            count, box = count.cpu().numpy(), box.cpu().numpy()
            want_c, want_b = gtprep.mask_bits_stats_host(packed, n)
            assert np.array_equal(count, want_c) and np.array_equal(box, want_b), (H, W, n)
            assert np.array_equal(count, np.sum(m, axis=(0, 1))) and np.array_equal(box, utils.extract_bboxes(m))


@pytest.mark.parametrize("frame", FRAMES)
def test_gather_equals_the_host_statement(dev, frame):
    from caesar_mrcnn_amd import gtprep, ops
    H, W = frame
    for n in COUNTS:
        r = np.random.RandomState(n)
        for m in list(_scenes(H, W, n))[:2]:
            packed = _pack_dirty(m)
            packed_d = torch.from_numpy(packed).to(dev)
            for G in (8, 10, 300):
                full = min(n, G)
                for sel in ([], np.arange(full), r.permutation(n)[:max(1, full // 2)]):
                    sel = np.asarray(sel, dtype=np.int32)
                    batch = torch.full((3, H, W, G), SENTINEL, dtype=torch.uint8, device=dev)
                    out = ops.mask_bits_gather(packed_d, sel, G, out=batch[1])
                    assert out.data_ptr() == batch[1].data_ptr()
                    got = batch.cpu().numpy()
                    assert np.all(got[0] == SENTINEL) and np.all(got[2] == SENTINEL), (H, W, n, G)
                    assert np.array_equal(got[1], gtprep.mask_bits_gather_host(packed, sel, G)), (H, W, n, G, sel)
                    assert np.array_equal(got[1], np.pad(m[:, :, sel].astype(np.uint8), ((0, 0), (0, 0), (0, G - sel.size))))
            fresh = ops.mask_bits_gather(packed_d, [n - 1], 12)                       # no out: allocated here
            assert np.array_equal(fresh.cpu().numpy(), gtprep.mask_bits_gather_host(packed, [n - 1], 12))


def test_wrappers_refuse_and_leave_the_output_alone(dev):
    from caesar_mrcnn_amd import ops
    good = torch.zeros((4, 4, 4), dtype=torch.uint8, device=dev)
    out = torch.full((4, 4, 8), SENTINEL, dtype=torch.uint8, device=dev)
    for bad in (good.to(torch.int32), good[0], good[:, :, :3].contiguous()):
        with pytest.raises(ValueError):
            ops.mask_bits_stats(bad, 1)
        with pytest.raises(ValueError):
            ops.mask_bits_gather(bad, [0], 8, out=out)
    with pytest.raises(ValueError):
        ops.mask_bits_stats(good, 33)
    for sel in ([32], [-1], [0] * 9):
        with pytest.raises(ValueError):
            ops.mask_bits_gather(good, sel, 8, out=out)
    with pytest.raises(ValueError):
        ops.mask_bits_gather(good, [0], 8, out=out[:, :, :4])                        # wrong shape, not contiguous
    wide = torch.zeros((1, ops.GTPREP_MAX_SIDE + 1, 4), dtype=torch.uint8, device=dev)
    wide_out = torch.full((1, ops.GTPREP_MAX_SIDE + 1, 8), SENTINEL, dtype=torch.uint8, device=dev)
    with pytest.raises(ops.GtPrepUnsupported):
        ops.mask_bits_stats(wide, 1)
    with pytest.raises(ops.GtPrepUnsupported):
        ops.mask_bits_gather(wide, [0], 8, out=wide_out)
    with pytest.raises(ops.GtPrepUnsupported):
        ops.mask_bits_gather(good, [0], ops.GTPREP_MAX_INSTANCES + 1)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((wide_out == SENTINEL).all())


# ---- the generator -------------------------------------------------------------------------------------------------
class _Toy(object):
    """Duck-typed like mrcnn.utils.Dataset as load_image_gt uses it (the pattern of test_augment_gpu._Toy) at 64 x 64.  Image 1
    is 56 x 60 (scale 1, padded), image 2 has no instance, image 3 has 9 (above the lowered MAX_GT_INSTANCES), image 4 carries
    uint8 0 / 1 masks; every image has a two-pixel instance in a corner, which most rotations and shifts empty.  `small`: the
    index of an image of 32 x 32, which resize_image scales (the host's sample, in the same batch).  `loads` logs the ids."""

    def __init__(self, n=7, small=None):
        self.image_ids = np.arange(n)
        self.image_info = [{"source": "toy", "id": i} for i in range(n)]
        self.num_classes = 4
        self.source_class_ids = {"toy": [0, 1, 2, 3]}
        self.small = small
        self.loads = []

    def _make(self, i):
        r = np.random.RandomState(500 + i)
        h, w = (56, 60) if i == 1 else (32, 32) if i == self.small else (64, 64)
        img = r.randint(0, 40, (h, w, 3)).astype(np.uint8)
        k = 0 if i == 2 else 9 if i == 3 else r.randint(2, 6)
        mask = np.zeros((h, w, k), bool)
        for g in range(k):
            y, x = r.randint(0, h - 14), r.randint(0, w - 14)
            bh, bw = r.randint(3, 14, 2)
            if g == 0:
                y, x, bh, bw = 0, 0, 1, 2
            mask[y:y + bh, x:x + bw, g] = True
            img[y:y + bh, x:x + bw] = r.randint(100, 256)
        return img, (mask.astype(np.uint8) if i == 4 else mask), r.randint(1, 4, k).astype(np.int32)

    def load_image(self, i):
        self.loads.append(int(i))
        return self._make(i)[0]

    def load_mask(self, i):
        return self._make(i)[1], self._make(i)[2]


def _cfg():
    from caesar_mrcnn_amd.config import run_py_config
    cfg = run_py_config(backbone="custom", imgsize=64)
    cfg.IMAGE_MIN_DIM = 48                                 # 56 x 60 keeps its scale and is padded to 64 x 64; 32 x 32 is scaled by 1.5
    cfg.MAX_GT_INSTANCES = 6
    cfg.TRAIN_ROIS_PER_IMAGE, cfg.RPN_TRAIN_ANCHORS_PER_IMAGE = 16, 32
    return cfg


def _run(ds, cfg, n_batches, aug_seed, device_targets, seed=7, **kw):
    from caesar_mrcnn_amd.augment import ReferenceAugmenter
    from caesar_mrcnn_amd.datagen import data_generator
    np.random.seed(11)
    aug = ReferenceAugmenter(seed=aug_seed) if aug_seed is not None else None
    gen = data_generator(ds, cfg, shuffle=True, augmentation=aug, batch_size=2, seed=seed, device_targets=device_targets, **kw)
    return [next(gen)[0] for _ in range(n_batches)]


def _host_masks(batch, G):
    m = np.asarray(batch[6]) != 0
    if m.shape[-1] > G:                                    # device_targets rounds the host batch's planes up to 8
        assert not m[..., G:].any()
        m = m[..., :G]
    return np.pad(m, ((0, 0), (0, 0), (0, 0), (0, G - m.shape[-1]))).astype(np.uint8)


def _assert_same_batch(got, want, G):
    assert len(got) == 7 and torch.is_tensor(got[0]) and torch.is_tensor(got[6])
    assert got[0].dtype == torch.float32 and got[6].dtype == torch.uint8 and tuple(got[6].shape[-1:]) == (G,)
    ready = getattr(got, "ready", None)
    assert ready is not None
    ready.synchronize()
    assert torch.equal(got[0].cpu(), torch.from_numpy(want[0]))
    assert np.array_equal(got[6].cpu().numpy(), _host_masks(want, G))
    for g, w in zip(got[1:6], want[1:6]):
        assert (g is None and w is None) or (g.dtype == w.dtype and np.array_equal(g, w))


@pytest.mark.parametrize("aug_seed", [3, None])
@pytest.mark.parametrize("device_targets", [True, False])
def test_generator_equals_the_host_generator(dev, aug_seed, device_targets):
    from caesar_mrcnn_amd import gtprep
    cfg = _cfg()
    before = dict(gtprep.counters)
    want = _run(_Toy(small=5), cfg, 6, aug_seed, device_targets)
    ds = _Toy(small=5)
    got = _run(ds, cfg, 6, aug_seed, device_targets, device_samples=True, device=dev)
    for g, w in zip(got, want):
        _assert_same_batch(g, w, cfg.MAX_GT_INSTANCES)
    built = {k: gtprep.counters[k] - before[k] for k in before}
    assert built["device"] > 0 and built["host"] > 0 and built["device"] + built["host"] == 12       # image 5 is the host's
    assert {1, 3, 4, 5} <= set(ds.loads)
    if aug_seed is not None:                               # the warp emptied an instance somewhere: fewer ids than the image has
        lost = [b for w in want for b in range(2) if np.count_nonzero(w[4][b]) < min(cfg.MAX_GT_INSTANCES, ds._make(int(w[1][b, 0]))[2].size)]
        assert lost


def test_to_device_sees_the_same_step(dev, tmp_path):
    from caesar_mrcnn_amd.model import MaskRCNN
    cfg = _cfg()
    model = MaskRCNN("training", cfg, str(tmp_path / "logs"), device=dev, seed=0)
    for device_targets in (True, False):
        want = _run(_Toy(small=5), cfg, 3, 3, device_targets)
        got = _run(_Toy(small=5), cfg, 3, 3, device_targets, device_samples=True, device=dev)
        r = np.random.RandomState(0)
        for g, w in zip(got, want):
            keys = r.uniform(0, 1, (2, cfg.POST_NMS_ROIS_TRAINING))
            model.get_anchors((64, 64, 3))
            rpn_keys = r.uniform(0, 1, (2, model.anchors.shape[0])).astype(np.float32)
            a = model._to_device(w, keys, rpn_keys)
            b = model._to_device(g, keys, rpn_keys)
            assert model.last_mask_h2d_bytes == 0
            torch.cuda.synchronize()
            assert len(a) == len(b) == 8
            for x, y in zip(a, b):
                assert x.dtype == y.dtype and x.shape == y.shape and torch.equal(x, y)
            assert b[0].data_ptr() == g[0].data_ptr() and b[5].data_ptr() == g[6].data_ptr()       # taken as they are


def test_mini_mask_config_keeps_the_host_generator(dev, caplog):
    cfg = _cfg()
    cfg.USE_MINI_MASK = True
    cfg.MINI_MASK_SHAPE = (16, 16)
    want = _run(_Toy(), cfg, 2, 3, False)
    with caplog.at_level(logging.INFO, logger="mrcnn"):
        got = _run(_Toy(), cfg, 2, 3, False, device_samples=True, device=dev)
    said = [r.getMessage() for r in caplog.records if "device_samples" in r.getMessage()]
    assert len(said) == 1 and "USE_MINI_MASK" in said[0]
    for g, w in zip(got, want):
        assert type(g) is list
        for x, y in zip(g, w):
            assert isinstance(x, np.ndarray) and x.dtype == y.dtype and np.array_equal(x, y)


def test_four_prefetcher_workers(dev):
    """Worker k's generator is deterministic (its own shuffle seed, its own augmenter seed, device targets, no image above
    MAX_GT_INSTANCES: nothing draws from the shared global RNG), so the host generator with the same seeds walks the same image
    ids with the same plans.  All 12 batches are collected first, while the workers go on producing, and compared afterwards:
    a batch buffer rewritten after it was handed over would show."""
    from caesar_mrcnn_amd.augment import ReferenceAugmenter
    from caesar_mrcnn_amd.datagen import Prefetcher, data_generator
    cfg = _cfg()
    cfg.MAX_GT_INSTANCES = 12
    G = cfg.MAX_GT_INSTANCES

    def gens(**kw):
        return [data_generator(_Toy(small=5), cfg, shuffle=True, augmentation=ReferenceAugmenter(seed=20 + k), batch_size=2,
                               seed=100 + k, device_targets=True, **kw) for k in range(4)]
    expected = [[next(g)[0] for _ in range(12)] for g in gens()]
    pf = Prefetcher(gens(device_samples=True, device=dev), depth=4)
    try:
        got = [next(pf)[0] for _ in range(12)]
    finally:
        pf.close()
    torch.cuda.synchronize()
    nxt = [0, 0, 0, 0]                                     # each worker's batches arrive in its own order
    for g in got:
        for k in range(4):
            w = expected[k][nxt[k]]
            if np.array_equal(g[1], w[1]) and np.array_equal(g[4], w[4]) and np.array_equal(g[5], w[5]) and \
                    torch.equal(g[0].cpu(), torch.from_numpy(w[0])) and np.array_equal(g[6].cpu().numpy(), _host_masks(w, G)):
                nxt[k] += 1
                break
        else:
            raise AssertionError("a batch equals no worker's next host batch (image ids %r)" % (g[1][:, 0],))
    assert sum(nxt) == 12


def test_maskrcnn_train_builds_its_samples_on_the_device(dev, tmp_path):
    import bench
    from caesar_mrcnn_amd import gtprep
    from caesar_mrcnn_amd.augment import ReferenceAugmenter
    from caesar_mrcnn_amd.model import MaskRCNN
    cfg = _cfg()
    cfg.IMAGE_MIN_DIM = 64
    cfg.MAX_GT_INSTANCES = 20
    cfg.IMAGES_PER_GPU, cfg.STEPS_PER_EPOCH, cfg.VALIDATION_STEPS = 2, 2, 1
    cfg.DEVICE_SAMPLES = True
    ds = bench.synthetic_fits_dataset(cfg, 6, str(tmp_path / "data"), seed=3)
    model = MaskRCNN("training", cfg, str(tmp_path / "logs"), device=dev, seed=0)
    before = dict(gtprep.counters)
    model.train(ds, ds, learning_rate=cfg.LEARNING_RATE, epochs=1, layers="all", augmentation=ReferenceAugmenter(seed=0),
                n_worker_threads=2)
    assert gtprep.counters["device"] - before["device"] >= 2 * 3 and gtprep.counters["host"] == before["host"]
    assert len(model.history["loss"]) == 1 and np.isfinite(model.history["loss"][0]) and np.isfinite(model.history["val_loss"][0])


def test_cli_train_device_samples(dev, tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_cli_gpu as T
    d = str(tmp_path)
    lst = T._make_dataset(d)
    args = ["train", "--imgsize", "128", "--backbone", "custom", "--logs", os.path.join(d, "logs"), "--datalist", lst,
            "--train_rois_per_image", "32", "--rpn_train_anchors_per_image", "64", "--max_gt_instances", "10",
            "--nepochs", "1", "--epoch_length", "2", "--nvalidation_steps", "1", "--nimg_per_gpu", "2", "--reference_augmentation",
            "--device_samples"]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "run.py")] + args, cwd=d, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=280)
    out = r.stdout.decode()
    assert r.returncode == 0, out[-3000:]
    assert "Epoch 1/1" in out and "samples stay on the host" not in out
    ckpts = glob.glob(os.path.join(d, "logs", "rg-dataset*", "mask_rcnn_rg-dataset_0001.h5"))
    assert len(ckpts) == 1 and open(ckpts[0], "rb").read(4) == b"\x89HDF"
