"""The reference's training augmentation on the device (csrc/augment.hip through ops / augment.ReferenceAugmenter):
byte-identical to the float64 host statement augment.warp_host, through load_image_gt, from four loader threads at once,
inside MaskRCNN.train() and through `run.py train --reference_augmentation`."""
import glob
import os
import subprocess
import sys
import threading

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _A():
    from caesar_mrcnn_amd import augment
    return augment


def _u8_stages(H, W):
    return [None, ("fliplr",), ("flipud",), ("rotate", 90.0), ("rotate", -90.0), ("rotate", 37.3), ("rotate", -0.001),
            ("translate", 0.3, -0.3), ("translate", 0.5 / W, 0.0)]


@pytest.mark.parametrize("shape", [(256, 256, 3), (200, 312, 3), (129, 131, 1)])
def test_warp_u8_matches_host(dev, shape):
    from caesar_mrcnn_amd import ops
    A = _A()
    H, W, C = shape
    img = np.random.RandomState(H + W).randint(0, 256, shape).astype(np.uint8)
    src = torch.from_numpy(img).to(dev)
    for st in _u8_stages(H, W):
        m = np.array([[1.0, 0, 0], [0, 1.0, 0]]) if st is None else A.stage_matrix(st, H, W)
        got = ops.augment_warp_u8(src, m).cpu().numpy()
        assert np.array_equal(got, A.warp_host(img, m, "image")), st
    # 200 plans of the sampler, every stage checked against the host statement of the previous stage's output
    rng = np.random.RandomState(11)
    out = torch.empty_like(src)
    for _ in range(200):
        cur, cur_d = img, src
        for m in A.ReferenceAugmenter.matrices(A.ReferenceAugmenter.draw(rng), H, W):
            ops.augment_warp_u8(cur_d, m, out=out)
            cur = A.warp_host(cur, m, "image")
            assert np.array_equal(out.cpu().numpy(), cur)
            cur_d = out.clone()
    torch.cuda.synchronize()


@pytest.mark.parametrize("N", [1, 7, 8, 9, 31, 32, 33, 300])
def test_warp_mask_bits_matches_host(dev, N):
    from caesar_mrcnn_amd import ops
    A = _A()
    H, W = 96, 80
    rng = np.random.RandomState(N)
    mk = rng.rand(H, W, N) > 0.8
    mk[38:43, 27:34, N - 1] = False                        # the last instance: a one-pixel spot, so that the 0.5-pixel
    mk[40, 30, N - 1] = True                               # shifts below make exact 0.5 ties
    packed = np.packbits(mk, axis=-1, bitorder="little")
    nb = packed.shape[-1]
    stages = [("fliplr",), ("flipud",), ("rotate", 90.0), ("rotate", -37.3), ("translate", 0.3, -0.3),
              ("translate", 0.5 / W, 0.0), ("translate", 0.0, 0.5 / H)]
    stages += A.ReferenceAugmenter.draw(np.random.RandomState(3)) + [("rotate", 12.5)]
    for st in stages:
        m = A.stage_matrix(st, H, W)
        want = A.warp_host(mk, m, "mask")
        for pad in sorted({0, -nb % 4}):                   # the byte path (any nbytes) and the 32-bit word path
            p = np.concatenate([packed, np.zeros((H, W, pad), np.uint8)], axis=2) if pad else packed
            got = ops.augment_warp_mask_bits(torch.from_numpy(p).to(dev), m).cpu().numpy()
            assert not np.any(got[:, :, nb:])
            assert np.array_equal(np.unpackbits(got, axis=-1, count=N, bitorder="little").view(bool), want), (st, pad)
    m = A.stage_matrix(("translate", 0.5 / W, 0.0), H, W)
    assert not A.warp_host(mk[..., N - 1:], m, "mask")[40, 30:32].any()      # the tie itself: both neighbours unset


class _Toy(object):
    """Duck-typed like mrcnn.utils.Dataset as load_image_gt uses it: 256 x 256 uint8 images with 1..12 box instances."""

    def __init__(self, n=6, size=256):
        self.image_ids = np.arange(n)
        self.image_info = [{"source": "toy", "id": i} for i in range(n)]
        self.num_classes = 4
        self.source_class_ids = {"toy": [0, 1, 2, 3]}
        self.size = size

    def _make(self, i):
        r = np.random.RandomState(200 + i)
        img = r.randint(0, 40, (self.size, self.size, 3)).astype(np.uint8)
        k = r.randint(1, 13)
        mask = np.zeros((self.size, self.size, k), bool)
        for g in range(k):
            y, x = r.randint(0, self.size - 30, 2)
            h, w = r.randint(3, 30, 2)
            mask[y:y + h, x:x + w, g] = True
            img[y:y + h, x:x + w] = r.randint(100, 256)
        return img, mask, r.randint(1, 4, k).astype(np.int32)

    def load_image(self, i):
        return self._make(i)[0]

    def load_mask(self, i):
        return self._make(i)[1], self._make(i)[2]


def _cfg(size=256):
    from caesar_mrcnn_amd.config import run_py_config
    cfg = run_py_config(backbone="custom", imgsize=size)
    cfg.MAX_GT_INSTANCES = 20
    return cfg


def test_apply_device_equals_host_through_load_image_gt(dev):
    from caesar_mrcnn_amd.datagen import load_image_gt
    A = _A()
    ds, cfg = _Toy(), _cfg()
    dev_aug, host_aug = A.ReferenceAugmenter(device=dev), A.ReferenceAugmenter()
    rng = np.random.RandomState(5)
    plans = [[("translate", -0.3, 0.25), ("rotate", 61.0)], [("rotate", -90.0)], []] + \
            [A.ReferenceAugmenter.draw(rng) for _ in range(12)]
    for k, plan in enumerate(plans):
        i = k % len(ds.image_ids)
        got = load_image_gt(ds, cfg, i, augmentation=lambda im, mk: dev_aug.apply(im, mk, plan))
        want = load_image_gt(ds, cfg, i, augmentation=lambda im, mk: host_aug.apply(im, mk, plan, device=None))
        for g, w in zip(got, want):
            assert g.dtype == w.dtype and np.array_equal(g, w), plan
    assert dev_aug.device_calls == sum(1 for p in plans if p) and host_aug.device_calls == 0
    # no instances: only the image is warped
    img = ds.load_image(0)
    gi, gm = dev_aug.apply(img, np.zeros((256, 256, 0), bool), [("rotate", 20.0)])
    assert gm.shape == (256, 256, 0) and np.array_equal(gi, A.warp_host(img, A.stage_matrix(("rotate", 20.0), 256, 256)))


def test_four_loader_threads_share_one_augmenter(dev):
    A = _A()
    ds = _Toy()
    aug = A.ReferenceAugmenter(seed=1, device=dev)
    host = A.ReferenceAugmenter()
    errors, done = [], []

    def worker(t):
        try:
            for j in range(8):
                i = (t + j) % len(ds.image_ids)
                img, mk = ds.load_image(i), ds.load_mask(i)[0]
                with aug._lock:                     # the plan __call__ would draw, drawn the same way
                    plan = aug.draw(aug._rng)
                gi, gm = aug.apply(img, mk, plan)
                wi, wm = host.apply(img, mk, plan)
                if not (np.array_equal(gi, wi) and np.array_equal(gm, wm)):
                    errors.append((t, j, plan))
                gi, gm = aug(img, mk)                # and the callable itself, concurrently
                if gi.shape != img.shape or gm.shape != mk.shape:
                    errors.append((t, j, "shape"))
                done.append(1)
        except Exception as e:                       # surfaced below
            errors.append(repr(e))
    threads = [threading.Thread(target=worker, args=(t,)) for t in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=120)
    assert not any(t.is_alive() for t in threads)
    assert not errors, errors[:3]
    assert len(done) == 32 and aug.device_calls > 0


def test_maskrcnn_train_runs_the_device_augmenter(dev, tmp_path):
    import bench
    from caesar_mrcnn_amd.model import MaskRCNN
    A = _A()
    cfg = _cfg(128)
    cfg.TRAIN_ROIS_PER_IMAGE, cfg.RPN_TRAIN_ANCHORS_PER_IMAGE = 32, 64
    cfg.IMAGES_PER_GPU, cfg.STEPS_PER_EPOCH, cfg.VALIDATION_STEPS = 2, 2, 1
    ds = bench.synthetic_fits_dataset(cfg, 6, str(tmp_path / "data"), seed=3)
    model = MaskRCNN("training", cfg, str(tmp_path / "logs"), device=dev, seed=0)
    aug = A.ReferenceAugmenter(seed=0)
    model.train(ds, ds, learning_rate=cfg.LEARNING_RATE, epochs=1, layers="all", augmentation=aug, n_worker_threads=2)
    assert aug.device is not None and torch.device(aug.device) == torch.device(model.engine.dev)
    assert aug.device_calls > 0
    assert len(model.history["loss"]) == 1 and np.isfinite(model.history["loss"][0]) and np.isfinite(model.history["val_loss"][0])


def test_cli_train_reference_augmentation(dev, tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_cli_gpu as T
    d = str(tmp_path)
    lst = T._make_dataset(d)
    args = ["train", "--imgsize", "128", "--backbone", "custom", "--logs", os.path.join(d, "logs"), "--datalist", lst,
            "--train_rois_per_image", "32", "--rpn_train_anchors_per_image", "64", "--max_gt_instances", "10",
            "--nepochs", "1", "--epoch_length", "2", "--nvalidation_steps", "1", "--nimg_per_gpu", "2", "--reference_augmentation"]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "run.py")] + args, cwd=d, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=280)
    out = r.stdout.decode()
    assert r.returncode == 0, out[-3000:]
    assert "Epoch 1/1" in out
    ckpts = glob.glob(os.path.join(d, "logs", "rg-dataset*", "mask_rcnn_rg-dataset_0001.h5"))
    assert len(ckpts) == 1 and open(ckpts[0], "rb").read(4) == b"\x89HDF"
