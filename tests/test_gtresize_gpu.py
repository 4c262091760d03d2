"""Scaled training samples on the device (csrc/gtprep.hip: mrcnn_mask_bits_zoom, csrc/mold.hip:
mrcnn_resize_image_u8, through ops / gtprep.DeviceSampler(resize=True) / data_generator(device_resize=True)): the two kernels
against their host statements, byte for byte; the generator against the host generator, item by item; MaskRCNN.train()."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SENTINEL = 0xAB
ZOOMS = [(32, 32, 1.5), (28, 30, 0.5), (90, 60, 64 / 90), (1, 7, 3.0), (29, 61, 1.5), (255, 40, 1.37), (64, 130, 0.5), (7, 5, 9.0)]
COUNTS = [1, 32, 33, 70]                                   # nb = 4, 4, 8, 12


def _canvases(oh, ow):
    """(top, left, OH, OW): canvas widths 48, 64 and 65 where the window fits (rows that are no multiple of 64 pixels), the
    window alone, and one wider than the window on both sides."""
    out = [(0, 0, oh, ow), (2, 3, oh + 5, ow + 4)]
    for k, OW in enumerate((48, 64, 65)):
        if ow <= OW:
            out.append((k, (OW - ow) // 2, oh + 2 * k, OW))
    return out


@pytest.mark.parametrize("zoom", ZOOMS)
def test_mask_zoom_equals_the_host_statement(dev, zoom):
    from caesar_mrcnn_amd import gtprep, ops, utils
    h, w, scale = zoom
    iy, ix = gtprep.zoom_index_tables(h, w, scale)
    oh, ow = iy.size, ix.size
    iy_d, ix_d = torch.from_numpy(iy).to(dev), torch.from_numpy(ix).to(dev)
    for n in COUNTS:
        r = np.random.RandomState(h + 100 * n)
        mask = r.rand(h, w, n) > 0.5
        bits = np.unpackbits(gtprep.mask_bits_pack(mask), axis=-1, bitorder="little")
        bits[:, :, n:] = r.randint(0, 2, bits[:, :, n:].shape)             # whole words move: the padding bits with them
        packed = np.packbits(bits, axis=-1, bitorder="little")
        packed_d = torch.from_numpy(packed).to(dev)
        nb = packed.shape[2]
        for top, left, OH, OW in _canvases(oh, ow):
            want = gtprep.mask_bits_zoom_host(packed, iy, ix, top, left, OH, OW)
            batch = torch.full((3, OH, OW, nb), SENTINEL, dtype=torch.uint8, device=dev)
            out = ops.mask_bits_zoom(packed_d, iy, ix, (top, left), (OH, OW), out=batch[1])
            assert out.data_ptr() == batch[1].data_ptr()
            got = batch.cpu().numpy()
            assert np.all(got[0] == SENTINEL) and np.all(got[2] == SENTINEL), (zoom, n, OH, OW)
            assert np.array_equal(got[1], want), (zoom, n, top, left, OH, OW)
            # and against the reference's own statement on the unpacked planes
            planes = np.unpackbits(got[1], axis=-1, bitorder="little")[:, :, :n].astype(bool)
            pad = [(top, OH - oh - top), (left, OW - ow - left), (0, 0)]
            assert np.array_equal(planes, utils.resize_mask(mask, scale, pad)), (zoom, n, top, left, OH, OW)
        fresh = ops.mask_bits_zoom(packed_d, iy_d, ix_d, (1, 0), (oh + 1, ow + 2))           # device tables, no out: allocated here
        assert fresh.dtype == torch.uint8 and tuple(fresh.shape) == (oh + 1, ow + 2, nb)
        assert np.array_equal(fresh.cpu().numpy(), gtprep.mask_bits_zoom_host(packed, iy, ix, 1, 0, oh + 1, ow + 2))


def test_mask_zoom_reads_entries_outside_the_source_as_the_constant(dev):
    """Device tables are not checked on the host: whatever they hold, nothing outside the source is read."""
    from caesar_mrcnn_amd import gtprep, ops
    packed = gtprep.mask_bits_pack(np.ones((4, 5, 33), bool))
    iy = np.array([0, -1, 3, 4, 2 ** 31 - 1, -2 ** 31], np.int32)
    ix = np.array([4, 5, -1, 0, -7], np.int32)
    got = ops.mask_bits_zoom(torch.from_numpy(packed).to(dev), torch.from_numpy(iy).to(dev), torch.from_numpy(ix).to(dev), (0, 0), (6, 5))
    want = np.zeros((6, 5, 8), np.uint8)
    want[np.ix_([0, 2], [0, 3])] = packed[0, 0]
    assert np.array_equal(got.cpu().numpy(), want)


IMAGES = [(32, 32, 3), (20, 50, 3), (90, 60, 3), (32, 32, 1), (90, 60, 1), (20, 50, 4), (255, 40, 4), (56, 60, 3), (64, 64, 3)]


@pytest.mark.parametrize("shape", IMAGES)
def test_image_resize_equals_resize_image(dev, shape):
    """IMAGE_MIN_DIM 48, IMAGE_MAX_DIM 64: 32 x 32 and 20 x 50 are scaled up, 90 x 60 and 255 x 40 down, 56 x 60 is padded only,
    64 x 64 copied; a constant image has min = max, so the clip decides every value of its (border-darkened) interpolation."""
    from caesar_mrcnn_amd import ops, utils
    h, w, C = shape
    r = np.random.RandomState(h * w + C)
    noise = r.randint(0, 256, shape).astype(np.uint8)
    narrow = r.randint(100, 140, shape).astype(np.uint8)
    for img in (noise, narrow, np.full(shape, 77, np.uint8), np.zeros(shape, np.uint8), np.full(shape, 255, np.uint8)):
        want, window, scale, padding, _ = utils.resize_image(img, min_dim=48, max_dim=64, mode="square")
        plan = utils.resize_plan(shape, min_dim=48, max_dim=64, mode="square")
        assert plan[0] == scale and tuple(plan[3]) == tuple(window) and want.dtype == np.uint8 and want.shape == (64, 64, C)
        (oh, ow), (top, left) = plan[1], (padding[0][0], padding[1][0])
        batch = torch.full((3, 64, 64, C), SENTINEL, dtype=torch.uint8, device=dev)
        out = ops.resize_image_u8(torch.from_numpy(img).to(dev), (oh, ow), (top, left), (64, 64), out=batch[1])
        assert out.data_ptr() == batch[1].data_ptr()
        got = batch.cpu().numpy()
        assert np.all(got[0] == SENTINEL) and np.all(got[2] == SENTINEL)
        assert np.array_equal(got[1], want), (shape, scale, int(np.abs(got[1].astype(int) - want).max()))
    # padding on one side only, a canvas that is no square, no out: allocated here
    oh, ow = round(h * 1.3), round(w * 0.8)
    want = np.pad(utils.resize(noise, (oh, ow), preserve_range=True), [(0, 3), (5, 0), (0, 0)]).astype(np.uint8)
    fresh = ops.resize_image_u8(torch.from_numpy(noise).to(dev), (oh, ow), (0, 5), (oh + 3, ow + 5))
    assert fresh.dtype == torch.uint8 and np.array_equal(fresh.cpu().numpy(), want)


def test_wrappers_refuse_and_leave_the_output_alone(dev):
    from caesar_mrcnn_amd import ops
    good = torch.zeros((4, 4, 4), dtype=torch.uint8, device=dev)
    out = torch.full((8, 8, 4), SENTINEL, dtype=torch.uint8, device=dev)
    t6 = np.zeros(6, np.int32)
    for bad in (good.to(torch.int32), good[0], good[:, :, :3].contiguous(), good.cpu()):
        with pytest.raises((ValueError, ops._hip.HipPathError)):
            ops.mask_bits_zoom(bad, t6, t6, (1, 1), (8, 8), out=out)
    for t in ([4] * 6, [-2] * 6, [], torch.zeros(6, dtype=torch.int32), torch.zeros(6, dtype=torch.int64, device=dev)):
        with pytest.raises(ValueError):
            ops.mask_bits_zoom(good, t, t6, (1, 1), (8, 8), out=out)
        with pytest.raises(ValueError):
            ops.mask_bits_zoom(good, t6, t, (1, 1), (8, 8), out=out)
    for pad_tl in ((3, 1), (1, 3), (-1, 0)):
        with pytest.raises(ValueError):
            ops.mask_bits_zoom(good, t6, t6, pad_tl, (8, 8), out=out)
    with pytest.raises(ValueError):
        ops.mask_bits_zoom(good, t6, t6, (1, 1), (8, 8), out=out[:, :, :2])
    with pytest.raises(ValueError):
        ops.mask_bits_zoom(good, t6, t6, (1, 1), (8, 8), out=out.cpu())
    wide_out = torch.full((6, ops.GTPREP_MAX_SIDE + 1, 4), SENTINEL, dtype=torch.uint8, device=dev)
    with pytest.raises(ops.GtPrepUnsupported):
        ops.mask_bits_zoom(good, t6, t6, (0, 0), (6, ops.GTPREP_MAX_SIDE + 1), out=wide_out)
    img = torch.zeros((4, 4, 3), dtype=torch.uint8, device=dev)
    out_i = torch.full((8, 8, 3), SENTINEL, dtype=torch.uint8, device=dev)
    for bad in (img.to(torch.float32), img[0], img.permute(1, 0, 2)[:, :2], torch.zeros((4, 4, 5), dtype=torch.uint8, device=dev)):
        with pytest.raises(ValueError):
            ops.resize_image_u8(bad, (6, 6), (1, 1), (8, 8), out=out_i)
    for out_hw, pad_tl in (((0, 6), (1, 1)), ((6, 6), (3, 1)), ((6, 6), (1, -1)), ((6, 9), (0, 0))):
        with pytest.raises(ValueError):
            ops.resize_image_u8(img, out_hw, pad_tl, (8, 8), out=out_i)
    for bad_out in (out_i[:, :, :2], out_i.to(torch.float32), out_i.cpu(), torch.zeros((8, 9, 3), dtype=torch.uint8, device=dev)):
        with pytest.raises(ValueError):
            ops.resize_image_u8(img, (6, 6), (1, 1), (8, 8), out=bad_out)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((wide_out == SENTINEL).all()) and bool((out_i == SENTINEL).all())


# ---- the generator -------------------------------------------------------------------------------------------------
SIZES = {0: (90, 60), 1: (56, 60), 5: (32, 32), 6: (20, 50), 7: (32, 32), 8: (70, 64)}      # every other image: 64 x 64
SCALED = {0, 5, 6, 7, 8}


class _Toy(object):
    """Duck-typed like mrcnn.utils.Dataset as load_image_gt uses it (the pattern of test_gtprep_gpu._Toy) at IMAGE_MIN_DIM 48,
    IMAGE_MAX_DIM 64: images 5 and 7 (32 x 32) and 6 (20 x 50) are scaled up, 0 (90 x 60) and 8 (70 x 64) down, 1 (56 x 60) is
    padded only; image 2 has no instance, image 3 has 9 (above the lowered MAX_GT_INSTANCES), image 4 carries uint8 0 / 1 masks;
    every image has a two-pixel instance in a corner, which most rotations and shifts (and a down-scaling) empty."""

    def __init__(self, n=9):
        self.image_ids = np.arange(n)
        self.image_info = [{"source": "toy", "id": i} for i in range(n)]
        self.num_classes = 4
        self.source_class_ids = {"toy": [0, 1, 2, 3]}
        self.loads = []

    def _make(self, i):
        r = np.random.RandomState(500 + i)
        h, w = SIZES.get(int(i), (64, 64))
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
    cfg.IMAGE_MIN_DIM, cfg.IMAGE_MAX_DIM = 48, 64
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


N_BATCHES = 8                                              # 16 samples: every image of the toy set at least once


def _scaled_samples(batches):
    """How many samples of the host generator's batches are scaled images, and the image ids (image_meta[0]) it walked.  (The
    scale itself, image_meta[11], is truncated where a batch's first image has an integer meta row, as in the reference.)"""
    ids = [int(b[1][k, 0]) for b in batches for k in range(2)]
    return sum(i in SCALED for i in ids), set(ids)


@pytest.fixture(scope="module")
def host_batches():
    """The host generator's batches per (aug_seed, device_targets), computed once and never written."""
    cache = {}

    def get(aug_seed, device_targets):
        key = (aug_seed, device_targets)
        if key not in cache:
            cache[key] = _run(_Toy(), _cfg(), N_BATCHES, aug_seed, device_targets)
        return cache[key]
    return get


@pytest.mark.parametrize("aug_seed", [3, None])
@pytest.mark.parametrize("device_targets", [True, False])
def test_generator_scales_on_the_device_and_equals_the_host_generator(dev, host_batches, aug_seed, device_targets):
    from caesar_mrcnn_amd import gtprep
    cfg = _cfg()
    want = host_batches(aug_seed, device_targets)
    n_scaled, seen = _scaled_samples(want)
    assert n_scaled > 0 and {0, 5, 6} <= seen             # 90 x 60, 32 x 32 and 20 x 50 are among the samples
    before = dict(gtprep.counters)
    ds = _Toy()
    got = _run(ds, cfg, N_BATCHES, aug_seed, device_targets, device_samples=True, device_resize=True, device=dev)
    for g, w in zip(got, want):
        _assert_same_batch(g, w, cfg.MAX_GT_INSTANCES)
        assert np.array_equal(g[1][:, 7:12], w[1][:, 7:12])                # window and the true scale, named
    built = {k: gtprep.counters[k] - before[k] for k in before}
    assert built["host"] == 0 and built["device"] == 2 * N_BATCHES and built["scaled"] == n_scaled > 0, built


@pytest.mark.parametrize("aug_seed", [3, None])
def test_without_the_switch_scaled_images_are_the_hosts(dev, host_batches, aug_seed):
    from caesar_mrcnn_amd import gtprep
    cfg = _cfg()
    want = host_batches(aug_seed, True)
    n_scaled, _ = _scaled_samples(want)
    before = dict(gtprep.counters)
    got = _run(_Toy(), cfg, N_BATCHES, aug_seed, True, device_samples=True, device=dev)
    for g, w in zip(got, want):
        _assert_same_batch(g, w, cfg.MAX_GT_INSTANCES)
    built = {k: gtprep.counters[k] - before[k] for k in before}
    assert built["scaled"] == 0 and built["host"] == n_scaled and built["device"] == 2 * N_BATCHES - n_scaled, built


def test_the_sampler_caches_its_tables_on_the_host_and_on_the_device(dev):
    from caesar_mrcnn_amd import gtprep
    cfg = _cfg()
    ds = _Toy()
    sampler = gtprep.DeviceSampler(cfg, dev, resize=True)
    kind, s5 = sampler.load(ds, 5, None)
    assert kind == "device" and s5.scaled and s5.shape == (64, 64, 3) and len(sampler._zoom) == 1
    assert s5.image_meta[1:12].tolist() == [32, 32, 3, 64, 64, 3, 8, 8, 56, 56, 1.5]          # the true window and scale
    entry = sampler._zoom[(32, 32, 1.5)]
    assert torch.is_tensor(entry[2]) and entry[2].device.type == "cuda" and np.array_equal(entry[2].cpu().numpy(), entry[0])
    assert np.array_equal(entry[3].cpu().numpy(), entry[1])
    kind, s7 = sampler.load(ds, 7, None)                   # the same size again: the same tables
    assert kind == "device" and len(sampler._zoom) == 1 and sampler._zoom[(32, 32, 1.5)] is entry
    kind, s1 = sampler.load(ds, 1, None)                   # scale 1: no table
    assert kind == "device" and not s1.scaled and len(sampler._zoom) == 1


def test_maskrcnn_train_scales_its_samples_on_the_device(dev, tmp_path):
    """Two steps of MaskRCNN.train() on the toy set, one loader thread, targets and keys drawn on the device / in the main thread
    from seeds set here (no loader thread draws from a global generator: MAX_GT_INSTANCES covers every image): history["loss"]
    with both switches on equals that of the host loader bit for bit.  Learning rate 0: the comparison is about what the loader
    feeds, and the second step must not depend on the backward pass, whose float atomics are not ordered -- measured with the
    host loader alone, twice from the same seeds at the default rate: loss 32.58167365193367 both times, val_loss (after two
    updates) 19.6918762922287 against 19.691876769065857.  val_loss is therefore only required to be finite."""
    from caesar_mrcnn_amd import gtprep
    from caesar_mrcnn_amd.augment import ReferenceAugmenter
    from caesar_mrcnn_amd.model import MaskRCNN

    def run(tag, **switches):
        cfg = _cfg()
        cfg.MAX_GT_INSTANCES = 12
        cfg.IMAGES_PER_GPU, cfg.STEPS_PER_EPOCH, cfg.VALIDATION_STEPS = 2, 2, 1
        cfg.DEVICE_RPN_TARGETS = True
        for k, v in switches.items():
            setattr(cfg, k, v)
        np.random.seed(21)
        torch.manual_seed(21)
        model = MaskRCNN("training", cfg, str(tmp_path / tag), device=dev, seed=0)
        before = dict(gtprep.counters)
        model.train(_Toy(), _Toy(), learning_rate=0.0, epochs=1, layers="all", augmentation=ReferenceAugmenter(seed=0),
                    n_worker_threads=1)
        torch.cuda.synchronize()
        return model.history, {k: gtprep.counters[k] - before[k] for k in before}
    want, built = run("host")
    assert built == {"device": 0, "host": 0, "scaled": 0}
    got, built = run("device", DEVICE_SAMPLES=True, DEVICE_SAMPLE_RESIZE=True)
    assert built["scaled"] > 0 and built["host"] == 0 and built["device"] >= 2 * 3, built
    print("history: host %r device %r" % (want, got))
    assert len(got["loss"]) == 1 and np.isfinite(got["loss"][0]) and np.isfinite(got["val_loss"][0])
    assert got["loss"] == want["loss"]
