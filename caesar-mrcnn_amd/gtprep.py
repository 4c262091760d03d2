"""Training samples assembled on the GPU, instance masks kept bit-packed.

Per training image load_image_gt + data_generator (mrcnn/model.py:1277-1377, 1721-1904) reduce the [H, W, N] instance masks
twice on the host -- np.sum(mask, axis=(0, 1)) picks the instances that kept a pixel, utils.extract_bboxes loops over them
-- and copy the kept planes into the zeroed [H, W, MAX_GT_INSTANCES] batch.  This module states both on the loader's
bit-packed layout (`mask_bits_stats_host`, `mask_bits_gather_host`: the answers csrc/gtprep.hip is held to) and builds a
sample with them on the device (`DeviceSampler`): the pixels go up once and never come back, only the [N, 5] table of counts
and boxes does.  An image resize_image scales is scaled there too when asked for: utils.resize_mask's
nearest-neighbour zoom as two index tables taken from scipy itself (`zoom_index_tables`) and its statement on the packed
layout (`mask_bits_zoom_host`), the image by ops.resize_image_u8.

Layout: packed [H, W, nb] uint8 = np.packbits(mask != 0, axis=-1, bitorder="little"), padded with zero bytes to nb % 4 == 0
(`mask_bits_pack`); instance j is bit j & 7 of byte j >> 3.  It is what ops.augment_warp_mask_bits reads and writes.
"""
import threading

import numpy as np

from . import utils

# samples data_generator(device_samples=True) built on the device / handed to the host path one by one (a scale other than 1
# without device_resize, ...); "scaled": those of "device" that were scaled there (device_resize=True)
counters = {"device": 0, "host": 0, "scaled": 0}
ZOOM_CACHE_ENTRIES = 256          # (h, w, scale) keys a DeviceSampler keeps index tables for; the oldest goes first
_counters_lock = threading.Lock()


def _count(kind):
    with _counters_lock:
        counters[kind] += 1


def mask_bits_pack(mask):
    """[H, W, N] masks (bool, or any dtype: != 0) -> packed [H, W, nb] uint8, nb = 4 ceil(N / 32) (at least 4)."""
    mask = np.asarray(mask)
    bits = mask if mask.dtype == np.bool_ else mask != 0
    packed = np.packbits(bits, axis=-1, bitorder="little")
    nb = max(4, -(-packed.shape[2] // 4) * 4)
    if nb != packed.shape[2]:
        packed = np.concatenate([packed, np.zeros(packed.shape[:2] + (nb - packed.shape[2],), np.uint8)], axis=2)
    return np.ascontiguousarray(packed)


def mask_bits_stats_host(packed, n):
    """(count [n] int32, box [n, 4] int32) of the first n instances of packed masks: count = np.sum(mask, axis=(0, 1)), box =
    utils.extract_bboxes(mask) -- (y1, x1, y2 + 1, x2 + 1), zeros for an instance without a pixel.  Bits >= n are ignored."""
    packed = np.asarray(packed)
    if packed.dtype != np.uint8 or packed.ndim != 3 or not 1 <= n <= 8 * packed.shape[2]:
        raise ValueError("packed must be uint8 [H, W, nb] with 1 <= n <= 8 nb")
    H, W = packed.shape[:2]
    bits = np.unpackbits(packed, axis=-1, count=int(n), bitorder="little").view(bool)
    count = bits.sum(axis=(0, 1), dtype=np.int64).astype(np.int32)
    rows, cols = bits.any(axis=1), bits.any(axis=0)                        # [H, n], [W, n]
    box = np.stack([rows.argmax(axis=0), cols.argmax(axis=0), H - rows[::-1].argmax(axis=0), W - cols[::-1].argmax(axis=0)], axis=1)
    box[count == 0] = 0
    return count, box.astype(np.int32)


def mask_bits_gather_host(packed, sel, G):
    """uint8 [H, W, G]: plane j = instance sel[j] of the packed masks (0 / 1) for j < len(sel), zeros from there on --
    np.pad(mask[:, :, sel], ((0, 0), (0, 0), (0, G - len(sel))))."""
    packed = np.asarray(packed)
    sel = np.asarray(sel, dtype=np.int64).reshape(-1)
    if packed.dtype != np.uint8 or packed.ndim != 3 or sel.size > G:
        raise ValueError("packed must be uint8 [H, W, nb] and len(sel) <= G")
    if sel.size and (sel.min() < 0 or sel.max() >= 8 * packed.shape[2]):
        raise ValueError("sel must lie in [0, 8 nb)")
    out = np.zeros(packed.shape[:2] + (int(G),), np.uint8)
    out[:, :, :sel.size] = np.unpackbits(packed, axis=-1, bitorder="little")[:, :, sel]
    return out


def zoom_index_tables(h, w, scale):
    """(iy [oh] int32, ix [ow] int32): the input row / column scipy.ndimage.zoom(mask, [scale, scale, 1], order=0) copies into
    every output row / column of an [h, w, N] mask, -1 where it writes its constant 0 instead (the last coordinate can land a
    hair past n - 1).  The zoom is separable and its choice on an axis depends on that axis alone, so the tables are scipy's own
    answers on the two 1-D ramps 1 .. n -- its coordinate arithmetic is not restated here."""
    import warnings
    import scipy.ndimage
    tables = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for n in (int(h), int(w)):
            tables.append((scipy.ndimage.zoom(np.arange(1, n + 1), scale, order=0) - 1).astype(np.int32))
    return tables[0], tables[1]


def mask_bits_zoom_host(packed, iy, ix, top, left, OH, OW):
    """uint8 [OH, OW, nb]: pixel (top + y, left + x) = packed pixel (iy[y], ix[x]), zeros where a table entry is -1 and outside
    the len(iy) x len(ix) window -- utils.resize_mask (zoom by the tables of zoom_index_tables, then np.pad) on packed masks."""
    packed = np.asarray(packed)
    iy, ix = np.asarray(iy, dtype=np.int64).reshape(-1), np.asarray(ix, dtype=np.int64).reshape(-1)
    if packed.dtype != np.uint8 or packed.ndim != 3 or min(packed.shape) < 1 or not iy.size or not ix.size:
        raise ValueError("packed must be a non-empty uint8 [h, w, nb] and the tables non-empty")
    h, w, nb = packed.shape
    if iy.min() < -1 or iy.max() >= h or ix.min() < -1 or ix.max() >= w:
        raise ValueError("the tables must lie in [-1, h) and [-1, w)")
    if top < 0 or left < 0 or top + iy.size > OH or left + ix.size > OW:
        raise ValueError("the zoomed window does not fit the canvas")
    padded = np.zeros((h + 1, w + 1, nb), np.uint8)                         # row / column -1: the constant
    padded[:h, :w] = packed
    out = np.zeros((int(OH), int(OW), nb), np.uint8)
    out[top:top + iy.size, left:left + ix.size] = padded[iy][:, ix]
    return out


def generator_refusal(config, device, augment, augmentation):
    """Why a whole generator keeps the host path although device samples were asked for (None: it need not)."""
    from .augment import ReferenceAugmenter
    if device is None:
        return "no GPU device was given"
    try:
        import torch
        if torch.device(device).type != "cuda" or not torch.cuda.is_available():
            return "no GPU (%s)" % (device,)
    except Exception as e:                                   # torch missing or a malformed device
        return "no GPU (%s)" % (e,)
    if config.USE_MINI_MASK:
        return "USE_MINI_MASK resizes every instance on the host"
    if config.IMAGE_RESIZE_MODE == "crop":
        return "IMAGE_RESIZE_MODE 'crop' draws its window on the host"
    if augment:
        return "the deprecated augment=True flips on the host"
    if augmentation is not None and not isinstance(augmentation, ReferenceAugmenter):
        return "the augmentation is not a ReferenceAugmenter"
    return None


class DeviceSample(object):
    """One image's ground truth after DeviceSampler.load: the padded, augmented uint8 image and the bit-packed masks on the
    device, the kept instances' class ids / boxes / bit indices and image_meta on the host."""
    __slots__ = ("img", "bits", "shape", "sel", "class_ids", "bbox", "image_meta", "scaled")


class DeviceSampler(object):
    """Builds training samples on `device`, on the loader threads' one side stream under its lock (loader_stream.py)."""

    def __init__(self, config, device, resize=False):
        """resize: an image resize_image scales is scaled on the device too (Config.DEVICE_SAMPLE_RESIZE);
        without it such a sample is the host's."""
        import collections
        import torch
        self.config = config
        self.device = torch.device(device)
        self.resize = bool(resize)
        self._zoom = collections.OrderedDict()        # (h, w, scale) -> [iy, ix, iy on the device, ix on the device]

    def zoom_tables(self, h, w, scale):
        """The cache entry of zoom_index_tables(h, w, scale): datasets repeat their sizes.  At most ZOOM_CACHE_ENTRIES are kept."""
        key = (int(h), int(w), float(scale))
        entry = self._zoom.get(key)
        if entry is None:
            iy, ix = zoom_index_tables(h, w, scale)
            entry = self._zoom[key] = [iy, ix, None, None]
            while len(self._zoom) > ZOOM_CACHE_ENTRIES:
                self._zoom.popitem(last=False)
        return entry

    def load(self, dataset, image_id, augmentation):
        """("device", DeviceSample) -- or ("host", image, mask, class_ids), the loaded arrays of a sample that only the host
        path takes (a scale other than 1 unless `resize`, an image that is not uint8 [h, w, C <= 4], masks that are not bool /
        0-1 uint8 [h, w, N >= 1], sizes past a cap of the kernels).  That decision is taken before the augmentation plan is
        drawn."""
        import torch
        from . import ops
        from .loader_stream import loader_stream
        cfg, dev = self.config, self.device
        if getattr(dataset, "device", None) is not None and hasattr(dataset, "zscale_contrasts"):     # SourceDataset, DEVICE_FITS
            image = dataset.load_image(image_id, device_out=True)
        else:
            image = dataset.load_image(image_id)
        mask, class_ids = dataset.load_mask(image_id)
        on_dev = torch.is_tensor(image)

        def host():
            return "host", (image.cpu().numpy() if on_dev else image), mask, class_ids
        shape = tuple(image.shape)
        if len(shape) != 3 or not 1 <= shape[2] <= 4 or image.dtype != (torch.uint8 if on_dev else np.uint8) or min(shape) < 1:
            return host()
        if not isinstance(mask, np.ndarray) or mask.ndim != 3 or mask.shape[:2] != shape[:2] or mask.shape[2] < 1:
            return host()
        if mask.dtype != np.bool_ and not (mask.dtype == np.uint8 and mask.max() <= 1):
            return host()                       # (values above 1 interpolate differently in the host warp than their bits do)
        h, w, C = shape
        N = mask.shape[2]
        scale, (oh, ow), padding, window = utils.resize_plan(shape, min_dim=cfg.IMAGE_MIN_DIM, max_dim=cfg.IMAGE_MAX_DIM,
                                                             min_scale=cfg.IMAGE_MIN_SCALE, mode=cfg.IMAGE_RESIZE_MODE)
        scaled = scale != 1
        if scaled and not self.resize:
            return host()
        (top, bottom), (left, right) = padding[0], padding[1]
        OH, OW = oh + top + bottom, ow + left + right
        G = cfg.MAX_GT_INSTANCES
        zoom = None
        try:
            if scaled:
                if oh < 1 or ow < 1:
                    return host()
                zoom = self.zoom_tables(h, w, scale)
                if zoom[0].size != oh or zoom[1].size != ow:              # scipy rounds the zoomed size its own way: the host's
                    return host()
                ops.gtprep_zoom_check(h, w, 4 * (-(-N // 32)), oh, ow, top, left, OH, OW)
            ops.gtprep_check(OH, OW, 4 * (-(-N // 32)), N, G)
        except ops.GtPrepUnsupported:
            return host()
        plan = augmentation.draw_plan() if augmentation is not None else []
        mats = augmentation.matrices(plan, OH, OW) if plan else []
        packed = mask_bits_pack(mask)
        nb = packed.shape[2]
        with loader_stream(dev) as st:
            with torch.cuda.stream(st):
                img = image if on_dev else torch.from_numpy(np.ascontiguousarray(image)).to(dev, non_blocking=True)
                bits = torch.from_numpy(packed).to(dev, non_blocking=True)
                if scaled:                                                # resize_image / resize_mask, their np.pad included
                    if zoom[2] is None:
                        zoom[2], zoom[3] = (torch.from_numpy(t).to(dev, non_blocking=True) for t in zoom[:2])
                    img = ops.resize_image_u8(img.contiguous(), (oh, ow), (top, left), (OH, OW))
                    bits = ops.mask_bits_zoom(bits, zoom[2], zoom[3], (top, left), (OH, OW))
                elif (OH, OW) != (h, w):                                  # np.pad of resize_image / resize_mask
                    canvas = torch.zeros((OH, OW, C), dtype=torch.uint8, device=dev)
                    canvas[top:top + h, left:left + w] = img
                    planes = torch.zeros((OH, OW, nb), dtype=torch.uint8, device=dev)
                    planes[top:top + h, left:left + w] = bits
                    img, bits = canvas, planes
                if mats:
                    img, bits = augmentation.warp_device(img, bits, mats)
                count_d, _ = ops.mask_bits_stats(bits, N)
                table = torch.empty((5 * N,), dtype=torch.int32, pin_memory=True)
                table.copy_(count_d._base, non_blocking=True)
            st.synchronize()                                              # (also: the pageable uploads above are done)
        table = table.numpy()
        count, box = table[:N], table[N:].reshape(N, 4)
        keep = count > 0
        s = DeviceSample()
        s.img, s.bits, s.shape, s.scaled = img, bits, (OH, OW, C), scaled
        s.sel = np.flatnonzero(keep).astype(np.int32)
        s.class_ids = class_ids[keep]
        s.bbox = box[keep].astype(np.int32)
        active_class_ids = np.zeros([dataset.num_classes], dtype=np.int32)
        active_class_ids[dataset.source_class_ids[dataset.image_info[image_id]["source"]]] = 1
        s.image_meta = utils.compose_image_meta(image_id, shape, s.shape, window, scale, active_class_ids)
        return "device", s

    def new_batch(self, batch_size, shape):
        """The batch's two device tensors, float32 [B, H, W, C] and uint8 [B, H, W, MAX_GT_INSTANCES], allocated on the loader
        stream (every writer below runs there; the consumer declares its own use with record_stream, MaskRCNN._to_device)."""
        import torch
        from .loader_stream import loader_stream
        with loader_stream(self.device) as st:
            with torch.cuda.stream(st):
                return (torch.empty((batch_size,) + tuple(shape), dtype=torch.float32, device=self.device),
                        torch.empty((batch_size,) + tuple(shape[:2]) + (self.config.MAX_GT_INSTANCES,), dtype=torch.uint8,
                                    device=self.device))

    def emit(self, sample, sel, out_image, out_masks):
        """A device sample into its batch slots: the instances `sel` (bit indices) as planes, the image minus MEAN_PIXEL."""
        import torch
        from . import ops
        from .loader_stream import loader_stream
        OH, OW, _ = sample.shape
        with loader_stream(self.device) as st:
            with torch.cuda.stream(st):
                ops.mask_bits_gather(sample.bits, sel, self.config.MAX_GT_INSTANCES, out=out_masks)
                ops.mold_image_u8(sample.img, (OH, OW), (0, 0), (OH, OW), utils.mean_pixel(self.config, sample.shape[2]), out=out_image)
        _count("device")
        if sample.scaled:
            _count("scaled")

    def emit_host(self, molded, gt_masks, out_image, out_masks):
        """A host-built sample (float32 molded image, [H, W, k] masks) into the same batch slots."""
        import torch
        from . import ops
        from .loader_stream import loader_stream
        G = self.config.MAX_GT_INSTANCES
        packed = mask_bits_pack(gt_masks)
        sel = np.arange(gt_masks.shape[2], dtype=np.int32)
        molded = np.ascontiguousarray(molded, dtype=np.float32)
        with loader_stream(self.device) as st:
            with torch.cuda.stream(st):
                out_image.copy_(torch.from_numpy(molded), non_blocking=True)
                try:
                    ops.gtprep_check(packed.shape[0], packed.shape[1], packed.shape[2], sel.size, G)
                    ops.mask_bits_gather(torch.from_numpy(packed).to(self.device, non_blocking=True), sel, G, out=out_masks)
                except ops.GtPrepUnsupported:                             # past a cap: the planes cross unpacked
                    out_masks.copy_(torch.from_numpy(mask_bits_gather_host(packed, sel, G)), non_blocking=True)
            st.synchronize()                                              # pageable uploads: done before the arrays go away
        _count("host")

    def ready_event(self):
        """An event on the loader stream after everything enqueued so far: the batch's hand-off to its consumer."""
        import torch
        from .loader_stream import loader_stream
        with loader_stream(self.device) as st:
            ev = torch.cuda.Event()
            ev.record(st)
        return ev


class DeviceBatch(list):
    """The 7-item list data_generator yields, with `images` and `gt_masks` as device tensors and `ready`: the event (on the
    loader stream) after which they hold the batch.  MaskRCNN._to_device makes its stream wait on it."""
    ready = None
