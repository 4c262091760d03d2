"""The reference's training augmentation, with its per-pixel warps on the GPU.

`run.py train` in the reference augments with imgaug (scripts/run.py:1091-1100)::

    iaa.SomeOf((0, 2), [Fliplr(1.0), Flipud(1.0),
                        Affine(rotate=(-90, 90), mode='constant', cval=0.0),
                        Affine(translate_percent={"x": (-0.3, 0.3), "y": (-0.3, 0.3)}, mode='constant', cval=0.0)],
               random_order=True)

and load_image_gt (mrcnn/model.py:1323-1359) applies it to the image and to the uint8 instance masks.  This module states
that pipeline exactly, as a float64 host statement (`warp_host`), and runs it on the device (csrc/augment.hip) with the same
bytes.  imgaug bit-parity is UNPINNED: imgaug, cv2 and skimage are not installed, so the statement below is our definition,
checked on the CPU against a second source (scipy.ndimage.map_coordinates), not against imgaug.

Contract
--------
A plan is a list of 0, 1 or 2 stages, drawn per image from a numpy.random.RandomState `rng` (`ReferenceAugmenter.draw`):

* ``n = rng.randint(0, 3)`` (uniform on {0, 1, 2});
* the stages are ``rng.choice(4, n, replace=False)``, in the order drawn (random_order=True), each drawing its parameters
  right after the choice, in stage order:
  0 ``("fliplr",)``, 1 ``("flipud",)``, 2 ``("rotate", deg)`` with ``deg = rng.uniform(-90, 90)``,
  3 ``("translate", fx, fy)`` with ``fx = rng.uniform(-0.3, 0.3)``, then ``fy = rng.uniform(-0.3, 0.3)``;
  the shift is (fx * W, fy * H) pixels and need not be whole.

Each stage is an inverse map of an output pixel (x, y) to a source point (sx, sy) (`stage_matrix`):

* flips: sx = W - 1 - x, or sy = H - 1 - y;
* rotation about c = ((W - 1) / 2, (H - 1) / 2), d = (x, y) - c:  sx = cos t dx + sin t dy + cx,  sy = -sin t dx + cos t dy + cy
  (rotate(+90) on a square image is np.rot90(img, -1));
* translation: (sx, sy) = (x - tx, y - ty).

The host folds each stage into a 2 x 3 float64 matrix, (sx, sy) = (m00 x + m01 y + m02, m10 x + m11 y + m12); cos and sin
are evaluated on the host only and the device receives the six doubles by value.  Sampling is bilinear in float64, in this
order: x0 = floor(sx), fx = sx - x0 (the same for y), then (tl (1 - fx) + tr fx) (1 - fy) + (bl (1 - fx) + br fx) fy.  A tap
outside the image reads 0 (imgaug's mode='constant', cval=0).  Every stage writes its output before the next stage reads
it, as imgaug does: a uint8 image is rounded with np.rint (half to even), a mask bit is set where the value is > 0.5
(np.round of a 0 / 1 plane), a float image is cast back to its dtype without rounding.  Two interpolating stages are never
folded into one matrix (that would round once where the reference rounds twice).  Shapes never change.

Device path: `ReferenceAugmenter.apply` runs on the GPU when it has a device, the image is uint8 [H, W, C] with C <= 4 and
the masks are bool [H, W, N]; anything else takes the host statement, which gives the same bytes.  The masks cross PCIe
bit-packed (numpy.packbits, the layout of mrcnn_unpack_mask_bits) and are warped without unpacking; the results come back
to the host on purpose (load_image_gt drops empty instances and data_generator skips images without one: both decisions
are the host's).  The work goes to the loader threads' one side stream (loader_stream.py), and only that stream is
synchronised.  data_generator(device_samples=True) keeps both on the device instead (gtprep.py): it draws the plan with
`draw_plan`, warps tensors with `warp_device` -- the core `apply` runs on, too -- and brings back only the instances' pixel
counts and boxes, from which the host takes the same two decisions.
"""
import threading

import numpy as np

STAGES = ("fliplr", "flipud", "rotate", "translate")
_HOST_CHUNK = 32            # planes per float64 pass of warp_host (bounds its temporaries at 300 instances)


def stage_matrix(stage, H, W):
    """The 2 x 3 float64 inverse map of one stage on an H x W image."""
    kind = stage[0]
    if kind == "fliplr":
        return np.array([[-1.0, 0.0, W - 1.0], [0.0, 1.0, 0.0]])
    if kind == "flipud":
        return np.array([[1.0, 0.0, 0.0], [0.0, -1.0, H - 1.0]])
    if kind == "rotate":
        t = np.deg2rad(float(stage[1]))
        c, s = np.cos(t), np.sin(t)
        cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
        return np.array([[c, s, cx - c * cx - s * cy], [-s, c, cy + s * cx - c * cy]])
    if kind == "translate":
        tx, ty = float(stage[1]) * W, float(stage[2]) * H
        return np.array([[1.0, 0.0, -tx], [0.0, 1.0, -ty]])
    raise ValueError("unknown augmentation stage %r" % (stage,))


def warp_host(arr, m, kind="image"):
    """The host statement of one stage: arr [H, W] or [H, W, C] sampled bilinearly (float64, taps outside read 0) at the
    inverse map m (2 x 3).  kind "image": integer images rounded with np.rint, float images cast back; kind "mask": value
    > 0.5.  Returns a new array of arr's shape and dtype."""
    arr = np.asarray(arr)
    m = np.asarray(m, dtype=np.float64).reshape(2, 3)
    if kind not in ("image", "mask"):
        raise ValueError("kind must be 'image' or 'mask'")
    H, W = arr.shape[:2]
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    sx = m[0, 0] * xs + m[0, 1] * ys + m[0, 2]
    sy = m[1, 0] * xs + m[1, 1] * ys + m[1, 2]
    x0f, y0f = np.floor(sx), np.floor(sy)
    fx, fy = (sx - x0f)[..., None], (sy - y0f)[..., None]
    gx, gy = 1.0 - fx, 1.0 - fy
    x0 = np.clip(x0f, -2, W).astype(np.int64)              # (clipped: a tap stays outside iff it was)
    y0 = np.clip(y0f, -2, H).astype(np.int64)
    inx0, inx1 = (x0 >= 0) & (x0 < W), (x0 + 1 >= 0) & (x0 + 1 < W)
    iny0, iny1 = (y0 >= 0) & (y0 < H), (y0 + 1 >= 0) & (y0 + 1 < H)
    cx0, cx1 = np.clip(x0, 0, W - 1), np.clip(x0 + 1, 0, W - 1)
    cy0, cy1 = np.clip(y0, 0, H - 1), np.clip(y0 + 1, 0, H - 1)
    ins = [(iny0 & inx0)[..., None], (iny0 & inx1)[..., None], (iny1 & inx0)[..., None], (iny1 & inx1)[..., None]]
    a = arr.reshape(H, W, -1)
    out = np.empty(a.shape, dtype=arr.dtype)
    for c0 in range(0, a.shape[2], _HOST_CHUNK):
        src = a[:, :, c0:c0 + _HOST_CHUNK].astype(np.float64)
        tl = np.where(ins[0], src[cy0, cx0], 0.0)
        tr = np.where(ins[1], src[cy0, cx1], 0.0)
        bl = np.where(ins[2], src[cy1, cx0], 0.0)
        br = np.where(ins[3], src[cy1, cx1], 0.0)
        v = (tl * gx + tr * fx) * gy + (bl * gx + br * fx) * fy
        if kind == "mask":
            out[:, :, c0:c0 + _HOST_CHUNK] = v > 0.5
        elif np.issubdtype(arr.dtype, np.integer):
            info = np.iinfo(arr.dtype)
            out[:, :, c0:c0 + _HOST_CHUNK] = np.clip(np.rint(v), info.min, info.max)
        else:
            out[:, :, c0:c0 + _HOST_CHUNK] = v
    return out.reshape(arr.shape)


def _device_ok(image, mask):
    return (image.dtype == np.uint8 and image.ndim == 3 and 1 <= image.shape[2] <= 4 and image.shape[0] >= 1
            and image.shape[1] >= 1 and mask is not None and mask.dtype == np.bool_ and mask.ndim == 3
            and mask.shape[:2] == image.shape[:2])


class ReferenceAugmenter(object):
    """The reference's augmentation pipeline as the ``f(image, mask) -> (image, mask)`` callable that load_image_gt accepts
    (see the module docstring for the contract).  One instance is shared by all loader threads: `__call__` draws the plan
    from the instance's own RandomState under a lock.  device: a torch GPU device for the warps (MaskRCNN.train sets its
    engine's device when this is None); None keeps them on the host.  device_calls counts the calls that ran on the device."""

    def __init__(self, seed=None, device=None):
        self.device = device
        self.device_calls = 0
        self._rng = np.random.RandomState(seed)
        self._lock = threading.Lock()

    @staticmethod
    def draw(rng):
        """One plan: a list of 0, 1 or 2 stages (tuples, see STAGES)."""
        n = rng.randint(0, 3)
        stages = []
        for k in rng.choice(4, n, replace=False):
            if k == 2:
                stages.append(("rotate", rng.uniform(-90.0, 90.0)))
            elif k == 3:
                fx = rng.uniform(-0.3, 0.3)
                stages.append(("translate", fx, rng.uniform(-0.3, 0.3)))
            else:
                stages.append((STAGES[k],))
        return stages

    @staticmethod
    def matrices(stages, H, W):
        """The 2 x 3 float64 inverse maps of a plan on an H x W image, in stage order."""
        return [stage_matrix(s, H, W) for s in stages]

    def apply(self, image, mask, stages, device=None):
        """(image, mask) after the plan `stages`, same shapes.  device: overrides self.device for this call."""
        device = self.device if device is None else device
        mats = self.matrices(stages, image.shape[0], image.shape[1])
        if not mats:
            return image, mask
        if device is not None and _device_ok(image, mask):
            return self._apply_device(image, mask, mats, device)
        for m in mats:
            image = warp_host(image, m, "image")
            if mask is not None:
                mask = warp_host(mask, m, "mask")
        return image, mask

    def draw_plan(self):
        """The plan `__call__` would draw next, drawn the same way (the instance's RandomState, under its lock)."""
        with self._lock:
            return self.draw(self._rng)

    def __call__(self, image, mask):
        return self.apply(image, mask, self.draw_plan())

    def warp_device(self, img, bits, mats):
        """The tensor-in / tensor-out core of the device path: img [H, W, C] uint8 (C <= 4) and bits [H, W, nb] bit-packed masks
        (or None), both on the device, after every stage of `mats`; the inputs may be overwritten (ping-pong buffers).  The
        caller holds the loader stream (loader_stream.py) and has made it current; nothing synchronises here."""
        from . import ops
        img = self._warp_all(img, mats, ops.augment_warp_u8)
        if bits is not None:
            bits = self._warp_all(bits, mats, ops.augment_warp_mask_bits)
        if mats:
            self.device_calls += 1
        return img, bits

    def _apply_device(self, image, mask, mats, device):
        import torch
        from .loader_stream import loader_stream
        H, W, C = image.shape
        N = mask.shape[2]
        image = np.require(image, np.uint8, ["C", "W"])
        packed = None
        if N:
            packed = np.packbits(mask, axis=-1, bitorder="little")
            pad = -packed.shape[2] % 4                             # whole 32-bit words per pixel
            if pad:
                packed = np.concatenate([packed, np.zeros((H, W, pad), np.uint8)], axis=2)
        with loader_stream(device) as st:
            with torch.cuda.stream(st):
                img, bits = self.warp_device(torch.from_numpy(image).to(device, non_blocking=True),
                                             torch.from_numpy(packed).to(device, non_blocking=True) if N else None, mats)
                host_img = torch.empty((H, W, C), dtype=torch.uint8, pin_memory=True)
                host_img.copy_(img, non_blocking=True)
                if N:
                    host_bits = torch.empty(tuple(packed.shape), dtype=torch.uint8, pin_memory=True)
                    host_bits.copy_(bits, non_blocking=True)
            st.synchronize()
        out_img = host_img.numpy().copy()
        if not N:
            return out_img, mask
        return out_img, np.unpackbits(host_bits.numpy(), axis=-1, count=N, bitorder="little").view(bool)

    @staticmethod
    def _warp_all(src, mats, warp):
        """Every stage in order, ping-ponging between src and one more device buffer (each stage reads what the last wrote)."""
        import torch
        other = torch.empty_like(src)
        for m in mats:
            warp(src, m, out=other)
            src, other = other, src
        return src
