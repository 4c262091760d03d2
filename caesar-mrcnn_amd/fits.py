"""FITS tile reader + zscale pre-processing: the step right before ``detect`` / ``load_image``
(reference: mrcnn/utils.py:989-1329 ``read_fits``, ``stretch_img``, ``normalize_img``, ``gray2rgb``,
``crop_img``, ``get_fits_header``, ``get_fits_size``, ``generate_tiles``).

astropy is not available on the target image, so this module carries
  * a dependency-free reader for the primary HDU of simple FITS images (2880-byte blocks, 80-char cards,
    BITPIX 8/16/32/64/-32/-64 big-endian, BSCALE/BZERO, NAXIS 2..4), and
  * a restatement of astropy.visualization.ZScaleInterval / ContrastBiasStretch [3P; parity unpinned:
    astropy itself cannot run here -- the algorithm follows the published astropy 2.x implementation,
    SURVEY App. C-6].
"""
import collections
import logging

import numpy as np

logger = logging.getLogger("mrcnn")

DEVICE_TILE_MAX_PIXELS = 4096 * 1024      # the size limit of the device chain (csrc/fits.hip: 4096 chunks of 1024 pixels)
# Chains without zscale that end in a gray image or skip the bias / contrast stretch too: on the device only from the size at
# which read_fits was measured ahead there (2048 x 2048; at 256 x 256 the host was level or ahead, no size between was measured)
DEVICE_LIGHT_CHAIN_MIN_PIXELS = 2048 * 2048

_BITPIX = {8: ">u1", 16: ">i2", 32: ">i4", 64: ">i8", -32: ">f4", -64: ">f8"}


class FitsHeader(dict):
    """Card values keyed by keyword (ints/floats/bools/strings parsed)."""


def _parse_card(card):
    key = card[:8].strip()
    if card[8:10] != "= " or key in ("COMMENT", "HISTORY", ""):
        return key, None
    body = card[10:]
    if body.lstrip().startswith("'"):
        s = body.lstrip()[1:]
        out, i = "", 0
        while i < len(s):
            if s[i] == "'":
                if i + 1 < len(s) and s[i + 1] == "'":
                    out += "'"
                    i += 2
                    continue
                break
            out += s[i]
            i += 1
        return key, out.rstrip()
    val = body.split("/")[0].strip()
    if val in ("T", "F"):
        return key, val == "T"
    try:
        return key, int(val)
    except ValueError:
        try:
            return key, float(val.replace("D", "E"))
        except ValueError:
            return key, val


def read_primary_hdu(filename, native=True):
    """Returns (data ndarray in native byte order with NAXISn..NAXIS1 axes, FitsHeader).  native=False leaves an unscaled
    image as the read-only big-endian view of the file's bytes (the device path swaps the tile it cuts, not the whole image)."""
    with open(filename, "rb") as f:
        raw = f.read()
    header = FitsHeader()
    pos, done = 0, False
    while not done:
        block = raw[pos:pos + 2880]
        if len(block) < 2880:
            raise ValueError("truncated FITS header in %s" % filename)
        for i in range(0, 2880, 80):
            card = block[i:i + 80].decode("ascii", "replace")
            if card.startswith("END") and card[3:].strip() == "":
                done = True
                break
            k, v = _parse_card(card)
            if v is not None and k not in header:
                header[k] = v
        pos += 2880
    if not header.get("SIMPLE", False):
        raise ValueError("%s is not a simple FITS file" % filename)
    naxis = int(header.get("NAXIS", 0))
    shape = [int(header["NAXIS%d" % (i + 1)]) for i in range(naxis)][::-1]
    dt = np.dtype(_BITPIX[int(header["BITPIX"])])
    n = int(np.prod(shape)) if shape else 0
    data = np.frombuffer(raw, dtype=dt, count=n, offset=pos).reshape(shape)
    bscale, bzero = header.get("BSCALE", 1), header.get("BZERO", 0)
    if bscale != 1 or bzero != 0:
        data = data.astype(np.float64) * bscale + bzero
        if dt.kind in "iu" or dt == np.dtype(">f4"):
            data = data.astype(np.float32)
    elif native:
        data = data.astype(dt.newbyteorder("="))
    return data, header


def write_fits(filename, data, extra_cards=None):
    """Minimal writer (float32, BITPIX = -32) -- used to synthesise test/benchmark tiles."""
    data = np.asarray(data, dtype=np.float32)
    cards = [("SIMPLE", True), ("BITPIX", -32), ("NAXIS", data.ndim)]
    cards += [("NAXIS%d" % (i + 1), n) for i, n in enumerate(data.shape[::-1])]
    cards += list((extra_cards or {}).items())
    lines = []
    for k, v in cards:
        if isinstance(v, bool):
            sv = "%20s" % ("T" if v else "F")
        elif isinstance(v, (int, np.integer)):
            sv = "%20d" % v
        elif isinstance(v, float):
            sv = "%20s" % repr(v)
        else:
            sv = "'%-8s'" % str(v)
        lines.append(("%-8s= %s" % (k, sv)).ljust(80))
    lines.append("END".ljust(80))
    hdr = "".join(lines)
    hdr += " " * ((2880 - len(hdr) % 2880) % 2880)
    body = data.astype(">f4").tobytes()
    body += b"\0" * ((2880 - len(body) % 2880) % 2880)
    with open(filename, "wb") as f:
        f.write(hdr.encode("ascii"))
        f.write(body)


# ---- stretches -------------------------------------------------------------------------------------
def zscale_limits(values, contrast=0.25, nsamples=1000, max_reject=0.5, min_npixels=5, krej=2.5,
                  max_iterations=5):
    """astropy.visualization.ZScaleInterval.get_limits [3P]."""
    values = np.asarray(values)
    values = values[np.isfinite(values)]
    stride = int(max(1.0, values.size / nsamples))
    samples = values[::stride][:nsamples]
    samples = np.sort(samples)
    npix = len(samples)
    vmin, vmax = samples[0], samples[-1]
    minpix = max(min_npixels, int(npix * max_reject))
    x = np.arange(npix)
    ngoodpix, last_ngoodpix = npix, npix + 1
    badpix = np.zeros(npix, dtype=bool)
    ngrow = max(1, int(npix * 0.01))
    kernel = np.ones(ngrow, dtype=bool)
    fit = (0.0, 0.0)
    for _ in range(max_iterations):
        if ngoodpix >= last_ngoodpix or ngoodpix < minpix:
            break
        fit = np.polyfit(x, samples, deg=1, w=(~badpix).astype(int))
        flat = samples - np.poly1d(fit)(x)
        threshold = krej * flat[~badpix].std()
        badpix[(flat < -threshold) | (flat > threshold)] = True
        badpix = np.convolve(badpix, kernel, mode='same')
        last_ngoodpix = ngoodpix
        ngoodpix = np.sum(~badpix)
    slope = fit[0]
    if ngoodpix >= minpix:
        if contrast > 0:
            slope = slope / contrast
        center_pixel = (npix - 1) // 2
        median = np.median(samples)
        vmin = max(vmin, median - (center_pixel - 1) * slope)
        vmax = min(vmax, median + (npix - center_pixel) * slope)
    return vmin, vmax


def sigma_clipped_stats(values, sigma=3.0, maxiters=5):
    """astropy.stats.sigma_clipped_stats with its defaults (cenfunc median, stdfunc std with ddof 0) [3P; parity unpinned:
    astropy cannot run here -- the algorithm is the documented one].  Non-finite values are dropped; every iteration takes
    c = median and s = std of what is kept and keeps c - sigma s <= x <= c + sigma s; it stops when an iteration removed nothing
    or after `maxiters`.  Works on the values as float64 (the median of an even count is the mean of the two middle values).
    Returns (mean, median, std, kept count, iterations run) of what is left -- NaNs when nothing is."""
    x = np.asarray(values).ravel()
    x = x[np.isfinite(x)].astype(np.float64)
    iters = 0
    while iters < maxiters and x.size:
        c, s = np.median(x), np.std(x)
        keep = (x >= c - sigma * s) & (x <= c + sigma * s)
        iters += 1
        removed = x.size - int(keep.sum())
        x = x[keep]
        if not removed:
            break
    if not x.size:
        return float("nan"), float("nan"), float("nan"), 0, iters
    return float(np.mean(x)), float(np.median(x)), float(np.std(x)), int(x.size), iters


def stretch_img(data, contrast=0.25):
    """ZScaleInterval(contrast)(data): map [vmin, vmax] to [0, 1] with clipping (utils.py:1166-1172)."""
    vmin, vmax = zscale_limits(data, contrast)
    out = np.subtract(data, float(vmin)).astype(np.float64)
    if (vmax - vmin) != 0:
        np.true_divide(out, vmax - vmin, out=out)
    return np.clip(out, 0.0, 1.0)


def stretch_img_biasconstrast(data, contrast=1, bias=0.5):
    """ContrastBiasStretch(contrast, bias)(data) = clip((x - bias) * contrast + 0.5, 0, 1) [3P]."""
    return np.clip((np.asarray(data, dtype=np.float64) - bias) * contrast + 0.5, 0.0, 1.0)


def normalize_img(data):
    return data / np.max(data)


def gray2rgb(data_float, to_uint8=True):
    if to_uint8:
        chans = [np.array((c * 255).round(), dtype=np.uint8) for c in data_float[:3]]
    else:
        chans = [np.array(c * 255, dtype=np.float32) for c in data_float[:3]]
    return np.stack(chans, axis=-1)


DeviceChain = collections.namedtuple("DeviceChain", "zscale biascontrast normalize out_kind zscale_contrasts bias contrast")
DeviceChain.__doc__ = """read_fits flags as the device chain takes them (mrcnn_fits_chain, include/mrcnn_hip.h).  out_kind: 0 uint8
[H, W, 3], 1 float32 [H, W, 3], 2 float32 [H, W]."""


def device_chain(stretch, normalize, convertToRGB, to_uint8, stretch_biascontrast, zscale_contrasts, contrast, bias, pixels=None):
    """Whether the device chain (csrc/fits.hip) computes read_fits with these flags: (DeviceChain, None), or (None, why) when the
    host path must run.  The only place that decides it -- read_fits(device=) and SFinder's batched front end both ask here.
    Refused: uint8 output with neither stretch.  Nothing then clips the channel to [0, 1] (radio maps are negative in half their
    pixels), the host casts out-of-range floats to uint8, and NumPy leaves that cast to the platform.  With either stretch on
    every value is in [0, 1] before the division; the float outputs are IEEE arithmetic whatever the values.
    pixels: the tile's size when the caller knows it.  Without zscale, a gray image or one without the bias / contrast stretch
    is a few host operations per pixel, and the device branch pays an upload and a download for them: measured behind or level
    with the host on a 256 x 256 tile and ahead on a 2048 x 2048 one, so these are refused below
    DEVICE_LIGHT_CHAIN_MIN_PIXELS."""
    if len(zscale_contrasts) != 3:
        zscale_contrasts = [0.25, 0.25, 0.25]                       # as read_fits: any other length is ignored
    try:
        zc = tuple(float(v) for v in zscale_contrasts)
        bias, contrast = float(bias), float(contrast)
    except (TypeError, ValueError):
        return None, "zscale contrasts, bias and contrast must be real numbers"
    stretch, normalize, stretch_biascontrast = bool(stretch), bool(normalize), bool(stretch_biascontrast)
    out_kind = (0 if to_uint8 else 1) if convertToRGB else 2        # without the RGB conversion to_uint8 is not looked at
    if out_kind == 0 and not stretch and not stretch_biascontrast:
        return None, "uint8 output with neither zscale nor the bias / contrast stretch: the cast of unclipped floats is platform-defined"
    if pixels is not None and pixels < DEVICE_LIGHT_CHAIN_MIN_PIXELS and not stretch and (out_kind == 2 or not stretch_biascontrast):
        return None, "no zscale and %s: the host is level or ahead below %d pixels" % (
            "a gray image" if out_kind == 2 else "no bias / contrast stretch", DEVICE_LIGHT_CHAIN_MIN_PIXELS)
    return DeviceChain(stretch, stretch_biascontrast, normalize, out_kind, zc, bias, contrast), None


def read_fits(filename, xmin=-1, xmax=-1, ymin=-1, ymax=-1, stretch=True, normalize=True, convertToRGB=True,
              zscale_contrasts=[0.25, 0.25, 0.25], to_uint8=True, stretch_biascontrast=False, contrast=1, bias=0.5, device=None,
              device_out=False):
    """Tile of a FITS image as the network's input image (utils.py:1033-1163): NaN -> min, per-channel
    zscale, normalise by the channel maximum, uint8 RGB.  Returns (image, header) or None on error.
    device: a torch GPU device -- the numeric part (everything after the header parse and the tile cut) runs there (the file's
    big-endian floats cross PCIe as they are) for every flag combination device_chain() accepts (mrcnn_fits_to_image); the
    image comes back to the host, identical to the host path's (uint8 byte for byte, float32 bit for bit).  device_out:
    True -- a uint8 RGB image of that device branch stays there, as a uint8 [H, W, 3] torch tensor (the device sample path of
    datagen.data_generator), a float32 image still comes back to the host; "any" -- every image of the device branch stays
    there, as a torch tensor of the host array's shape and dtype: uint8 [H, W, 3], float32 [H, W, 3] or, gray, float32 [H, W]
    (MaskRCNN.detect molds all three where they are).  A call that takes the host branch returns the host array as ever."""
    if len(zscale_contrasts) != 3:
        logger.warning("Size of input zscale_contrasts is !=3, ignoring inputs and using default (0.25,0.25,0.25)...")
        zscale_contrasts = [0.25, 0.25, 0.25]
    chain = None
    if device is not None:
        chain, _ = device_chain(stretch, normalize, convertToRGB, to_uint8, stretch_biascontrast, zscale_contrasts, contrast, bias)
    on_device = chain is not None
    try:
        data, header = read_primary_hdu(filename, native=not on_device)
    except Exception:
        logger.error('ERROR: Cannot read image file: ' + filename)
        return None
    read_tile = (xmin >= 0 and xmax >= 0 and ymin >= 0 and ymax >= 0)
    if read_tile:
        if xmax <= xmin:
            logger.error("xmax must be >xmin for tile reading!")
            return None
        if ymax <= ymin:
            logger.error("ymax must be >ymin for tile reading!")
            return None
    if data.ndim == 4:
        out = data[0, 0, ymin:ymax, xmin:xmax] if read_tile else data[0, 0, :, :]
    elif data.ndim == 2:
        out = data[ymin:ymax, xmin:xmax] if read_tile else data
    else:
        logger.error('ERROR: Invalid/unsupported number of channels found in file %s (nchan=%d)!' % (filename, data.ndim))
        return None
    if on_device and out.size and out.shape[0] * out.shape[1] <= DEVICE_TILE_MAX_PIXELS:
        chain, _ = device_chain(stretch, normalize, convertToRGB, to_uint8, stretch_biascontrast, zscale_contrasts, contrast, bias,
                                pixels=out.shape[0] * out.shape[1])
        if chain is not None:
            return _read_fits_device(out, chain, device, device_out), header
    out = out.astype(np.float32)
    out[np.isnan(out)] = np.nanmin(out)
    # The reference runs the whole per-channel chain three times (utils.py:1101-1157); the channels differ only in their
    # zscale contrast, so channels of equal contrast (all three on the run.py path: 0.25) are computed once and shared --
    # same values, a third of the host time of the loader threads (the feed-inclusive rate in bench.py's train_loop).
    done = {}

    def channel(zc):
        key = float(zc) if stretch else None
        if key not in done:
            c = out
            if stretch:
                c = stretch_img(c, zc).astype(np.float32)
            if stretch_biascontrast:
                c = stretch_img_biasconstrast(c, contrast, bias).astype(np.float32)
            if normalize:
                c = normalize_img(c).astype(np.float32)
            elif convertToRGB:
                c = normalize_img(c)
            done[key] = c
        return done[key]

    chans = [channel(zc) for zc in zscale_contrasts]
    if convertToRGB:
        return gray2rgb(chans, to_uint8), header
    return np.copy(chans[0]) if chans[0] is out else chans[0], header


def mosaic_overview_host(plane, shrink, contrast=0.25):
    """The overview frame of a whole mosaic, the statement ops.mosaic_overview is held to.  plane [ny, nx] (what
    SFinder._image_plane() returns); shrink: an integer k >= 1; contrast: a zscale contrast.
      G [ny, nx] uint8 = one channel of read_fits on the whole plane with the run.py flags and that contrast -- the same
        functions, type for type: astype(float32), NaN -> nanmin, stretch_img, normalize_img, round(255 x);
      O [ceil(ny / k), ceil(nx / k)]: O[Y, X] = max of G[k Y : k (Y + 1), k X : k (X + 1)] (partial blocks at the lower and
        right edge).  The maximum, not the mean: a compact source of a few pixels survives the shrink.
    Returns O in all three channels, uint8 [h, w, 3].  A plane without a single finite pixel gives zeros (read_fits raises
    there)."""
    k = int(shrink)
    if k != shrink or k < 1:
        raise ValueError("shrink must be an integer >= 1 (got %r)" % (shrink,))
    plane = np.asarray(plane)
    if plane.ndim != 2 or plane.size == 0:
        raise ValueError("plane must be a non-empty 2-D array (got shape %r)" % (plane.shape,))
    ny, nx = plane.shape
    h, w = -(-ny // k), -(-nx // k)
    out = plane.astype(np.float32)
    if not np.isfinite(out).any():
        return np.zeros((h, w, 3), np.uint8)
    out[np.isnan(out)] = np.nanmin(out)
    with np.errstate(invalid="ignore", divide="ignore"):
        c = stretch_img(out, contrast).astype(np.float32)
        c = normalize_img(c).astype(np.float32)
        G = np.array((c * 255).round(), dtype=np.uint8)
    padded = np.zeros((h * k, w * k), np.uint8)
    padded[:ny, :nx] = G
    O = padded.reshape(h, k, w, k).max(axis=(1, 3))
    return np.repeat(O[:, :, None], 3, axis=2)


def _read_fits_device(tile, chain, device, device_out=False):
    """The cut tile (still in the file's dtype / byte order) -> the image of `chain` (a DeviceChain) through ops.fits_to_image;
    returns a host array of the host path's shape and dtype (device_out True and a uint8 RGB image, or device_out "any": the
    device tensor, allocated on the loader stream, where its consumers run too).
    Called from loader threads while the main thread issues training steps: the three launches go to ONE side stream shared
    by all loader threads (its own hardware queue beside the step's three; a stream per thread would wrap onto the step's
    queues and wait behind a whole step) under a lock (the stream's scratch buffer is shared), and only that stream is
    synchronised (loader_stream.py)."""
    import torch
    from . import ops
    from .loader_stream import loader_stream
    H, W = tile.shape
    big = tile.dtype == np.dtype(">f4")
    if not big and tile.dtype != np.float32:
        tile = tile.astype(np.float32)                              # integer / float64 images: converted on the host as the host path does
    raw = torch.from_numpy(np.array(tile, order="C", copy=True).view(np.uint8).reshape(-1))   # (a writable copy: the file view is read-only)
    device = torch.device(device)
    device_out = device_out == "any" or (bool(device_out) and chain.out_kind == 0)
    with loader_stream(device) as st:
        with torch.cuda.stream(st):
            img = ops.fits_to_image(raw.to(device, non_blocking=True), H, W, chain, big_endian=big)
            if not device_out:
                host = torch.empty(tuple(img.shape), dtype=img.dtype, pin_memory=True)
                host.copy_(img, non_blocking=True)
        st.synchronize()                                            # (device_out too: `raw` is pageable and freed on return)
    return img if device_out else host.numpy().copy()


def read_table(filename):
    """Rows of a whitespace-separated ascii table (utils.py:984-987 hands the file to astropy.io.ascii, which cannot run here): a
    list of lists, one per line that is neither empty nor starts with '#'.  A column whose every value parses as a float becomes
    float, any other stays str.  Every row must have the first row's number of columns.  None when the file cannot be read or
    rows differ in length."""
    try:
        with open(filename) as f:
            rows = [line.split() for line in f if line.strip() and not line.lstrip().startswith("#")]
    except (OSError, UnicodeDecodeError):
        logger.error('ERROR: Cannot read table file: ' + str(filename))
        return None
    if any(len(r) != len(rows[0]) for r in rows):
        logger.error('ERROR: Rows of table %s differ in their number of columns' % filename)
        return None

    def number(v):
        try:
            return float(v)
        except ValueError:
            return None
    for c in range(len(rows[0]) if rows else 0):
        vals = [number(r[c]) for r in rows]
        if all(v is not None for v in vals):
            for r, v in zip(rows, vals):
                r[c] = v
    return rows


def get_fits_header(filename):
    try:
        return read_primary_hdu(filename)[1]
    except Exception:
        logger.error('ERROR: Cannot read image file: ' + filename)
        return None


def get_fits_size(filename):
    """(nx, ny) of the image plane (utils.py:1007-1030)."""
    try:
        data, _ = read_primary_hdu(filename)
    except Exception:
        logger.error('ERROR: Cannot read image file: ' + filename)
        return None
    if data.ndim not in (2, 4):
        return None
    return data.shape[-1], data.shape[-2]


def crop_img(data, x0, y0, dx, dy, stretch=False, normalize=False, convertToRGB=False):
    """Sub-image of size (dx, dy) around pixel (x0, y0) (utils.py:1211-1249)."""
    xmin, xmax = int(x0 - dx / 2), int(x0 + dx / 2)
    ymin, ymax = int(y0 - dy / 2), int(y0 + dy / 2)
    crop = data[ymin:ymax, xmin:xmax]
    crop[np.isnan(crop)] = np.nanmin(crop)
    if stretch:
        crop = stretch_img(crop).astype(np.float32)
    if normalize:
        crop = normalize_img(crop).astype(np.float32)
    if convertToRGB:
        if not normalize:
            crop = normalize_img(crop)
        crop = gray2rgb([crop, crop, crop])
    return crop


def generate_tiles(img_xmin, img_xmax, img_ymin, img_ymax, tileSizeX, tileSizeY, gridStepSizeX, gridStepSizeY):
    """(xmin, xmax, ymin, ymax) tuples covering the image, row-major (utils.py:1254-1329)."""
    if img_xmax <= img_xmin or img_ymax <= img_ymin:
        logger.error("xmax/ymax must be > xmin/ymin!")
        return None
    if tileSizeX <= 0 or tileSizeY <= 0:
        logger.error("Invalid box size given!")
        return None
    if gridStepSizeX <= 0 or gridStepSizeY <= 0 or gridStepSizeX > 1 or gridStepSizeY > 1:
        logger.error("Invalid grid step size given (null or negative)!")
        return None
    Nx, Ny = img_xmax - img_xmin + 1, img_ymax - img_ymin + 1
    if tileSizeX > Nx or tileSizeY > Ny:
        logger.warning("Invalid box size given (too small or larger than image size)!")
        return None
    stepX, stepY = int(np.round(gridStepSizeX * tileSizeX)), int(np.round(gridStepSizeY * tileSizeY))

    def spans(N, tile, step):
        out, idx = [], 0
        while idx <= N:
            off = min(tile, N - idx)
            if idx >= N or off == 0:
                break
            out.append((idx, idx + off))
            idx += step
        return out
    xs, ys = spans(Nx, tileSizeX, stepX), spans(Ny, tileSizeY, stepY)
    return [(img_xmin + x0, img_xmin + x1, img_ymin + y0, img_ymin + y1) for (y0, y1) in ys for (x0, x1) in xs]


# ---- world coordinates -------------------------------------------------------------------------------------
class SimpleWCS(object):
    """astropy.wcs.WCS(header).all_pix2world for the celestial pair of axes, on the host in float64 [3P; parity unpinned:
    astropy cannot run here -- the arithmetic is FITS WCS Paper I (linear part) and Paper II (zenithal deprojection, spherical
    rotation)].  Linear part: CRPIXi, then CDi_j, or PCi_j with CDELTi, or CROTA2 with CDELTi, then CRVALi.  Projections: -TAN
    and -SIN without PV terms; a pair of axes without a projection code is purely linear.  ``valid`` is False -- and the caller
    writes -999 -- for any other projection code or a header without CRVAL / CDELT (CDi_j) of both axes.  ``naxis`` as the
    reference uses it (sfinder.py:1079-1095): the number of axes of the header."""

    def __init__(self, header):
        h = header or {}
        self.naxis = int(h.get("WCSAXES", h.get("NAXIS", 2)))
        self.lng, self.lat, self.proj = 0, 1, ""
        self.valid, self.why = True, ""
        ctype = [str(h.get("CTYPE%d" % (i + 1), "")).upper() for i in range(max(self.naxis, 2))]
        lng = [i for i, c in enumerate(ctype) if c[:4] in ("RA--", "GLON", "ELON") or c[1:4] == "LON"]
        lat = [i for i, c in enumerate(ctype) if c[:4] in ("DEC-", "GLAT", "ELAT") or c[1:4] == "LAT"]
        if lng and lat:
            self.lng, self.lat = lng[0], lat[0]
            codes = [c[5:8].rstrip("-") if len(c) > 5 and c[4] == "-" else "" for c in (ctype[self.lng], ctype[self.lat])]
            self.proj = codes[0] if codes[0] == codes[1] else "?"
        i, j = self.lng + 1, self.lat + 1
        self.h = h
        has_cd = any(("CD%d_%d" % (a, b)) in h for a in (i, j) for b in (i, j))
        if not all(("CRVAL%d" % a) in h for a in (i, j)) or not (has_cd or all(("CDELT%d" % a) in h for a in (i, j))):
            self.valid, self.why = False, "no CRVAL / CDELT for the celestial axes"
        elif self.proj not in ("", "TAN", "SIN"):
            self.valid, self.why = False, "projection %r not supported" % self.proj
        elif self.proj == "SIN" and any(float(h.get("PV%d_%d" % (j, m), 0.0)) != 0.0 for m in (1, 2)):
            self.valid, self.why = False, "SIN projection with PV terms not supported"
        if not self.valid:
            return
        self.crpix = (float(h.get("CRPIX%d" % i, 0.0)), float(h.get("CRPIX%d" % j, 0.0)))
        self.crval = (float(h["CRVAL%d" % i]), float(h["CRVAL%d" % j]))
        if has_cd:
            self.m = [[float(h.get("CD%d_%d" % (a, b), 0.0)) for b in (i, j)] for a in (i, j)]
        else:
            cd = (float(h["CDELT%d" % i]), float(h["CDELT%d" % j]))
            if any(("PC%d_%d" % (a, b)) in h for a in (i, j) for b in (i, j)):
                pc = [[float(h.get("PC%d_%d" % (a, b), 1.0 if a == b else 0.0)) for b in (i, j)] for a in (i, j)]
            else:
                rho = np.deg2rad(float(h.get("CROTA%d" % j, 0.0)))        # the AIPS convention: rotation on the latitude axis
                c_, s_ = np.cos(rho), np.sin(rho)
                pc = [[c_, -s_ * cd[1] / cd[0]], [s_ * cd[0] / cd[1], c_]] if rho != 0.0 else [[1.0, 0.0], [0.0, 1.0]]
            self.m = [[cd[0] * pc[0][0], cd[0] * pc[0][1]], [cd[1] * pc[1][0], cd[1] * pc[1][1]]]
        self.lonpole = float(h.get("LONPOLE", 0.0 if self.crval[1] >= 90.0 else 180.0))

    @classmethod
    def from_header(cls, header):
        """SimpleWCS(header), or an invalid one (-999 for the sky keys) when the header's keywords cannot be used at all: a
        non-numeric CRVAL / CDELT, CDELT = 0 under CROTA2."""
        try:
            with np.errstate(all="ignore"):
                w = cls(header)
            if w.valid and not np.all(np.isfinite(np.asarray(w.m + [list(w.crval), list(w.crpix)], dtype=np.float64))):
                raise ValueError("non-finite transformation")
            return w
        except Exception as e:
            w = cls({})
            w.naxis = 2
            w.valid, w.why = False, "unusable WCS keywords (%s: %s)" % (type(e).__name__, e)
            return w

    def pix2world(self, x, y):
        """(longitude, latitude) in degrees of the 0-based pixel (x, y) along the celestial axes."""
        p = (float(x) + 1.0 - self.crpix[0], float(y) + 1.0 - self.crpix[1])
        u = self.m[0][0] * p[0] + self.m[0][1] * p[1]
        v = self.m[1][0] * p[0] + self.m[1][1] * p[1]
        if not self.proj:
            return self.crval[0] + u, self.crval[1] + v
        r = np.hypot(u, v)
        phi = np.arctan2(u, -v) if r != 0.0 else 0.0
        theta = np.arctan2(180.0 / np.pi, r) if self.proj == "TAN" else np.arccos(min(np.deg2rad(r), 1.0))
        dphi = phi - np.deg2rad(self.lonpole)
        dp = np.deg2rad(self.crval[1])
        st, ct = np.sin(theta), np.cos(theta)
        lng = self.crval[0] + np.rad2deg(np.arctan2(-ct * np.sin(dphi), st * np.cos(dp) - ct * np.sin(dp) * np.cos(dphi)))
        lat = np.rad2deg(np.arcsin(max(-1.0, min(1.0, st * np.sin(dp) + ct * np.cos(dp) * np.cos(dphi)))))
        return float(lng % 360.0), float(lat)

    def all_pix2world(self, points, origin):
        """Rows [x, y, ...] of pixel coordinates (origin 0 or 1) -> rows of world coordinates; the celestial pair is transformed,
        any further axis linearly (CRVAL + CDELT (p - CRPIX))."""
        out = []
        for pt in points:
            pt = [float(v) - float(origin) for v in pt]
            row = list(pt)
            row[self.lng], row[self.lat] = self.pix2world(pt[self.lng], pt[self.lat])
            for k in range(len(pt)):
                if k not in (self.lng, self.lat):
                    row[k] = float(self.h.get("CRVAL%d" % (k + 1), 0.0)) + float(self.h.get("CDELT%d" % (k + 1), 1.0)) * (
                        pt[k] + 1.0 - float(self.h.get("CRPIX%d" % (k + 1), 0.0)))
            out.append(row)
        return out
