"""The read_fits flag combinations the device chain takes (fits.device_chain), the host statement they are held to, and the
monotonicity argument the pixel kernel relies on for the channel maximum -- all without a GPU."""
import itertools
import os
import sys
import warnings

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

BIAS_CONTRAST = [(0.5, 1), (0.2, 3.5), (-1, 0.5), (2, 1), (0.5, 0), (0.5, -2)]


def test_device_chain_over_all_flag_combinations():
    """All 32 combinations of (stretch, normalize, convertToRGB, to_uint8, stretch_biascontrast): refused exactly when the output
    is uint8 RGB and neither stretch is on; out_kind 0 / 1 / 2 = uint8 RGB / float32 RGB / gray (to_uint8 is not looked at
    without the RGB conversion, as in read_fits); the descriptor carries the flags and nothing else."""
    from caesar_mrcnn_amd import fits
    n_ok = 0
    for stretch, normalize, rgb, u8, bc in itertools.product((False, True), repeat=5):
        chain, why = fits.device_chain(stretch, normalize, rgb, u8, bc, [0.1, 0.25, 0.6], 3.5, 0.2)
        refused = rgb and u8 and not stretch and not bc
        assert (chain is None) == refused, (stretch, normalize, rgb, u8, bc)
        assert (why is None) != refused
        if refused:
            assert isinstance(why, str) and "uint8" in why
            continue
        n_ok += 1
        assert chain.out_kind == ((0 if u8 else 1) if rgb else 2)
        assert (chain.zscale, chain.biascontrast, chain.normalize) == (stretch, bc, normalize)
        assert chain.zscale_contrasts == (0.1, 0.25, 0.6) and (chain.bias, chain.contrast) == (0.2, 3.5)
        assert chain._fields == ("zscale", "biascontrast", "normalize", "out_kind", "zscale_contrasts", "bias", "contrast")
    assert n_ok == 30


def test_device_chain_leaves_light_chains_of_small_tiles_to_the_host():
    """With the tile size given: no zscale and a gray image, or no zscale and no bias / contrast stretch either, is refused
    below DEVICE_LIGHT_CHAIN_MIN_PIXELS (the host was measured level or ahead on a 256 x 256 tile) and accepted from it on;
    every other combination does not depend on the size."""
    from caesar_mrcnn_amd import fits
    assert fits.DEVICE_LIGHT_CHAIN_MIN_PIXELS == 2048 * 2048 <= fits.DEVICE_TILE_MAX_PIXELS
    n_light = 0
    for stretch, normalize, rgb, u8, bc in itertools.product((False, True), repeat=5):
        flags = (stretch, normalize, rgb, u8, bc, [0.25] * 3, 1, 0.5)
        whole = fits.device_chain(*flags)
        small = fits.device_chain(*flags, pixels=256 * 256)
        large = fits.device_chain(*flags, pixels=2048 * 2048)
        assert large == whole
        light = whole[0] is not None and not stretch and (not rgb or not bc)
        n_light += light
        if light:
            assert small[0] is None and "host" in small[1]
        else:
            assert small == whole
    assert n_light == 2 * 4 + 2                    # gray: normalize x to_uint8 x bias/contrast; float32 RGB with no stretch: normalize


def test_device_chain_replaces_a_contrast_list_of_the_wrong_length():
    from caesar_mrcnn_amd import fits
    for zc in ([], [0.3], [0.3, 0.4], [0.1, 0.2, 0.3, 0.4]):
        chain, why = fits.device_chain(True, True, True, True, False, zc, 1, 0.5)
        assert why is None and chain.zscale_contrasts == (0.25, 0.25, 0.25)
        assert (chain.zscale, chain.biascontrast, chain.normalize, chain.out_kind) == (True, False, True, 0)
    chain, _ = fits.device_chain(True, True, True, True, False, (0.3, 0.4, 0.5), 1, 0.5)
    assert chain.zscale_contrasts == (0.3, 0.4, 0.5)
    assert fits.device_chain(True, True, True, True, True, [0.25] * 3, "x", 0.5)[0] is None


def _tile(seed=5, h=40, w=37):
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    img = rng.normal(0.0, 1.0, (h, w)).astype(np.float32)
    img += (50 * np.exp(-0.5 * (((yy - 12) / 3.0) ** 2 + ((xx - 20) / 4.0) ** 2))).astype(np.float32)
    img[rng.uniform(size=img.shape) < 0.03] = np.nan
    return img


def test_host_statement_of_four_combinations(tmp_path):
    """read_fits(device=None) against the chain spelt out here from stretch_img, stretch_img_biasconstrast and normalize_img: the
    yardstick the device is held to, pinned first."""
    from caesar_mrcnn_amd import fits
    img = _tile()
    assert np.isnan(img).any() and (img < 0).any()
    path = str(tmp_path / "tile.fits")
    fits.write_fits(path, img)
    filled = img.copy()
    filled[np.isnan(filled)] = np.nanmin(filled)
    zcs = [0.1, 0.25, 0.6]
    # zscale + bias / contrast, uint8 RGB
    got, _ = fits.read_fits(path, stretch_biascontrast=True, contrast=3.5, bias=0.2, zscale_contrasts=zcs)
    chans = []
    for zc in zcs:
        c = fits.stretch_img(filled, zc).astype(np.float32)
        c = fits.stretch_img_biasconstrast(c, 3.5, 0.2).astype(np.float32)
        c = fits.normalize_img(c).astype(np.float32)
        chans.append(np.array((c * 255).round(), dtype=np.uint8))
    want = np.stack(chans, axis=-1)
    assert got.dtype == np.uint8 and got.shape == (40, 37, 3) and np.array_equal(got, want)
    assert len(np.unique(got)) > 20 and not np.array_equal(got[..., 0], got[..., 2])
    # bias / contrast alone, normalize off: the RGB conversion normalises anyway; float32 RGB
    got, _ = fits.read_fits(path, stretch=False, normalize=False, to_uint8=False, stretch_biascontrast=True, contrast=0.5, bias=-1)
    c = fits.stretch_img_biasconstrast(filled, 0.5, -1).astype(np.float32)
    c = fits.normalize_img(c)
    want = np.stack([np.array(c * 255, dtype=np.float32)] * 3, axis=-1)
    assert got.dtype == np.float32 and got.shape == (40, 37, 3) and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # zscale alone, gray, not normalised: channel 0 with the first contrast
    got, _ = fits.read_fits(path, normalize=False, convertToRGB=False, zscale_contrasts=zcs)
    want = fits.stretch_img(filled, 0.1).astype(np.float32)
    assert got.dtype == np.float32 and got.shape == (40, 37) and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # no stretch, normalised gray with a negative contrast on the bias / contrast stretch
    got, _ = fits.read_fits(path, stretch=False, convertToRGB=False, stretch_biascontrast=True, contrast=-2, bias=0.5)
    c = fits.stretch_img_biasconstrast(filled, -2, 0.5).astype(np.float32)
    want = fits.normalize_img(c).astype(np.float32)
    assert got.dtype == np.float32 and got.shape == (40, 37) and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert want.max() == 1.0 and want.min() == 0.0


def _bits(x):
    return np.asarray(x, dtype=np.float32).view(np.uint32)


def test_channel_maximum_is_the_chain_of_an_end_of_the_tile():
    """The argument the pixel kernel takes its channel maximum from: every step of the map (float32 subtraction, float64
    division, clip, float32 rounding; float64 subtraction, multiplication, addition, clip, float32 rounding) is monotone and
    correctly rounded, so max(channel) is the chain applied to the tile's maximum -- to its minimum for a negative contrast -- bit
    for bit.  200 random float32 tiles x 6 (bias, contrast) x with / without zscale.  A failure here means the kernel needs a
    reduction pass over the pixels after all."""
    from caesar_mrcnn_amd import fits
    rng = np.random.RandomState(20)
    n = 0
    for t in range(200):
        h, w = rng.randint(1, 40), rng.randint(1, 40)
        tile = (rng.normal(0.0, 1.0, (h, w)) * 10.0 ** rng.uniform(-3, 3) + rng.normal(0.0, 1.0) * 10.0 ** rng.uniform(-3, 2))
        if t % 3 == 0:
            tile[rng.randint(h), rng.randint(w)] += 10.0 ** rng.uniform(0, 4)         # a bright pixel
        tile = tile.astype(np.float32)
        if t % 10 == 0:
            tile = (tile / np.float32(3)).astype(np.float32) if t % 20 else np.round(tile) + np.float32(0.5)     # odd mantissas / many ties
        ends = np.array([tile.min(), tile.max()], dtype=np.float32)
        for zscale in (False, True):
            if zscale:
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    zc = float(rng.choice([0.1, 0.25, 0.6]))
                    vmin, vmax = fits.zscale_limits(tile, zc)

                    def stretch(x):                                               # stretch_img with the tile's limits
                        out = np.subtract(x, float(vmin)).astype(np.float64)
                        if (vmax - vmin) != 0:
                            np.true_divide(out, vmax - vmin, out=out)
                        return np.clip(out, 0.0, 1.0).astype(np.float32)
                    base = fits.stretch_img(tile, zc).astype(np.float32)
                    assert np.array_equal(_bits(stretch(tile)), _bits(base))
                    base_ends = stretch(ends)
                    assert _bits(base.max()) == _bits(base_ends[1]) and base.min() == base_ends[0]
            else:
                base, base_ends = tile, ends
            for bias, contrast in BIAS_CONTRAST:
                c = fits.stretch_img_biasconstrast(base, contrast, bias).astype(np.float32)
                e = fits.stretch_img_biasconstrast(base_ends, contrast, bias).astype(np.float32)
                want = e[0] if contrast < 0 else e[1]
                assert _bits(c.max()) == _bits(want), (t, zscale, bias, contrast)
                if contrast == 0:
                    assert c.min() == c.max()                                     # a constant channel
                n += 1
    assert n == 200 * 2 * 6
