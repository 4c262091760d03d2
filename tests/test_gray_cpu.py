"""Gray-level models (run.py --grayimg) without a GPU: the stem's input channels follow config.IMAGE_SHAPE[2], MEAN_PIXEL is
read as a scalar or a vector through utils.mean_pixel, the command line builds the configuration and the dataset the flag names,
and a gray image is [H, W, 1] float32."""
import importlib.util
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _run_py():
    spec = importlib.util.spec_from_file_location("_gray_run_py", os.path.join(ROOT, "scripts", "run.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _cfg(channels, backbone="custom"):
    from caesar_mrcnn_amd.config import run_py_config
    cfg = run_py_config(backbone=backbone, imgsize=128)
    cfg.IMAGE_CHANNEL_COUNT = channels
    cfg.IMAGE_SHAPE = np.array([128, 128, channels])
    return cfg


@pytest.mark.parametrize("backbone,stem", [("custom", 16), ("resnet50", 64), ("resnet101", 64)])
def test_stem_follows_the_image_channels(backbone, stem):
    from caesar_mrcnn_amd.params import ParamLayout, init_weights
    gray, rgb = ParamLayout(_cfg(1, backbone)), ParamLayout(_cfg(3, backbone))
    assert gray.offsets["conv1/kernel"][2] == (7, 7, 1, stem) and gray.offsets["conv1/kernel"][1] == 49 * stem
    assert rgb.offsets["conv1/kernel"][2] == (7, 7, 3, stem)
    # nothing else depends on the image's channels
    assert {k: v[2] for k, v in gray.offsets.items() if k != "conv1/kernel"} == {k: v[2] for k, v in rgb.offsets.items() if k != "conv1/kernel"}
    assert init_weights(gray, seed=1)["conv1/kernel"].shape == (7, 7, 1, stem)
    for name, (off, n, shape) in gray.offsets.items():
        assert off % 64 == 0, name                              # the 256-byte alignment of every tensor survives the smaller stem


@pytest.mark.parametrize("channels", [0, 2, 4])
def test_other_channel_counts_raise(channels):
    from caesar_mrcnn_amd import utils
    from caesar_mrcnn_amd.model import MaskRCNN
    from caesar_mrcnn_amd.params import ParamLayout
    cfg = _cfg(channels)
    with pytest.raises(ValueError, match="channels"):
        ParamLayout(cfg)
    with pytest.raises(ValueError, match="channels"):
        utils.image_channels(cfg)
    with pytest.raises(ValueError, match="channels"):           # before the engine, the library or a device is looked for
        MaskRCNN("inference", cfg, "/tmp/mrcnn_logs")


def test_mean_pixel_scalar_and_vector():
    from caesar_mrcnn_amd import utils
    cfg = _cfg(1)
    for value in (0, 0.0, np.float32(0), [0], np.zeros(1), np.array([0])):
        cfg.MEAN_PIXEL = value
        m = utils.mean_pixel(cfg)
        assert m.dtype == np.float64 and m.shape == (1,) and m[0] == 0.0
    cfg.MEAN_PIXEL = 7.5
    assert np.array_equal(utils.mean_pixel(cfg), [7.5])
    cfg.MEAN_PIXEL = np.array([123.7, 116.8, 103.9])            # an RGB mean does not fit a gray model
    with pytest.raises(ValueError, match="MEAN_PIXEL"):
        utils.mean_pixel(cfg)
    rgb = _cfg(3)
    rgb.MEAN_PIXEL = np.array([123.7, 116.8, 103.9])
    assert np.array_equal(utils.mean_pixel(rgb), np.array([123.7, 116.8, 103.9], np.float64))
    rgb.MEAN_PIXEL = 2                                          # a scalar stands for every channel
    assert np.array_equal(utils.mean_pixel(rgb), [2.0, 2.0, 2.0])
    rgb.MEAN_PIXEL = [1.0, 2.0]
    with pytest.raises(ValueError, match="MEAN_PIXEL"):
        utils.mean_pixel(rgb)
    # mold_image reads the same vector: float32 minus float64, as the reference's expression
    cfg.MEAN_PIXEL = 0.25
    img = np.arange(12, dtype=np.float32).reshape(3, 4, 1)
    got = utils.mold_image(img, cfg)
    assert got.dtype == np.float64 and np.array_equal(got, img.astype(np.float64) - 0.25)
    rgb.MEAN_PIXEL = np.array([1.0, 2.0, 3.0])
    img3 = np.arange(24, dtype=np.uint8).reshape(2, 4, 3)
    assert np.array_equal(utils.mold_image(img3, rgb), img3.astype(np.float32) - np.array([1.0, 2.0, 3.0]))
    assert np.array_equal(utils.unmold_image(utils.mold_image(img3, rgb), rgb), img3)


def test_build_config_grayimg():
    from caesar_mrcnn_amd import utils
    run = _run_py()
    classes = {"sidelobe": 1, "source": 2, "galaxy": 3}
    base = ["train", "--datalist", "x.dat", "--imgsize", "128", "--backbone", "custom"]
    gray = run.build_config(run.parse_args(base + ["--grayimg"]), classes)
    assert gray.IMAGE_CHANNEL_COUNT == 1
    assert tuple(int(v) for v in gray.IMAGE_SHAPE) == (128, 128, 1)
    assert np.array_equal(utils.mean_pixel(gray), [0.0])
    assert gray.IMG_TO_RGB is False
    assert utils.image_channels(gray) == 1
    rgb = run.build_config(run.parse_args(base), classes)
    assert rgb.IMAGE_CHANNEL_COUNT == 3
    assert tuple(int(v) for v in rgb.IMAGE_SHAPE) == (128, 128, 3)
    assert np.array_equal(np.asarray(rgb.MEAN_PIXEL), [0, 0, 0]) and np.array_equal(utils.mean_pixel(rgb), [0.0, 0.0, 0.0])
    assert rgb.IMG_TO_RGB is True
    # the flag changes an instance, not the class the next configuration starts from
    from caesar_mrcnn_amd.config import SDetectorConfig
    assert SDetectorConfig.IMAGE_CHANNEL_COUNT == 3 and SDetectorConfig.IMG_TO_RGB is True and SDetectorConfig().IMAGE_SHAPE[2] == 3


def _write_list(d, n=2, size=40):
    from caesar_mrcnn_amd import fits
    rng = np.random.RandomState(3)
    yy, xx = np.mgrid[0:size, 0:size]
    rows = []
    for i in range(n):
        blob = np.exp(-0.5 * (((yy - 20) / 4.0) ** 2 + ((xx - 17) / 6.0) ** 2))
        img = (rng.normal(0, 1, (size, size)) + 50 * blob).astype(np.float32)
        fits.write_fits(os.path.join(d, "img%d.fits" % i), img, {"BUNIT": "JY/BEAM"})
        fits.write_fits(os.path.join(d, "mask%d.fits" % i), (blob > 0.3).astype(np.float32))
        rows.append("%s,%s,source" % (os.path.join(d, "img%d.fits" % i), os.path.join(d, "mask%d.fits" % i)))
    lst = os.path.join(d, "train.dat")
    with open(lst, "w") as f:
        f.write("\n".join(rows) + "\n")
    return lst


def test_make_dataset_and_load_image(tmp_path):
    from caesar_mrcnn_amd import fits
    run = _run_py()
    lst = _write_list(str(tmp_path))
    base = ["train", "--datalist", lst, "--imgsize", "64", "--backbone", "custom"]
    for flags, rgb in (([], True), (["--grayimg"], False), (["--grayimg", "--no_uint8"], False), (["--no_uint8"], True)):
        ds = run.make_dataset(run.parse_args(base + flags), lst)
        assert ds is not None and ds.convert_to_rgb is rgb, flags
        image = ds.load_image(0)
        if rgb:
            assert image.shape == (40, 40, 3) and image.dtype == (np.float32 if "--no_uint8" in flags else np.uint8)
            continue
        assert image.shape == (40, 40, 1) and image.dtype == np.float32
        want = fits.read_fits(os.path.join(str(tmp_path), "img0.fits"), convertToRGB=False)[0]
        assert want.shape == (40, 40) and np.array_equal(image[:, :, 0], want)
        assert float(image.max()) == 1.0                          # zscale + normalisation: a gray image lives in [0, 1]


def test_host_loader_carries_gray_float_images(tmp_path):
    """load_image_gt on a [H, W, 1] float32 image at a scale other than 1, and the flips / rot90 callable of run.py: shapes and
    dtype survive, the pixels are resize_image's."""
    from caesar_mrcnn_amd import utils
    from caesar_mrcnn_amd.datagen import load_image_gt
    run = _run_py()
    lst = _write_list(str(tmp_path))
    args = run.parse_args(["train", "--datalist", lst, "--imgsize", "64", "--backbone", "custom", "--grayimg"])
    cfg = run.build_config(args, {"source": 1})
    ds = run.make_dataset(args, lst)
    raw = ds.load_image(1)
    for aug in (None, run.build_augmentation(args)):
        image, meta, class_ids, bbox, mask = load_image_gt(ds, cfg, 1, augmentation=aug)
        assert image.shape == (64, 64, 1) and image.dtype == np.float32 and mask.shape[:2] == (64, 64)
        assert tuple(meta[1:4]) == (40, 40, 1) and tuple(meta[4:7]) == (64, 64, 1)
        if aug is None:
            want = utils.resize_image(raw, min_dim=64, max_dim=64, min_scale=0, mode="square")[0]
            assert np.array_equal(image, want)
    molded = utils.mold_image(image, cfg)
    assert molded.shape == (64, 64, 1) and np.array_equal(molded, image.astype(np.float64))


def test_weight_mismatch_message_names_the_way_out():
    """engine.set_weights' size check, reached without a device: the message for conv1/kernel names exclude / the CLI flag."""
    from caesar_mrcnn_amd import engine
    from caesar_mrcnn_amd.params import ParamLayout, init_weights

    class _Stub(object):
        layout = ParamLayout(_cfg(1))
    w = init_weights(ParamLayout(_cfg(3)), seed=0)
    with pytest.raises(ValueError) as e:
        engine.MaskRCNNEngine.set_weights(_Stub(), {"conv1/kernel": w["conv1/kernel"]}, strict=False)
    msg = str(e.value)
    assert "conv1/kernel" in msg and 'exclude="conv1"' in msg and "--exclude_first_layer_weights" in msg


def test_draw_scene_takes_a_gray_frame_of_a_gray_configuration():
    """Analyzer._draw_scene: a uint8 [H, W, 1] frame is drawn as its three-fold copy when the configuration is a gray-level one;
    with an RGB configuration it is refused as before."""
    from caesar_mrcnn_amd.analyze import Analyzer
    frame = (np.arange(20 * 30, dtype=np.uint32) % 251).astype(np.uint8).reshape(20, 30, 1)
    scenes = {}
    for channels in (1, 3):
        cfg = _cfg(channels)
        cfg.CLASS_NAMES = ["bkg", "sidelobe", "source", "galaxy"]
        an = Analyzer(None, cfg)
        an.image, an.image_id = frame, "g"
        an.masks_final, an.bboxes, an.class_ids_final, an.scores_final, an.captions = [], [], [], [], []
        an.bboxes_gt, an.class_ids_gt_merged = [], []
        scenes[channels] = an._draw_scene()
    assert scenes[3] is None
    assert scenes[1] is not None and np.array_equal(scenes[1]["image"], np.repeat(frame, 3, axis=2))
