#!/usr/bin/env python3
"""Command line entry point with the reference's interface (scripts/run.py:1263-1384, 1448-1760):

    run.py train  --datalist train.dat [--datalist_val val.dat] --nepochs 10 --backbone resnet101 ...
    run.py test   --datalist test.dat  --weights w.h5 --scoreThr 0.7 --iouThr 0.6
    run.py detect --image map.fits --weights w.h5 [--xmin/--xmax/--ymin/--ymax] [--split_img_in_tiles ...]

Same flag names and defaults; the model behind them is caesar_mrcnn_amd.model.MaskRCNN (MI355X).
Multi-GPU training: ``torchrun --nproc-per-node NGPU scripts/run.py train --ngpu NGPU ...``.
`test` reports completeness / reliability per class from mask-IoU matching, or with `--reference_tester` runs the reference's
ModelTester (caesar_mrcnn_amd/analyze.py: confusion matrix, purity, completeness.csv and reliability.csv; with `--compute_map` also
its compute_mAP: mask AP per image and the Pascal-VOC box AP / mAP, and with `--sweep_map` the sweep over every score threshold
and the mAP over IoU 0.50 ... 0.95 of its second metric tool, caesar_mrcnn_amd/metrics.py); `detect` runs the Analyzer
post-processing (caesar_mrcnn_amd/analyze.py: score filter, connected-mask merging, best-of-overlapping
selection) on every tile and writes the objects as JSON (`out_<image>.json`: image_id, objs[name, x1, x2,
y1, y2, class_id, class_name, score, pixels, vertexes, edge]) and DS9 regions.  With `--draw` or `--detect_outfile NAME` it also
writes the overlay PNG of the frame (`out_<image>.png` or NAME; rendered on the GPU); matplotlib plots are not
produced.
`detect --split_img_in_tiles --merge_tile_sources` is the reference's SFinder (caesar_mrcnn_amd/sfinder.py): sources that
straddle tile borders are merged and one catalogue (objects gain `merged`, names S1..Sn) is written by rank 0; with
`--compute_source_params` every object also gains the reference's parameters (nPix, S .. flux, X0 .. Y0w_wcs, Xmin .. Ymax_wcs);
with `--tile_batch N` the mosaic is read and uploaded once and the tiles are cut, stretched and detected N at a time on the GPU;
with `--draw_mosaic` the overview picture of the whole mosaic, the merged catalogue drawn on it, is written as well.
"""
import argparse
import json
import logging
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

logger = logging.getLogger("mrcnn")
DEFAULT_LOGS_DIR = os.path.join(os.getcwd(), "logs")


def parse_args(argv=None):
    p = argparse.ArgumentParser(description='Train Mask R-CNN to detect radio sources.')
    p.add_argument("command", metavar="<command>", help="'train', 'test' or 'detect'")
    p.add_argument('--imgsize', type=int, default=256)
    p.add_argument('--grayimg', action='store_true', default=False)
    p.add_argument('--no_uint8', dest='to_uint8', action='store_false', default=True)
    p.add_argument('--no_zscale', dest='zscale', action='store_false', default=True)
    p.add_argument('--zscale_contrasts', type=str, default='0.25,0.25,0.25')
    p.add_argument('--biascontrast', action='store_true', default=False)
    p.add_argument('--bias', type=float, default=0.5)
    p.add_argument('--contrast', type=float, default=1.0)
    p.add_argument('--no_norm_img', dest='norm_img', action='store_false', default=True)
    p.add_argument('--classdict', type=str, default='{"sidelobe":1,"source":2,"galaxy":3}')
    p.add_argument('--classdict_model', type=str, default='')
    p.add_argument('--dataloader', type=str, default='datalist', help='{datalist,datalist_json,datadir_json}')
    p.add_argument('--datalist', default=None)
    p.add_argument('--datalist_train', default=None)
    p.add_argument('--datalist_val', default=None)
    p.add_argument('--datadir', default=None)
    p.add_argument('--validation_data_fract', type=float, default=0.1)
    p.add_argument('--maxnimgs', type=int, default=-1)
    p.add_argument('--weights', default=None, help="Path to weights .h5 (Keras) or .npz file")
    p.add_argument('--logs', default=DEFAULT_LOGS_DIR)
    p.add_argument('--nthreads', type=int, default=1)
    p.add_argument('--ngpu', type=int, default=1)
    p.add_argument('--nimg_per_gpu', type=int, default=1)
    p.add_argument('--nepochs', type=int, default=1)
    p.add_argument('--epoch_length', type=int, default=None)
    p.add_argument('--nvalidation_steps', type=int, default=None)
    p.add_argument('--rpn_anchor_scales', type=str, default='4,8,16,32,64')
    p.add_argument('--max_gt_instances', type=int, default=300)
    p.add_argument('--backbone', type=str, default='resnet101')
    p.add_argument('--backbone_strides', type=str, default='4,8,16,32,64')
    p.add_argument('--rpn_nms_threshold', type=float, default=0.7)
    p.add_argument('--rpn_train_anchors_per_image', type=int, default=512)
    p.add_argument('--train_rois_per_image', type=int, default=512)
    p.add_argument('--rpn_anchor_ratios', type=str, default='0.5,1,2')
    for n in ("rpn_class", "rpn_bbox", "mrcnn_class", "mrcnn_bbox", "mrcnn_mask"):
        p.add_argument('--%s_loss_weight' % n, type=float, default=1.0)
        p.add_argument('--%s_loss' % n, dest='%s_loss' % n, action='store_true', default=True)
        p.add_argument('--no_%s_loss' % n, dest='%s_loss' % n, action='store_false')
    p.add_argument('--mask_loss_function', type=str, default='binary_crossentropy',
                   choices=['binary_crossentropy', 'dice_coef_loss'])
    p.add_argument('--weight_classes', action='store_true', default=False)
    p.add_argument('--exclude_first_layer_weights', action='store_true', default=False)
    p.add_argument('--head_dtype', type=str, default="", help="extension: float16 | bfloat16 mask-head convolutions")
    p.add_argument('--no_augmentation', dest='use_augmentation', action='store_false', default=True)
    p.add_argument('--reference_augmentation', action='store_true', default=False,
                   help="extension: augment with the reference's imgaug pipeline (0-2 of flip lr / flip ud / rotate -90..90 / "
                        "translate +-30%%), warped on the GPU; default: flips + 90-degree rotations")
    p.add_argument('--device_samples', action='store_true', default=False,
                   help="extension: `train` assembles its samples on the GPU (padding, --reference_augmentation warps, kept "
                        "instances, boxes, batch planes; Config.DEVICE_SAMPLES); with the default flip / rot90 augmentation "
                        "the samples stay on the host and a log line says so: combine with --reference_augmentation or "
                        "--no_augmentation")
    p.add_argument('--device_sample_resize', action='store_true', default=False,
                   help="extension: with --device_samples, images the loader has to scale (cut-outs whose short side is not "
                        "--imgsize) are scaled on the GPU too, image and masks (Config.DEVICE_SAMPLE_RESIZE); without "
                        "--device_samples it is ignored and a log line says so")
    p.add_argument('--reference_tester', action='store_true', default=False,
                   help="extension: `test` runs the reference's ModelTester (masks merged and selected first, its matching rule, "
                        "confusion matrix and purity, completeness.csv and reliability.csv); needs a JSON dataloader; default: the "
                        "per-class completeness / reliability summary")
    p.add_argument('--compute_map', action='store_true', default=False,
                   help="with `test --reference_tester`: after the tables, the reference's compute_mAP -- per-image mask AP, the "
                        "Pascal-VOC box AP per class and mAP at IoU 0.5 and --iouThr (matched on the GPU)")
    p.add_argument('--map_outdir', type=str, default="",
                   help="with --compute_map: write the input files of the three external metric tools under this directory")
    p.add_argument('--sweep_map', action='store_true', default=False,
                   help="with --compute_map: also what the reference's second vendored tool (tarlen5-calculate-mean-ap) computes "
                        "from the boxes -- average precision over every score threshold at IoU 0.50 ... 0.95, their mAP and the "
                        "per-class APs at 0.5 and 0.6 -- printed as the tool prints them (matched on the GPU)")
    p.add_argument('--remap_classids', action='store_true', default=False)
    p.add_argument('--classid_remap_dict', type=str, default='', help='Dictionary used to remap detected classid to gt classid')
    p.add_argument('--consider_sources_near_mixed_sidelobes', dest='consider_sources_near_mixed_sidelobes', action='store_true',
                   default=True)
    p.add_argument('--no_consider_sources_near_mixed_sidelobes', dest='consider_sources_near_mixed_sidelobes', action='store_false')
    p.add_argument('--scoreThr', type=float, default=0.7)
    p.add_argument('--iouThr', type=float, default=0.6)
    p.add_argument('--image', type=str, default=None)
    for n in ("xmin", "xmax", "ymin", "ymax"):
        p.add_argument('--' + n, type=int, default=-1)
    p.add_argument('--detect_outfile', type=str, default="",
                   help="`detect`: draw the overlay PNG (the frame, the detected masks' contours, their boxes and scores) to this file")
    p.add_argument('--draw', action='store_true', default=False,
                   help="extension: draw the overlay PNGs under the reference's default names -- out_<image>.png in `detect`, "
                        "out_<base>_id<uuid>.png per image in `test --reference_tester` (the reference always draws; here it is off "
                        "by default).  A tiled `detect` (--split_img_in_tiles), merged or not, draws nothing")
    p.add_argument('--detect_outfile_json', type=str, default="")
    p.add_argument('--split_img_in_tiles', action='store_true', default=False)
    p.add_argument('--tile_xsize', type=int, default=512)
    p.add_argument('--tile_ysize', type=int, default=512)
    p.add_argument('--tile_xstep', type=float, default=1.0)
    p.add_argument('--tile_ystep', type=float, default=1.0)
    p.add_argument('--merge_tile_sources', action='store_true', default=False,
                   help="with --split_img_in_tiles: the reference's SFinder -- sources cut by tile borders or seen in several "
                        "overlapping tiles are merged (on the GPU) and ONE catalogue is written by rank 0; default: per-tile "
                        "objects concatenated")
    p.add_argument('--compute_source_params', action='store_true', default=False,
                   help="with --merge_tile_sources: add the reference's source parameters (pixel count, flux statistics, "
                        "centroids, sky positions) to every catalogue entry before it is written")
    p.add_argument('--tile_batch', type=int, default=0,
                   help="extension, with --split_img_in_tiles --merge_tile_sources: read and upload the mosaic once, cut and stretch "
                        "the tiles on the GPU and detect them N at a time (the model is built for batches of N); needs the default "
                        "stretch flags; default 0: one file read, host stretch and detect call per tile")
    p.add_argument('--draw_mosaic', action='store_true', default=False,
                   help="extension, with --split_img_in_tiles --merge_tile_sources: draw the overview picture of the whole mosaic -- "
                        "stretched as a tile is, shrunk by block maxima -- with the merged catalogue's contours, boxes and names on "
                        "it, to mosaic_<image>.png (rendered on the GPU)")
    p.add_argument('--mosaic_outfile', type=str, default="", help="--draw_mosaic to this file")
    p.add_argument('--mosaic_shrink', type=int, default=0,
                   help="with --draw_mosaic: mosaic pixels per picture pixel and side; default 0: ceil(longer side / 1024)")
    args = p.parse_args(argv)
    if (args.compute_map or args.map_outdir) and not (args.command == "test" and args.reference_tester):
        p.error("--compute_map / --map_outdir belong to `test --reference_tester`")
    if args.map_outdir and not args.compute_map:
        p.error("--map_outdir needs --compute_map")
    if args.sweep_map and not args.compute_map:
        p.error("--sweep_map needs --compute_map")
    return args


def tile_batch_of(args):
    """--tile_batch N where it means something: `detect --split_img_in_tiles --merge_tile_sources`; else 0."""
    n = getattr(args, "tile_batch", 0)
    return n if n >= 1 and args.command == "detect" and args.split_img_in_tiles and args.merge_tile_sources else 0


def draw_settings(args, ntiles=1):
    """(Analyzer.draw, Analyzer.outfile) of `detect`: --detect_outfile NAME draws to NAME, --draw under the default name; tiles are
    never drawn (they would all carry the image's name; the reference's TileTask does not draw either)."""
    wanted = bool(getattr(args, "draw", False) or getattr(args, "detect_outfile", ""))
    if wanted and ntiles > 1:
        logger.warning("A tiled detect draws nothing: --draw / --detect_outfile ignored")
    return wanted and ntiles == 1, getattr(args, "detect_outfile", "") or ""


def mosaic_settings(args):
    """(SFinder.draw_mosaic, SFinder.mosaic_outfile, SFinder.mosaic_shrink) of `detect`: --mosaic_outfile NAME implies
    --draw_mosaic; both mean something only with --split_img_in_tiles --merge_tile_sources, elsewhere one warning and nothing."""
    wanted = bool(getattr(args, "draw_mosaic", False) or getattr(args, "mosaic_outfile", ""))
    tiled = args.command == "detect" and args.split_img_in_tiles and args.merge_tile_sources
    if wanted and not tiled:
        logger.warning("--draw_mosaic / --mosaic_outfile need `detect --split_img_in_tiles --merge_tile_sources`: ignored")
    shrink = getattr(args, "mosaic_shrink", 0)
    return wanted and bool(tiled), getattr(args, "mosaic_outfile", "") or "", shrink if shrink >= 1 else None


def build_config(args, class_dict_model):
    """SDetectorConfig + the CLI overrides of scripts/run.py:1628-1706."""
    from caesar_mrcnn_amd.config import SDetectorConfig
    cfg = SDetectorConfig()
    cfg.NUM_CLASSES = len(class_dict_model) + 1
    cfg.CLASS_NAMES = ["bkg"] + [k for k, _ in sorted(class_dict_model.items(), key=lambda kv: kv[1])]
    cfg.CLASS_DICT = class_dict_model
    cfg.IMAGE_META_SIZE = 1 + 3 + 3 + 4 + 1 + cfg.NUM_CLASSES
    inference = args.command in ("test", "detect")
    cfg.GPU_COUNT = 1 if inference else args.ngpu
    cfg.IMAGES_PER_GPU = 1 if inference else args.nimg_per_gpu
    if tile_batch_of(args):
        cfg.IMAGES_PER_GPU = tile_batch_of(args)             # SFinder hands the model that many tiles per detect call
    cfg.LOSS_WEIGHTS = {"%s_loss" % n: getattr(args, "%s_loss_weight" % n)
                        for n in ("rpn_class", "rpn_bbox", "mrcnn_class", "mrcnn_bbox", "mrcnn_mask")}
    cfg.USE_LOSSES = {"%s_loss" % n: getattr(args, "%s_loss" % n)
                      for n in ("rpn_class", "rpn_bbox", "mrcnn_class", "mrcnn_bbox", "mrcnn_mask")}
    cfg.MASK_LOSS_FUNCTION = args.mask_loss_function
    cfg.RPN_ANCHOR_SCALES = tuple(int(v) for v in args.rpn_anchor_scales.split(","))
    cfg.MAX_GT_INSTANCES = args.max_gt_instances
    cfg.BACKBONE = args.backbone
    cfg.BACKBONE_STRIDES = [int(v) for v in args.backbone_strides.split(",")]
    cfg.RPN_NMS_THRESHOLD = args.rpn_nms_threshold
    cfg.RPN_TRAIN_ANCHORS_PER_IMAGE = args.rpn_train_anchors_per_image
    cfg.TRAIN_ROIS_PER_IMAGE = args.train_rois_per_image
    cfg.RPN_ANCHOR_RATIOS = [float(v) for v in args.rpn_anchor_ratios.split(",")]
    cfg.IMAGE_MIN_DIM = cfg.IMAGE_MAX_DIM = args.imgsize
    if args.grayimg:                       # scripts/run.py:897-900 / 1686-1689: one channel, nothing subtracted, no RGB conversion
        cfg.IMAGE_CHANNEL_COUNT = 1
        cfg.MEAN_PIXEL = np.zeros(1)
        cfg.IMG_TO_RGB = False
    cfg.IMAGE_SHAPE = np.array([args.imgsize, args.imgsize, cfg.IMAGE_CHANNEL_COUNT])
    cfg.ZSCALE_STRETCH, cfg.IMG_TO_UINT8, cfg.NORMALIZE_IMG = args.zscale, args.to_uint8, args.norm_img
    cfg.ZSCALE_CONTRASTS = [float(v) for v in args.zscale_contrasts.split(",")]
    cfg.BIAS_CONTRAST_STRETCH, cfg.IMG_BIAS, cfg.IMG_CONTRAST = args.biascontrast, args.bias, args.contrast
    cfg.IOU_THR, cfg.SCORE_THR = args.iouThr, args.scoreThr
    cfg.IMG_PATH = args.image or ""
    cfg.IMG_XMIN, cfg.IMG_XMAX, cfg.IMG_YMIN, cfg.IMG_YMAX = args.xmin, args.xmax, args.ymin, args.ymax
    cfg.SPLIT_IMG_IN_TILES = args.split_img_in_tiles
    cfg.TILE_XSIZE, cfg.TILE_YSIZE, cfg.TILE_XSTEP, cfg.TILE_YSTEP = args.tile_xsize, args.tile_ysize, args.tile_xstep, args.tile_ystep
    cfg.HEAD_DTYPE = args.head_dtype or None
    cfg.DEVICE_SAMPLES = bool(args.device_samples)
    cfg.DEVICE_SAMPLE_RESIZE = bool(getattr(args, "device_sample_resize", False)) and cfg.DEVICE_SAMPLES
    if getattr(args, "device_sample_resize", False) and not cfg.DEVICE_SAMPLES:
        logger.warning("--device_sample_resize needs --device_samples: ignored")
    return cfg


def make_dataset(args, path):
    from caesar_mrcnn_amd.dataset import SourceDataset
    ds = SourceDataset()
    if ds.set_class_dict(args.classdict) < 0:
        return None
    ds.apply_zscale, ds.convert_to_uint8 = args.zscale, args.to_uint8
    ds.convert_to_rgb = not args.grayimg              # gray: load_image returns float32 [H, W, 1]
    ds.zscale_contrasts = [float(v) for v in args.zscale_contrasts.split(",")]
    ds.apply_biascontrast, ds.bias, ds.contrast = args.biascontrast, args.bias, args.contrast
    if args.dataloader == 'datalist':
        rc = ds.load_data_from_list(path, args.maxnimgs)
    elif args.dataloader == 'datalist_json':
        rc = ds.load_data_from_json_list(path, args.maxnimgs)
    elif args.dataloader == 'datadir_json':
        rc = ds.load_data_from_json_search(path, args.maxnimgs)
    else:
        logger.error("Invalid/unknown dataloader (%s)!" % args.dataloader)
        return None
    if rc < 0:
        logger.error("Failed to load dataset %s" % path)
        return None
    ds.prepare()
    return ds


def build_augmentation(args):
    """The training augmentation: None with --no_augmentation; with --reference_augmentation the reference's pipeline
    (run.py:1091-1100, caesar_mrcnn_amd.augment.ReferenceAugmenter, warped on the training GPU); else flips + 90-degree
    rotations."""
    if not args.use_augmentation:
        return None
    if args.reference_augmentation:
        from caesar_mrcnn_amd.augment import ReferenceAugmenter
        return ReferenceAugmenter(seed=0)
    rng = np.random.RandomState(0)

    def aug(image, mask):        # flips + 90-degree rotations (imgaug SomeOf in run.py:1091-1100)
        if rng.rand() < 0.5:
            image, mask = np.fliplr(image), np.fliplr(mask)
        if rng.rand() < 0.5:
            image, mask = np.flipud(image), np.flipud(mask)
        k = rng.randint(0, 4)
        if image.shape[0] == image.shape[1]:
            image, mask = np.rot90(image, k), np.rot90(mask, k)
        return np.ascontiguousarray(image), np.ascontiguousarray(mask)
    return aug


def weight_classes_refusal(class_dict, class_dict_model):
    """--weight_classes: the weights are indexed by the model's class ids.  The message that refuses a training class
    dictionary with an id the model does not have, or None."""
    num_classes = len(class_dict_model) + 1
    bad = {k: v for k, v in class_dict.items() if not (isinstance(v, int) and 0 <= v < num_classes)}
    if not bad:
        return None
    return ("--weight_classes: class id(s) %s of --classdict are outside the model's %d classes (ids 0..%d, --classdict_model): "
            "their objects would have no weight" % (", ".join("%s=%r" % kv for kv in sorted(bad.items(), key=str)), num_classes,
                                                    num_classes - 1))


def log_class_weights(weights, cfg):
    names = list(getattr(cfg, "CLASS_NAMES", []))
    for cid, w in sorted(weights.items()):
        logger.info("Class weight of %s (id %d): %g" % (names[cid] if cid < len(names) else "?", cid, w))


def train(args, model, cfg):
    src = args.datadir if args.dataloader == 'datadir_json' else (args.datalist_train or args.datalist)
    ds_train = make_dataset(args, src)
    ds_val = make_dataset(args, args.datalist_val) if args.datalist_val else ds_train
    if ds_train is None or ds_val is None:
        return -1
    world = max(1, cfg.GPU_COUNT)
    cfg.STEPS_PER_EPOCH = args.epoch_length or max(1, len(ds_train.image_ids) // (cfg.IMAGES_PER_GPU * world))
    cfg.VALIDATION_STEPS = args.nvalidation_steps or max(1, len(ds_val.image_ids) // (cfg.IMAGES_PER_GPU * world))
    aug = build_augmentation(args)
    class_weights = None
    if args.weight_classes:                # (main() has refused a training dictionary with ids the model does not have)
        class_weights = ds_train.compute_class_weights()
        log_class_weights(class_weights, cfg)
    model.train(ds_train, ds_val, learning_rate=cfg.LEARNING_RATE, epochs=args.nepochs, layers='all', augmentation=aug,
                n_worker_threads=args.nthreads, class_weights=class_weights)
    return 0


def _mask_iou(a, b):
    inter = np.logical_and(a, b).sum()
    union = np.logical_or(a, b).sum()
    return inter / union if union else 0.0


def test_reference(args, model, cfg):
    """--reference_tester: the reference's test() (run.py:1132-1166) -- ModelTester over the dataset, two CSV tables written."""
    import ast
    from caesar_mrcnn_amd.analyze import ModelTester
    if args.dataloader == 'datalist':
        # The reference's tester reads the telescope, background and noise of every image from its metadata and raises on list
        # input, which has none.
        logger.error("--reference_tester needs the image metadata of a JSON dataset: use --dataloader datalist_json or datadir_json")
        return -1
    classid_remap_dict = {}
    if args.remap_classids:
        if args.classid_remap_dict == "":
            logger.error("Classid remap dictionary is empty (you need to provide one if you give the option --remap_classids)!")
            return -1
        try:
            classid_remap_dict = ast.literal_eval(args.classid_remap_dict)
        except Exception:
            logger.error("Failed to convert classid remap dict string to dict!")
            return -1
    ds = make_dataset(args, args.datadir if args.dataloader == 'datadir_json' else args.datalist)
    if ds is None:
        return -1
    ds.consider_sources_near_mixed_sidelobes = args.consider_sources_near_mixed_sidelobes
    tester = ModelTester(model, cfg, ds)
    tester.score_thr = args.scoreThr
    tester.iou_thr = args.iouThr
    tester.n_max_img = args.maxnimgs
    tester.remap_classids = args.remap_classids
    tester.classid_map = classid_remap_dict
    tester.draw = bool(getattr(args, "draw", False))
    tester.compute_mAP_metrics = bool(getattr(args, "compute_map", False))
    tester.metrics_outdir = getattr(args, "map_outdir", "") or None
    tester.sweep_map = bool(getattr(args, "sweep_map", False))
    tester.test()
    return 0


def test(args, model, cfg):
    if getattr(args, "reference_tester", False):
        return test_reference(args, model, cfg)
    ds = make_dataset(args, args.datadir if args.dataloader == 'datadir_json' else args.datalist)
    if ds is None:
        return -1
    C = cfg.NUM_CLASSES
    n_true, n_true_det = np.zeros(C), np.zeros(C)
    n_det, n_det_ok = np.zeros(C), np.zeros(C)
    for image_id in ds.image_ids:
        image = ds.load_image(image_id)
        gt_masks, gt_ids = ds.load_mask(image_id)
        r = model.detect([image], verbose=0)[0]
        keep = r["scores"] >= cfg.SCORE_THR
        det_masks, det_ids = r["masks"][:, :, keep], r["class_ids"][keep]
        matched_det = set()
        for g in range(gt_masks.shape[-1]):
            n_true[gt_ids[g]] += 1
            best, bj = 0.0, -1
            for j in range(det_masks.shape[-1]):
                iou = _mask_iou(gt_masks[:, :, g], det_masks[:, :, j])
                if iou > best:
                    best, bj = iou, j
            if best >= cfg.IOU_THR:
                n_true_det[gt_ids[g]] += 1
                matched_det.add(bj)
        for j in range(det_masks.shape[-1]):
            n_det[det_ids[j]] += 1
            if j in matched_det:
                n_det_ok[det_ids[j]] += 1
    for c in range(1, C):
        name = cfg.CLASS_NAMES[c]
        comp = n_true_det[c] / n_true[c] if n_true[c] else float("nan")
        rel = n_det_ok[c] / n_det[c] if n_det[c] else float("nan")
        print("class %s: completeness %.3f (%d/%d) reliability %.3f (%d/%d)" % (name, comp, n_true_det[c], n_true[c], rel,
                                                                                 n_det_ok[c], n_det[c]))
    return 0


def detect_merged(args, model, cfg):
    """--split_img_in_tiles --merge_tile_sources: SFinder.run_parallel (mrcnn/sfinder.py:549-638; the reference's run.py:1420-1437
    drives it the same way).  Tiles go round robin over the RANK / WORLD_SIZE processes; rank 0 gathers, merges and writes."""
    from caesar_mrcnn_amd.sfinder import SFinder
    base = os.path.splitext(os.path.basename(args.image))[0]
    sf = SFinder(model, cfg)
    sf.outfile_json = args.detect_outfile_json or ("out_%s.json" % base)
    sf.outfile_ds9 = os.path.splitext(sf.outfile_json)[0] + ".reg"
    sf.compute_params = bool(args.compute_source_params)
    sf.tile_batch = tile_batch_of(args)
    sf.draw_mosaic, sf.mosaic_outfile, sf.mosaic_shrink = mosaic_settings(args)
    if sf.run_parallel() < 0:
        logger.error("Failed to run the tiled source finder on image %s!" % args.image)
        return -1
    if sf.procId == sf.MASTER_ID:
        n_merged = sum(1 for s in sf.sources["sources"] if s["merged"])
        print("%d sources (%d merged across tiles) written to %s" % (len(sf.sources["sources"]), n_merged, sf.outfile_json))
    return 0


def detect(args, model, cfg):
    from caesar_mrcnn_amd import fits
    if not args.image:
        logger.error("No input image given (--image)")
        return -1
    if cfg.SPLIT_IMG_IN_TILES and args.merge_tile_sources:
        return detect_merged(args, model, cfg)
    tiles = [(args.xmin, args.xmax, args.ymin, args.ymax)]
    if cfg.SPLIT_IMG_IN_TILES:
        size = fits.get_fits_size(args.image)
        if size is None:
            return -1
        nx, ny = size
        x0, x1 = (args.xmin, args.xmax) if args.xmin >= 0 and args.xmax >= 0 else (0, nx - 1)
        y0, y1 = (args.ymin, args.ymax) if args.ymin >= 0 and args.ymax >= 0 else (0, ny - 1)
        tiles = fits.generate_tiles(x0, x1, y0, y1, cfg.TILE_XSIZE, cfg.TILE_YSIZE, cfg.TILE_XSTEP, cfg.TILE_YSTEP) or tiles
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    from caesar_mrcnn_amd.analyze import Analyzer
    base = os.path.splitext(os.path.basename(args.image))[0]
    analyzer = Analyzer(model, cfg)
    analyzer.score_thr, analyzer.iou_thr = args.scoreThr, args.iouThr
    analyzer.write_to_json = analyzer.write_to_ds9 = False          # one file for all tiles, written below
    analyzer.draw, analyzer.outfile = draw_settings(args, len(tiles))
    objs, regions = [], []
    for t, (xmin, xmax, ymin, ymax) in enumerate(tiles):
        if t % world != rank:            # tiles are independent: replicas only (sfinder.py:1235-1251 round-robin)
            continue
        res = fits.read_fits(args.image, xmin, xmax, ymin, ymax, stretch=cfg.ZSCALE_STRETCH,
                             zscale_contrasts=cfg.ZSCALE_CONTRASTS, normalize=cfg.NORMALIZE_IMG, convertToRGB=cfg.IMG_TO_RGB,
                             to_uint8=cfg.IMG_TO_UINT8, stretch_biascontrast=cfg.BIAS_CONTRAST_STRETCH, bias=cfg.IMG_BIAS,
                             contrast=cfg.IMG_CONTRAST)
        if res is None:
            return -1
        image, header = res
        if image.ndim == 2:                  # --grayimg: the model's gray image is [H, W, 1]
            image = image[:, :, None]
        analyzer.obj_name_tag = "t%d" % t if len(tiles) > 1 else ""
        if analyzer.predict(image, image_id=base, header=header, xmin=max(xmin, 0), ymin=max(ymin, 0)) < 0:
            logger.error("Failed to run model prediction on image %s!" % args.image)
            return -1
        if analyzer.results:
            objs.extend(analyzer.results["objs"])
            regions.extend(analyzer.obj_regions)
    suffix = "" if world == 1 else "_rank%d" % rank
    out = args.detect_outfile_json or ("out_%s%s.json" % (base, suffix))
    analyzer.results = {"image_id": base, "objs": objs}
    analyzer.write_json_results(out)
    analyzer.obj_regions = regions
    analyzer.write_ds9_regions(os.path.splitext(out)[0] + ".reg")
    print("%d sources written to %s" % (len(objs), out))
    return 0


def main(argv=None):
    logging.basicConfig(level=logging.INFO, format="%(asctime)s %(levelname)s - %(message)s")
    args = parse_args(argv)
    if args.command not in ("train", "test", "detect"):
        logger.error("Unknown command %s" % args.command)
        return 1
    if args.command in ("train", "test") and not (args.datalist or args.datalist_train or args.datadir):
        logger.error("Argument --datalist/--datadir is required for training/testing")
        return 1
    try:
        class_dict = json.loads(args.classdict)
        class_dict_model = json.loads(args.classdict_model) if args.classdict_model else class_dict
    except Exception:
        logger.error("Failed to convert class dict string to dict!")
        return 1
    if args.command == "train" and args.weight_classes:
        refusal = weight_classes_refusal(class_dict, class_dict_model)
        if refusal:
            logger.error(refusal)
            return 1
    if not (args.command == "detect" and args.split_img_in_tiles and args.merge_tile_sources):
        mosaic_settings(args)                    # the one warning for flags that mean nothing here
    from caesar_mrcnn_amd import model as modellib
    cfg = build_config(args, class_dict_model)
    cfg.display()
    mode = "training" if args.command == "train" else "inference"
    model = modellib.MaskRCNN(mode=mode, config=cfg, model_dir=args.logs)
    if args.weights:
        if args.exclude_first_layer_weights:
            model.load_weights(args.weights, by_name=True, exclude='conv1')
        else:
            model.load_weights(args.weights, by_name=True)
    else:
        logger.info("No weights given: starting from random initialisation")
    rc = {"train": train, "test": test, "detect": detect}[args.command](args, model, cfg)
    return 0 if rc == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
