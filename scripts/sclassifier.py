#!/usr/bin/env python3
"""Classify the sources of a CAESAR catalogue with Mask R-CNN (reference: scripts/sclassifier.py).

    python scripts/sclassifier.py --image mosaic.fits --scatalog catalog.dat --weights weights.h5 [--cutout_batch 8] [--plan_device]

A window of --scutout_size pixels is cut around every catalogue source not yet seen in another source's window, the model runs
on it, and each catalogue source in the window gets the class and score of the detection whose box matches its own (IoU above
--iouThr).  The result is one catalogue, sclass_<image>.json and .dat under --outdir.  With --cutout_batch N the mosaic is
uploaded once and the windows are cut, NaN-filled, stretched and detected N at a time on the GPU; --plan_device computes the
member lists of the whole catalogue on the GPU.  Both give the catalogue of the one-at-a-time run and are off by default.
"""
import argparse
import logging
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

logger = logging.getLogger("mrcnn")
DEFAULT_LOGS_DIR = os.path.join(os.getcwd(), "logs")


def make_config(cutout_batch=0):
    """The reference's SClassifierConfig (scripts/sclassifier.py:32-130)."""
    from caesar_mrcnn_amd.config import Config

    class SClassifierConfig(Config):
        NAME = "sources"
        IMAGES_PER_GPU = max(1, int(cutout_batch))       # SClassifier hands the model that many cut-outs per detect call
        GPU_COUNT = 1
        NUM_CLASSES = 1 + 4
        CLASS_NAMES = ["bkg", "sidelobe", "source", "galaxy_C2", "galaxy_C3"]
        STEPS_PER_EPOCH = 1
        DETECTION_MIN_CONFIDENCE = 0
        DETECTION_NMS_THRESHOLD = 0.3
        RPN_ANCHOR_SCALES = (4, 8, 16, 32, 64)
        MAX_GT_INSTANCES = 300
        BACKBONE = "resnet101"
        BACKBONE_STRIDES = [4, 8, 16, 32, 64]
        IMAGE_RESIZE_MODE = "square"
        IMAGE_MIN_DIM = 256
        IMAGE_MAX_DIM = 256
        MEAN_PIXEL = np.array([0, 0, 0])
        RPN_NMS_THRESHOLD = 0.9
        RPN_TRAIN_ANCHORS_PER_IMAGE = 512
        TRAIN_ROIS_PER_IMAGE = 512
        RPN_ANCHOR_RATIOS = [0.5, 1, 2]
        LEARNING_RATE = 0.0005
        # (the reference also sets OPTIMIZER = "ADAM": nothing is trained here, so it is dropped)
        USE_MINI_MASK = False
    return SClassifierConfig()


def parse_args(argv=None):
    p = argparse.ArgumentParser(description='Use Mask R-CNN to classify radio sources')
    p.add_argument('--image', required=True, type=str, help='FITS image the catalogue was extracted from')
    p.add_argument('--scatalog', required=True, type=str, help='CAESAR source catalogue (ascii table)')
    p.add_argument('--weights', required=True, type=str, help='Path to weights .h5 file')
    p.add_argument('--logs', default=DEFAULT_LOGS_DIR, help='Logs and checkpoints directory (default=logs/)')
    p.add_argument('--scoreThr', default=0.7, type=float, help='Object detection score threshold')
    p.add_argument('--iouThr', default=0.6, type=float, help='IOU threshold used to match detected objects with catalogue sources')
    p.add_argument('--nsources_max', default=-1, type=int, help='Max number of sources to be processed')
    p.add_argument('--scutout_size', default=132, type=int, help='Source cutout image size')
    p.add_argument('--cutout_batch', default=0, type=int,
                   help='N >= 1: cut, stretch and detect N cut-outs at a time on the GPU (default 0: one at a time)')
    p.add_argument('--plan_device', action='store_true', default=False, help='Member lists of the whole catalogue on the GPU')
    p.add_argument('--outdir', default=".", type=str, help='Directory of sclass_<image>.json / .dat (default: the current one)')
    p.add_argument('--save_cutout_results', action='store_true', default=False,
                   help='Also write the out_<source>.json / .reg of every cut-out, as the reference does')
    return p.parse_args(argv)


def main(argv=None):
    logging.basicConfig(level=logging.INFO, format="%(asctime)s %(levelname)s - %(message)s")
    args = parse_args(argv)
    from caesar_mrcnn_amd import model as modellib
    from caesar_mrcnn_amd.classifier import SClassifier
    config = make_config(args.cutout_batch)
    config.display()
    logger.info("Creating model according to given config ...")
    model = modellib.MaskRCNN(mode="inference", config=config, model_dir=args.logs)
    logger.info("Loading weights %s ..." % args.weights)
    model.load_weights(args.weights, by_name=True)
    classifier = SClassifier(model, config)
    classifier.n_max_sources = args.nsources_max
    classifier.iou_thr, classifier.score_thr = args.iouThr, args.scoreThr
    classifier.scutout_size = args.scutout_size
    classifier.cutout_batch, classifier.plan_device = max(0, args.cutout_batch), args.plan_device
    classifier.outdir, classifier.save_cutout_results = args.outdir, args.save_cutout_results
    logger.info("Running source classification ...")
    if classifier.run(args.image, args.scatalog) < 0:
        logger.error("Failed to run source classifier!")
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
