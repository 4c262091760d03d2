#!/usr/bin/env python3
"""Ten eager training steps of the headline model (ResNet-101, 256 x 256, 4 images) without or with class weights on the head
losses, to be run under a kernel trace; tools/kernel_means.py then gives the five loss launches of each run:
    rocprofv3 --kernel-trace --output-format csv -d <dir> -- python tools/class_weight_steps.py [--weights]
    python tools/kernel_means.py <dir>/.../*_kernel_trace.csv loss
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--weights", action="store_true", help="class weights [1, 2.5, 0.4, 3] instead of none")
    ap.add_argument("--steps", type=int, default=10)
    args = ap.parse_args()
    import torch
    from caesar_mrcnn_amd.config import run_py_config
    from caesar_mrcnn_amd.model import MaskRCNN
    if not torch.cuda.is_available():
        sys.exit("class_weight_steps.py needs a GPU")
    cfg = run_py_config(num_classes=4, imgsize=256, backbone="resnet101", images_per_gpu=4)
    cfg.TRAIN_LAUNCH_TAPE = False
    model = MaskRCNN("training", cfg, "/tmp/mrcnn_logs", device=torch.device("cuda:0"), seed=1)
    rng = np.random.RandomState(0)
    B, S, G = 4, 256, 8
    images = rng.normal(20, 8, (B, S, S, 3)).astype(np.float32)
    gt_boxes = np.zeros((B, G, 4), np.int32)
    gt_cls = np.zeros((B, G), np.int32)
    gt_masks = np.zeros((B, S, S, G), bool)
    for b in range(B):
        for g in range(G):
            y, x, h, w = rng.randint(8, S - 72), rng.randint(8, S - 72), rng.randint(12, 64), rng.randint(12, 64)
            gt_boxes[b, g], gt_cls[b, g] = (y, x, y + h, x + w), rng.randint(1, 4)
            gt_masks[b, y:y + h, x:x + w, g] = True
            images[b, y:y + h, x:x + w] += 100
    meta = np.stack([np.array([b, S, S, 3, S, S, 3, 0, 0, S, S, 1.0] + [1] * cfg.NUM_CLASSES) for b in range(B)])
    inputs = [images, meta, None, None, gt_cls, gt_boxes, gt_masks]
    if args.weights:
        model.set_class_weights([1.0, 2.5, 0.4, 3.0])
    model.compile(0.001, 0.9)
    for _ in range(args.steps):
        losses = model.train_on_batch(inputs)
    torch.cuda.synchronize()
    print("class weights %s: losses of the last step %s" % (
        "none" if model.engine.class_weights is None else model.engine.class_weights.cpu().tolist(), losses.cpu().tolist()))


if __name__ == "__main__":
    main()
