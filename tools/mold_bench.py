"""Molding float32 images for detect(): the host statement against the device path, the two kernels of
mrcnn_mold_image_f32 alone, and the stem convolution at one input channel beside three.  Writes one JSON object with --out
(default profiles/gray_float_bench.json); the later forms add to the file the first one wrote.

    python tools/mold_bench.py [--sizes 256,1024] [--reps 5] [--out FILE]
    rocprofv3 --kernel-trace --output-format csv -d <dir> -- python tools/mold_bench.py --kernels-only
    python tools/mold_bench.py --kernel-trace <dir>/.../<pid>_kernel_trace.csv [--out FILE]
    rocprofv3 --kernel-trace --output-format csv -d <dir> -- python tools/mold_bench.py --train-steps CHANNELS

  mold        a float32 HOST array of size x size pixels and C channels to the molded batch ON THE DEVICE, where the graph reads
              it: host = MaskRCNN.mold_inputs, the float32 cast and the upload; device = MaskRCNN._mold_inputs_device (upload of the
              image, mrcnn_mold_image_f32).  "unscaled": the canvas is the image's size; "scaled": the canvas is twice the image's
              side (bilinear up-scaling and the min / max pass).  perf_counter with the device synchronised before and after, host
              and device alternating within every repetition, median of --reps.  `host_over_device` > 1: the device path is ahead.
  kernels     --kernels-only issues, on a 2048 x 2048 canvas, groups of launches of mrcnn_mold_image_f32 per (C, scaled); under
              rocprofv3 the trace holds every launch, and --kernel-trace reads the rows back in issue order: median duration of the
              timed launches of each group, the bytes the pass has to move (pixel kernel: 4 read per source value + 4 written per
              canvas value; min / max: 4 read per source value) per second and its fraction of the 6.3 TB/s copy rate.
  train-steps --train-steps C runs ten training steps of the headline model (ResNet-101, 256 x 256, 4 images) with C input
              channels; tools/step_kernels.py on the trace lists the stem's forward and weight-gradient launches."""
import argparse
import csv
import json
import os
import sys
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_COPY_RATE = 6.3e12                    # bytes / s, the copy rate DESIGN.md 4.20 compares with
KERNEL_CANVAS = 2048
KERNEL_WARM, KERNEL_TIMED = 3, 10
KERNEL_GROUPS = [(1, False), (3, False), (1, True), (3, True)]          # (channels, scaled: a 1024 x 1024 source doubled)
KERNEL_NAMES = ("mold_f32_minmax_partial_kernel", "mold_f32_minmax_final_kernel", "mold_f32_resize_kernel")


def synth_image(size, C, seed=3):
    rng = np.random.RandomState(seed)
    return (rng.normal(0.3, 0.2, (size, size, C))).astype(np.float32)


def molder(C, canvas, dev):
    """A MaskRCNN without its engine: both molding paths read the configuration and the device only."""
    from caesar_mrcnn_amd.config import run_py_config
    from caesar_mrcnn_amd.model import MaskRCNN
    cfg = run_py_config(backbone="custom", imgsize=canvas, mode="inference")
    cfg.IMAGE_CHANNEL_COUNT, cfg.IMAGE_SHAPE = C, np.array([canvas, canvas, C])
    cfg.MEAN_PIXEL = 0 if C == 1 else np.zeros(3)
    m = object.__new__(MaskRCNN)
    m.config, m.engine = cfg, types.SimpleNamespace(dev=dev)
    return m


def bench_mold(sizes, reps, dev):
    import torch
    from caesar_mrcnn_amd import model as model_mod
    model_mod.DEVICE_MOLD_F32_MIN_PIXELS = 0              # measure the device path at every size
    rows = []

    def host(m, img):
        molded, metas, windows = m.mold_inputs([img])
        return torch.from_numpy(np.ascontiguousarray(molded, dtype=np.float32)).to(dev)

    def device(m, img):
        return m._mold_inputs_device([img])[0]
    for size in sizes:
        for C in (1, 3):
            for scaled in (False, True):
                m = molder(C, 2 * size if scaled else size, dev)
                img = synth_image(size, C)
                a, b = host(m, img), device(m, img)
                torch.cuda.synchronize()
                equal = bool(torch.equal(a.view(torch.int32), b.view(torch.int32)))
                t = {"host": [], "device": []}
                for _ in range(2):                         # warm-up of both
                    host(m, img), device(m, img)
                torch.cuda.synchronize()
                for _ in range(reps):
                    for name, f in (("host", host), ("device", device)):
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        f(m, img)
                        torch.cuda.synchronize()
                        t[name].append(time.perf_counter() - t0)
                h, d = float(np.median(t["host"])), float(np.median(t["device"]))
                rows.append({"size": size, "channels": C, "scaled": scaled, "canvas": 2 * size if scaled else size, "bit_equal": equal,
                             "host_ms": round(1e3 * h, 3), "device_ms": round(1e3 * d, 3), "host_over_device": round(h / d, 2),
                             "host_all_ms": [round(1e3 * v, 3) for v in t["host"]], "device_all_ms": [round(1e3 * v, 3) for v in t["device"]]})
                sys.stderr.write("[mold_bench] %r\n" % (rows[-1],))
    return rows


def issue_kernels(dev):
    import torch
    from caesar_mrcnn_amd import ops
    for C, scaled in KERNEL_GROUPS:
        side = KERNEL_CANVAS // 2 if scaled else KERNEL_CANVAS
        src = torch.from_numpy(synth_image(side, C)).to(dev)
        out = torch.empty((KERNEL_CANVAS, KERNEL_CANVAS, C), dtype=torch.float32, device=dev)
        for _ in range(KERNEL_WARM + KERNEL_TIMED):
            ops.mold_image_f32(src, (KERNEL_CANVAS, KERNEL_CANVAS), (0, 0), (KERNEL_CANVAS, KERNEL_CANVAS), 0.0, out=out)
        torch.cuda.synchronize()


def read_trace(path):
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    per = {n: [int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in rows if r["Kernel_Name"].split("(")[0].replace("void ", "").startswith(n)]
           for n in KERNEL_NAMES}
    n_scaled = sum(1 for _, s in KERNEL_GROUPS if s)
    per_group = KERNEL_WARM + KERNEL_TIMED
    assert len(per["mold_f32_resize_kernel"]) == per_group * len(KERNEL_GROUPS), len(per["mold_f32_resize_kernel"])
    assert len(per["mold_f32_minmax_partial_kernel"]) == per_group * n_scaled == len(per["mold_f32_minmax_final_kernel"])
    out, k_scaled = [], 0
    for gi, (C, scaled) in enumerate(KERNEL_GROUPS):
        side = KERNEL_CANVAS // 2 if scaled else KERNEL_CANVAS
        src_bytes, out_bytes = 4 * side * side * C, 4 * KERNEL_CANVAS * KERNEL_CANVAS * C
        dur = per["mold_f32_resize_kernel"][gi * per_group + KERNEL_WARM:(gi + 1) * per_group]
        med = float(np.median(dur)) * 1e-9
        row = {"channels": C, "scaled": scaled, "source": [side, side, C], "canvas": [KERNEL_CANVAS, KERNEL_CANVAS, C],
               "pixel_kernel_us": round(1e6 * med, 2), "pixel_kernel_bytes": src_bytes + out_bytes,
               "pixel_kernel_TB_per_s": round((src_bytes + out_bytes) / med / 1e12, 3),
               "pixel_kernel_fraction_of_copy_rate": round((src_bytes + out_bytes) / med / HBM_COPY_RATE, 3)}
        if scaled:
            for key, name in (("minmax_partial", "mold_f32_minmax_partial_kernel"), ("minmax_final", "mold_f32_minmax_final_kernel")):
                dur = per[name][k_scaled * per_group + KERNEL_WARM:(k_scaled + 1) * per_group]
                row[key + "_us"] = round(1e6 * float(np.median(dur)) * 1e-9, 2)
            med = float(np.median(per["mold_f32_minmax_partial_kernel"][k_scaled * per_group + KERNEL_WARM:(k_scaled + 1) * per_group])) * 1e-9
            row["minmax_partial_TB_per_s"] = round(src_bytes / med / 1e12, 3)
            row["minmax_partial_fraction_of_copy_rate"] = round(src_bytes / med / HBM_COPY_RATE, 3)
            k_scaled += 1
        out.append(row)
    return out


def train_steps(C, dev, steps=10):
    import torch
    from caesar_mrcnn_amd.config import run_py_config
    from caesar_mrcnn_amd.model import MaskRCNN
    cfg = run_py_config(num_classes=4, imgsize=256, backbone="resnet101", images_per_gpu=4)
    cfg.IMAGE_CHANNEL_COUNT, cfg.IMAGE_SHAPE = C, np.array([256, 256, C])
    cfg.MEAN_PIXEL = 0 if C == 1 else np.zeros(3)
    cfg.TRAIN_LAUNCH_TAPE = False
    model = MaskRCNN("training", cfg, "/tmp/mrcnn_logs", device=dev, seed=1)
    rng = np.random.RandomState(0)
    B, S, G = 4, 256, 8
    images = rng.normal(20, 8, (B, S, S, C)).astype(np.float32)
    gt_boxes = np.zeros((B, G, 4), np.int32)
    gt_cls = np.zeros((B, G), np.int32)
    gt_masks = np.zeros((B, S, S, G), bool)
    for b in range(B):
        for g in range(G):
            y, x, h, w = rng.randint(8, S - 72), rng.randint(8, S - 72), rng.randint(12, 64), rng.randint(12, 64)
            gt_boxes[b, g], gt_cls[b, g] = (y, x, y + h, x + w), rng.randint(1, 4)
            gt_masks[b, y:y + h, x:x + w, g] = True
            images[b, y:y + h, x:x + w] += 100
    meta = np.stack([np.array([b, S, S, C, S, S, C, 0, 0, S, S, 1.0] + [1] * cfg.NUM_CLASSES) for b in range(B)])
    inputs = [images, meta, None, None, gt_cls, gt_boxes, gt_masks]
    model.compile(0.001, 0.9)
    for _ in range(steps):
        model.train_on_batch(inputs)
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256,1024")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--kernel-trace", default=None)
    ap.add_argument("--train-steps", type=int, default=0, metavar="CHANNELS")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gray_float_bench.json"))
    args = ap.parse_args()
    res = json.load(open(args.out)) if os.path.exists(args.out) else {}
    if args.kernel_trace:
        res["kernels"] = {"copy_rate_TB_per_s": HBM_COPY_RATE / 1e12, "timed_launches": KERNEL_TIMED, "groups": read_trace(args.kernel_trace)}
    else:
        import torch
        assert torch.cuda.is_available(), "needs a GPU: a CPU run gives no time"
        dev = torch.device("cuda:0")
        if args.kernels_only:
            issue_kernels(dev)
            return
        if args.train_steps:
            train_steps(args.train_steps, dev)
            return
        res["device"] = torch.cuda.get_device_name(0)
        res["reps"] = args.reps
        res["mold"] = bench_mold([int(v) for v in args.sizes.split(",")], args.reps, dev)
    line = json.dumps(res, indent=1, sort_keys=True)
    print(line)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
