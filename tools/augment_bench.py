"""The reference's training augmentation (caesar_mrcnn_amd.augment) measured on the GPU; prints one JSON object.

    python tools/augment_bench.py [--steps 40] [--out FILE]
        apply: wall time of one ReferenceAugmenter.apply on the device (uploads, warps, copies back, loader-stream
               synchronise, unpack) and of the host statement, 256 x 256 x 3 with N = 8, 32 and 300 masks, one rotate +
               translate plan;
        train_loop: MaskRCNN.train()'s own iteration (bench.py's train_loop leg: synthetic FITS tiles, data_generator(...,
               device_targets=True), Prefetcher, launch tape, product-default step) without augmentation, with the host
               statement (device=None) and with the device path: images/s and the mean wait for the loader per step.
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/augment_bench.py --kernels-only
        the two warp kernels alone, 200 launches per (stage, shape); then
    python tools/augment_bench.py --trace-report DIR/.../*_kernel_trace.csv
        the per-stage kernel time from that trace (the stats table merges the mask shapes: one kernel name).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PLAN = [("rotate", 23.7), ("translate", 0.17, -0.11)]


def _masks(H, W, N, seed):
    rng = np.random.RandomState(seed)
    mk = np.zeros((H, W, N), bool)
    for j in range(N):
        y, x = rng.randint(0, H - 40), rng.randint(0, W - 40)
        h, w = rng.randint(4, 40, 2)
        mk[y:y + h, x:x + w, j] = True
    return mk


def kernels_only(dev, reps=200):
    import torch
    from caesar_mrcnn_amd import augment, ops
    H, W = 256, 256
    img = torch.from_numpy(np.random.RandomState(0).randint(0, 256, (H, W, 3)).astype(np.uint8)).to(dev)
    mats = augment.ReferenceAugmenter.matrices(PLAN, H, W)
    out = torch.empty_like(img)
    for _ in range(reps):
        for m in mats:
            ops.augment_warp_u8(img, m, out=out)
    for N in (8, 32, 300):
        p = np.packbits(_masks(H, W, N, N), axis=-1, bitorder="little")
        p = np.concatenate([p, np.zeros((H, W, -p.shape[2] % 4), np.uint8)], axis=2)
        pd = torch.from_numpy(p).to(dev)
        o = torch.empty_like(pd)
        for _ in range(reps):
            for m in mats:
                ops.augment_warp_mask_bits(pd, m, out=o)
    torch.cuda.synchronize()
    return {"launches": reps * len(mats) * 4, "plan": PLAN}


def trace_report(path, reps=200, skip=10):
    """Per-stage kernel time from the kernel trace of a --kernels-only run: its launches come in blocks of 2 * reps (image, then
    masks with N = 8, 32, 300), alternating rotate / translate."""
    import csv
    rows = [r for r in csv.DictReader(open(path)) if "augment_warp" in r.get("Kernel_Name", "")]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    dur = np.array([int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in rows], dtype=np.float64) * 1e-3   # us
    out = {}
    for b, what in enumerate(("image_u8_256x256x3", "masks_N8", "masks_N32", "masks_N300")):
        block = dur[b * 2 * reps:(b + 1) * 2 * reps]
        for k, stage in enumerate(("rotate", "translate")):
            d = block[k::2][skip:]
            out["%s_%s" % (what, stage)] = {"us_mean": round(float(d.mean()), 2), "us_median": round(float(np.median(d)), 2),
                                             "us_min": round(float(d.min()), 2), "launches": int(d.size)}
    out["kernels"] = sorted({r["Kernel_Name"] for r in rows})
    return out


def apply_times(dev, reps=50):
    from caesar_mrcnn_amd import augment
    H, W = 256, 256
    img = np.random.RandomState(0).randint(0, 256, (H, W, 3)).astype(np.uint8)
    dev_aug, host_aug = augment.ReferenceAugmenter(device=dev), augment.ReferenceAugmenter()
    res = {}
    for N in (8, 32, 300):
        mk = _masks(H, W, N, N)
        for _ in range(5):
            gi, gm = dev_aug.apply(img, mk, PLAN)
        t = []
        for _ in range(reps):
            t0 = time.perf_counter()
            gi, gm = dev_aug.apply(img, mk, PLAN)
            t.append(time.perf_counter() - t0)
        h = []
        for _ in range(max(3, reps // 10)):
            t0 = time.perf_counter()
            wi, wm = host_aug.apply(img, mk, PLAN)
            h.append(time.perf_counter() - t0)
        assert np.array_equal(gi, wi) and np.array_equal(gm, wm), "device and host statement differ"
        res["N%d" % N] = {"device_ms_median": round(1e3 * float(np.median(t)), 3), "device_ms_p90": round(1e3 * float(np.percentile(t, 90)), 3),
                          "host_ms_median": round(1e3 * float(np.median(h)), 3), "identical": True}
    return res


def train_loop(dev, steps, nimg=4, threads=2):
    import torch
    import bench
    from caesar_mrcnn_amd import augment
    from caesar_mrcnn_amd.config import run_py_config
    from caesar_mrcnn_amd.datagen import Prefetcher, data_generator
    from caesar_mrcnn_amd.model import MaskRCNN
    cfg = run_py_config(num_classes=4, imgsize=256, backbone="resnet101", images_per_gpu=nimg, gpu_count=1)
    import contextlib
    with contextlib.redirect_stdout(sys.stderr):
        model = MaskRCNN("training", cfg, "/tmp/mrcnn_augbench_logs", device=dev, seed=0)
        model.compile(cfg.LEARNING_RATE, cfg.LEARNING_MOMENTUM)
    ds = bench.synthetic_fits_dataset(cfg, 32, "/tmp/mrcnn_augbench_data", seed=1234)
    cfg.DEVICE_RPN_TARGETS = True
    ds.device = model.engine.dev                      # FITS -> uint8 RGB on the GPU, as MaskRCNN.train sets it up
    legs = {"none": None, "host": augment.ReferenceAugmenter(seed=0), "device": augment.ReferenceAugmenter(seed=0, device=dev)}
    out = {}
    for name in ("none", "host", "device", "none_again"):
        aug = legs[name.split("_")[0]]
        gen = Prefetcher([data_generator(ds, cfg, shuffle=True, batch_size=nimg, seed=99 + 1000 * k, device_targets=True,
                                         augmentation=aug) for k in range(threads)], depth=2 * threads + 2)
        try:
            t_fill = time.time()
            while gen._q.qsize() < 2 * threads + 2 and time.time() - t_fill < 10.0:
                time.sleep(0.01)
            for _ in range(3):
                model.train_on_batch(next(gen)[0])
            torch.cuda.synchronize()
            t0, wait = time.time(), 0.0
            for _ in range(steps):
                t1 = time.time()
                inputs, _ = next(gen)
                wait += time.time() - t1
                model.train_on_batch(inputs)
            torch.cuda.synchronize()
            dt = time.time() - t0
        finally:
            gen.close()
        out[name] = {"images_per_s": round(nimg * steps / dt, 2), "ms_per_step": round(1e3 * dt / steps, 3),
                     "ms_per_step_waiting_for_loader": round(1e3 * wait / steps, 3),
                     "device_calls": None if aug is None else aug.device_calls}
    base = 0.5 * (out["none"]["images_per_s"] + out["none_again"]["images_per_s"])
    for name in ("host", "device"):
        out[name]["fraction_of_unaugmented"] = round(out[name]["images_per_s"] / base, 4)
    out.update(steps=steps, images_per_step=nimg, loader_threads=threads, backbone="resnet101", imgsize=256,
               what="feed-inclusive loop of MaskRCNN.train() (bench.py train_loop leg), product-default step; none_again = the "
                    "unaugmented leg repeated after the others (drift)")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--threads", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-report", metavar="KERNEL_TRACE_CSV", default=None)
    args = ap.parse_args()
    if args.trace_report:
        print(json.dumps(trace_report(args.trace_report), indent=1))
        return
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("augment_bench needs a GPU")
    dev = torch.device("cuda:0")
    if args.kernels_only:
        res = {"kernels": kernels_only(dev)}
    else:
        res = {"apply": apply_times(dev), "train_loop": train_loop(dev, args.steps, threads=args.threads)}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
