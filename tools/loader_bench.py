"""Training samples assembled on the host against on the GPU (data_generator(device_samples=...)), measured in
one process, the two paths alternating, median of 5; prints one JSON object.

    python tools/loader_bench.py [--steps 60] [--reps 5] [--out FILE]
        loader:     samples/s of the generators alone (nothing consumes the batches; the device path's last event is waited for):
                    in-memory 256 x 256 images with 4, 30 and 300 box instances, with and without ReferenceAugmenter (warps on
                    the GPU on both paths), 1 and 2 generator threads, device targets as in MaskRCNN.train;
        train_loop: images/s of MaskRCNN.train()'s own iteration in the configuration of profiles/augment_bench.json (synthetic
                    FITS tiles, ResNet-101, 4 images per step, 2 loader threads, ReferenceAugmenter, launch tape);
        pcie:       bytes that cross PCIe per image on either path, counted from the shapes (not timed).

    python tools/loader_bench.py --scaled [--steps 30] [--reps 5] [--out profiles/loader_bench_scaled.json]
        the same three figures on cut-outs the loader has to scale: sides drawn once, with a fixed seed, from
        40 ... 400 pixels at imgsize 256, so both up- and down-scaling occur; three paths alternate: host / device_samples alone
        (every scaled sample is handed to the host and uploaded) / device_samples with device_resize.  The train loop feeds from
        the in-memory cut-outs with 30 instances.
"""
import argparse
import contextlib
import json
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZE = 256


class InMemory(object):
    """A dataset as load_image_gt uses it: `n` images of SIZE x SIZE with `instances` box masks each, made once."""

    def __init__(self, instances, n=16):
        self.image_ids = np.arange(n)
        self.image_info = [{"source": "bench", "id": i} for i in range(n)]
        self.num_classes = 4
        self.source_class_ids = {"bench": [0, 1, 2, 3]}
        self.items = []
        for i in range(n):
            r = np.random.RandomState(i)
            img = r.randint(0, 40, (SIZE, SIZE, 3)).astype(np.uint8)
            mask = np.zeros((SIZE, SIZE, instances), bool)
            for g in range(instances):
                y, x = r.randint(0, SIZE - 40, 2)
                h, w = r.randint(4, 40, 2)
                mask[y:y + h, x:x + w, g] = True
            self.items.append((img, mask, r.randint(1, 4, instances).astype(np.int32)))

    def load_image(self, i):
        return self.items[i][0]

    def load_mask(self, i):
        return self.items[i][1], self.items[i][2]


SCALED_SIDES = (40, 400)          # --scaled: both sides of a cut-out are drawn from this range (inclusive), once, seed 2024


def scaled_sizes(n=16):
    return [tuple(int(v) for v in hw) for hw in np.random.RandomState(2024).randint(SCALED_SIDES[0], SCALED_SIDES[1] + 1, (n, 2))]


class ScaledInMemory(InMemory):
    """`n` cut-outs of scaled_sizes(n) with `instances` box masks each (sides a seventh of the cut-out's at most), made once:
    IMAGE_MIN_DIM = IMAGE_MAX_DIM = SIZE scales every one of them, up or down."""

    def __init__(self, instances, n=16):
        InMemory.__init__(self, 0, n)
        self.items = []
        for i, (H, W) in enumerate(scaled_sizes(n)):
            r = np.random.RandomState(i)
            img = r.randint(0, 40, (H, W, 3)).astype(np.uint8)
            mask = np.zeros((H, W, instances), bool)
            for g in range(instances):
                y, x = r.randint(0, H - H // 7), r.randint(0, W - W // 7)
                h, w = r.randint(2, max(3, H // 7)), r.randint(2, max(3, W // 7))
                mask[y:y + h, x:x + w, g] = True
            self.items.append((img, mask, r.randint(1, 4, instances).astype(np.int32)))


PATHS = {"host": {}, "device": dict(device_samples=True), "device_resize": dict(device_samples=True, device_resize=True)}


def _drain(gens, batches):
    """Every generator yields `batches` batches on its own thread; returns the wall time."""
    import torch
    last = [None] * len(gens)

    def work(k):
        for _ in range(batches):
            last[k] = next(gens[k])[0]
    threads = [threading.Thread(target=work, args=(k,)) for k in range(len(gens))]
    t0 = time.perf_counter()
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for b in last:
        if getattr(b, "ready", None) is not None:
            b.ready.synchronize()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def loader_only(dev, reps, nimg=4, scaled=False):
    from caesar_mrcnn_amd.augment import ReferenceAugmenter
    from caesar_mrcnn_amd.config import run_py_config
    from caesar_mrcnn_amd.datagen import data_generator
    cfg = run_py_config(num_classes=4, imgsize=SIZE, backbone="resnet101", images_per_gpu=nimg, gpu_count=1)
    paths = ("host", "device", "device_resize") if scaled else ("host", "device")
    out = {}
    for instances in (4, 30, 300):
        ds = ScaledInMemory(instances) if scaled else InMemory(instances)
        batches = (4 if instances < 300 else 2) if scaled else (8 if instances < 300 else 4)
        for augmented in (False, True):
            for threads in (1, 2):
                times = {p: [] for p in paths}
                for rep in range(reps + 1):                                  # rep 0 warms every path up
                    for path in paths:
                        aug = ReferenceAugmenter(seed=rep, device=dev) if augmented else None
                        kw = dict(PATHS[path], device=dev) if path != "host" else {}
                        gens = [data_generator(ds, cfg, shuffle=True, batch_size=nimg, seed=10 * rep + k, device_targets=True,
                                               augmentation=aug, **kw) for k in range(threads)]
                        dt = _drain(gens, batches)
                        if rep:
                            times[path].append(nimg * batches * threads / dt)
                key = "N%d_%s_%dthr" % (instances, "aug" if augmented else "noaug", threads)
                out[key] = {"host_samples_per_s": round(float(np.median(times["host"])), 1),
                            "device_samples_per_s": round(float(np.median(times["device"])), 1)}
                out[key]["device_over_host"] = round(out[key]["device_samples_per_s"] / out[key]["host_samples_per_s"], 3)
                if scaled:
                    out[key]["device_resize_samples_per_s"] = round(float(np.median(times["device_resize"])), 1)
                    out[key]["device_resize_over_host"] = round(out[key]["device_resize_samples_per_s"] / out[key]["host_samples_per_s"], 3)
                sys.stderr.write("[loader_bench] %s %r\n" % (key, out[key]))
    out["what"] = ("generators alone, %s uint8 in memory, %d images per batch, device targets; host = the default path "
                   "(ReferenceAugmenter warps on the GPU, everything else NumPy; the consumer's packbits / uploads are NOT in it); "
                   "median of %d alternating repetitions"
                   % ("cut-outs of %r (h, w) scaled to %d" % (scaled_sizes(), SIZE) if scaled else "%d x %d x 3" % (SIZE, SIZE), nimg, reps))
    return out


def train_loop(dev, steps, reps, nimg=4, threads=2, scaled=False):
    import torch
    import bench
    from caesar_mrcnn_amd import augment, gtprep
    from caesar_mrcnn_amd.config import run_py_config
    from caesar_mrcnn_amd.datagen import Prefetcher, data_generator
    from caesar_mrcnn_amd.model import MaskRCNN
    cfg = run_py_config(num_classes=4, imgsize=SIZE, backbone="resnet101", images_per_gpu=nimg, gpu_count=1)
    with contextlib.redirect_stdout(sys.stderr):
        model = MaskRCNN("training", cfg, "/tmp/mrcnn_loaderbench_logs", device=dev, seed=0)
        model.compile(cfg.LEARNING_RATE, cfg.LEARNING_MOMENTUM)
    cfg.DEVICE_RPN_TARGETS = True
    if scaled:
        ds = ScaledInMemory(30, n=32)
    else:
        ds = bench.synthetic_fits_dataset(cfg, 32, "/tmp/mrcnn_loaderbench_data", seed=1234)
        ds.device = model.engine.dev                  # FITS -> uint8 RGB on the GPU, as MaskRCNN.train sets it up
    paths = ("host", "device", "device_resize") if scaled else ("host", "device")
    rates = {p: [] for p in paths}
    waits = {p: [] for p in paths}
    built = dict(gtprep.counters)
    for rep in range(reps + 1):                       # rep 0 warms up (and records the launch tape)
        for path in paths:
            aug = augment.ReferenceAugmenter(seed=rep, device=dev)
            kw = dict(PATHS[path], device=model.engine.dev) if path != "host" else {}
            gen = Prefetcher([data_generator(ds, cfg, shuffle=True, batch_size=nimg, seed=99 + 1000 * k + rep, device_targets=True,
                                             augmentation=aug, **kw) for k in range(threads)], depth=2 * threads + 2)
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
            if rep:
                rates[path].append(nimg * steps / dt)
                waits[path].append(1e3 * wait / steps)
    out = {p: {"images_per_s": round(float(np.median(rates[p])), 2), "images_per_s_all": [round(v, 2) for v in rates[p]],
               "ms_per_step_waiting_for_loader": round(float(np.median(waits[p])), 3)} for p in rates}
    out["device_over_host"] = round(out["device"]["images_per_s"] / out["host"]["images_per_s"], 4)
    out["device_samples_built"] = gtprep.counters["device"] - built["device"]
    out["host_fallbacks"] = gtprep.counters["host"] - built["host"]
    out.update(steps=steps, repetitions=reps, images_per_step=nimg, loader_threads=threads, backbone="resnet101", imgsize=SIZE,
               what="feed-inclusive loop of MaskRCNN.train() (bench.py train_loop leg: synthetic FITS tiles, DEVICE_FITS, device "
                    "targets, launch tape, ReferenceAugmenter on the GPU), host-assembled against device-assembled samples, "
                    "alternating, median")
    if scaled:
        out["device_resize_over_host"] = round(out["device_resize"]["images_per_s"] / out["host"]["images_per_s"], 4)
        out["device_samples_scaled"] = gtprep.counters["scaled"] - built["scaled"]
        out["what"] = ("feed-inclusive loop of MaskRCNN.train() (device targets, launch tape, ReferenceAugmenter on the GPU) fed from "
                       "32 in-memory uint8 cut-outs of 40 ... 400 pixels a side with 30 instances, every one scaled to %d: host "
                       "loader / device_samples alone (every sample handed to the host) / with device_resize, alternating, median"
                       % SIZE)
    return out


def pcie_bytes_scaled(batch=4):
    """Bytes per image across PCIe for the --scaled cut-outs (uint8 in memory, no FITS), the mean over scaled_sizes(), counted
    from the shapes: N instances of which all are kept, an augmentation plan that warps.  Host: image + packed masks of the
    256 x 256 canvas up and back for the warp, float32 image + packed kept planes up for the step.  device_samples alone: the
    same warp traffic, then the float32 image + packed planes through emit_host.  With device_resize: the cut-out's own uint8
    image and packed masks, the two index tables (first time a size is seen) and the selection table up, the [N, 5] table
    back."""
    H = W = SIZE
    sizes = scaled_sizes()
    out = {}
    for N in (4, 30, 300):
        nb_aug = 4 * -(-N // 32)
        nb_step = -(-N // 8)
        warp = 3 * H * W + H * W * nb_aug
        host_up, host_down = warp + 12 * H * W + H * W * nb_step, warp
        alone_up, alone_down = warp + 12 * H * W + H * W * nb_aug + 4 * N, warp
        rs_up = float(np.mean([3 * h * w + h * w * nb_aug + 4 * (round(h * SIZE / max(h, w)) + round(w * SIZE / max(h, w))) for h, w in sizes])) + 4 * N
        rs_down = 20 * N
        out["N%d" % N] = {"host_total": host_up + host_down, "device_total": alone_up + alone_down,
                          "device_resize_h2d": round(rs_up), "device_resize_d2h": rs_down, "device_resize_total": round(rs_up + rs_down),
                          "device_resize_over_host": round((rs_up + rs_down) / (host_up + host_down), 4)}
    out["what"] = "per cut-out, mean over the sizes %r; see pcie_bytes_scaled" % (sizes,)
    return out


def pcie_bytes(H=SIZE, W=SIZE, batch=4):
    """Bytes per image across PCIe, counted from the shapes: a FITS tile of float32, N instances of which all are kept, an
    augmentation plan that warps (2 of 3 plans do).  Host path: data_generator + MaskRCNN._to_device as they are by default
    (DEVICE_FITS, ReferenceAugmenter on the GPU, device targets); device path: device_samples."""
    out = {}
    for N in (4, 30, 300):
        nb_aug = 4 * -(-N // 32)                       # the augmenter pads the packed masks to whole words
        nb_step = -(-N // 8)                           # _to_device packs the used planes
        host_up = 4 * H * W + (3 * H * W + H * W * nb_aug) + (12 * H * W + H * W * nb_step)
        host_down = 3 * H * W + (3 * H * W + H * W * nb_aug)
        dev_up = 4 * H * W + H * W * nb_aug + 4 * N
        dev_down = 20 * N
        out["N%d" % N] = {"host_h2d": host_up, "host_d2h": host_down, "device_h2d": dev_up, "device_d2h": dev_down,
                          "host_total": host_up + host_down, "device_total": dev_up + dev_down,
                          "device_over_host": round((dev_up + dev_down) / (host_up + host_down), 4)}
    out["what"] = ("per %d x %d image: host = FITS floats up, uint8 image back, image + packed masks up and back for the warp, "
                   "float32 image + packed kept planes up for the step; device = FITS floats, packed masks and the selection "
                   "table up, the [N, 5] int32 table back" % (H, W))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-train-loop", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--scaled", action="store_true", help="cut-outs the loader has to scale, three paths (DESIGN.md 4.19)")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("loader_bench needs a GPU")
    dev = torch.device("cuda:0")
    res = {"pcie": pcie_bytes_scaled() if args.scaled else pcie_bytes(), "loader": loader_only(dev, args.reps, scaled=args.scaled)}
    if not args.skip_train_loop:
        res["train_loop"] = train_loop(dev, args.steps, args.reps, scaled=args.scaled)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
