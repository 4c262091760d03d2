"""Training samples assembled on the host against on the GPU (data_generator(device_samples=...)), measured in
one process, the two paths alternating, median of 5; prints one JSON object.

    python tools/loader_bench.py [--steps 60] [--reps 5] [--out FILE]
        loader:     samples/s of the generators alone (nothing consumes the batches; the device path's last event is waited for):
                    in-memory 256 x 256 images with 4, 30 and 300 box instances, with and without ReferenceAugmenter (warps on
                    the GPU on both paths), 1 and 2 generator threads, device targets as in MaskRCNN.train;
        train_loop: images/s of MaskRCNN.train()'s own iteration in the configuration of profiles/augment_bench.json (synthetic
                    FITS tiles, ResNet-101, 4 images per step, 2 loader threads, ReferenceAugmenter, launch tape);
        pcie:       bytes that cross PCIe per image on either path, counted from the shapes (not timed).
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


def loader_only(dev, reps, nimg=4):
    from caesar_mrcnn_amd.augment import ReferenceAugmenter
    from caesar_mrcnn_amd.config import run_py_config
    from caesar_mrcnn_amd.datagen import data_generator
    cfg = run_py_config(num_classes=4, imgsize=SIZE, backbone="resnet101", images_per_gpu=nimg, gpu_count=1)
    out = {}
    for instances in (4, 30, 300):
        ds = InMemory(instances)
        batches = 8 if instances < 300 else 4
        for augmented in (False, True):
            for threads in (1, 2):
                times = {"host": [], "device": []}
                for rep in range(reps + 1):                                  # rep 0 warms both paths up
                    for path in ("host", "device"):
                        aug = ReferenceAugmenter(seed=rep, device=dev) if augmented else None
                        kw = dict(device_samples=True, device=dev) if path == "device" else {}
                        gens = [data_generator(ds, cfg, shuffle=True, batch_size=nimg, seed=10 * rep + k, device_targets=True,
                                               augmentation=aug, **kw) for k in range(threads)]
                        dt = _drain(gens, batches)
                        if rep:
                            times[path].append(nimg * batches * threads / dt)
                key = "N%d_%s_%dthr" % (instances, "aug" if augmented else "noaug", threads)
                out[key] = {"host_samples_per_s": round(float(np.median(times["host"])), 1),
                            "device_samples_per_s": round(float(np.median(times["device"])), 1)}
                out[key]["device_over_host"] = round(out[key]["device_samples_per_s"] / out[key]["host_samples_per_s"], 3)
                sys.stderr.write("[loader_bench] %s %r\n" % (key, out[key]))
    out["what"] = ("generators alone, %d x %d x 3 uint8 in memory, %d images per batch, device targets; host = the default path "
                   "(ReferenceAugmenter warps on the GPU, everything else NumPy; the consumer's packbits / uploads are NOT in it); "
                   "median of %d alternating repetitions" % (SIZE, SIZE, nimg, reps))
    return out


def train_loop(dev, steps, reps, nimg=4, threads=2):
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
    ds = bench.synthetic_fits_dataset(cfg, 32, "/tmp/mrcnn_loaderbench_data", seed=1234)
    cfg.DEVICE_RPN_TARGETS = True
    ds.device = model.engine.dev                      # FITS -> uint8 RGB on the GPU, as MaskRCNN.train sets it up
    rates = {"host": [], "device": []}
    waits = {"host": [], "device": []}
    built = dict(gtprep.counters)
    for rep in range(reps + 1):                       # rep 0 warms up (and records the launch tape)
        for path in ("host", "device"):
            aug = augment.ReferenceAugmenter(seed=rep, device=dev)
            kw = dict(device_samples=True, device=model.engine.dev) if path == "device" else {}
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
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("loader_bench needs a GPU")
    dev = torch.device("cuda:0")
    res = {"pcie": pcie_bytes(), "loader": loader_only(dev, args.reps)}
    if not args.skip_train_loop:
        res["train_loop"] = train_loop(dev, args.steps, args.reps)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
