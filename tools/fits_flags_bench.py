"""fits.read_fits for every flag combination the device chain takes: host branch against device branch, and the
pixel kernels of csrc/fits.hip per output kind.  Writes one JSON object with --out (default profiles/fits_flags_bench.json).

    python tools/fits_flags_bench.py [--sizes 256,2048] [--reps 5] [--out FILE]
    rocprofv3 --kernel-trace --output-format csv -d <dir> -- python tools/fits_flags_bench.py --kernels-only
    python tools/fits_flags_bench.py --kernel-trace <dir>/.../<pid>_kernel_trace.csv [--sfinder-tiles FILE] [--out FILE]

  read_fits   end to end (file read, header parse, cut, numeric chain; the device branch with its upload and download), per
              (stretch, stretch_biascontrast, normalize, output) and tile size: perf_counter with the device synchronised before
              and after, host and device alternating within every repetition, median of --reps.  Equal contrasts (0.25), bias
              0.5, contrast 1; the run.py flags once more with three distinct contrasts (0.1, 0.25, 0.6).  `host_over_device`
              > 1: the device branch is ahead.
  kernels     --kernels-only issues, on one 2048 x 2048 tile, groups of launches of mrcnn_fits_to_image per output kind; under
              rocprofv3 the trace holds every launch, and --kernel-trace reads the pixel kernels' rows back in issue order:
              median duration of the timed launches of each group, bytes moved (4 read + 3 / 12 / 4 written per pixel) per
              second and its fraction of the 6.3 TB/s copy rate of the card.
  --sfinder-tiles   the JSON of `tools/sfinder_tiles_bench.py --bias-contrast ...`, stored under "sfinder_tiles_bias_contrast".
The second and third form add to the file the first one wrote."""
import argparse
import csv
import itertools
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_COPY_RATE = 6.3e12                    # bytes / s, the copy rate the other sections compare with
KERNEL_SIZE = 2048
KERNEL_WARM, KERNEL_TIMED = 3, 10
OUT_BYTES = {0: 3, 1: 12, 2: 4}
EQUAL_CONTRASTS, DISTINCT_CONTRASTS = (0.25, 0.25, 0.25), (0.1, 0.25, 0.6)
# (label, zscale, biascontrast, normalize, out_kind, contrasts)
KERNEL_GROUPS = [
    ("uint8 RGB, zscale, equal contrasts", True, False, True, 0, (0.25, 0.25, 0.25)),
    ("uint8 RGB, zscale, three contrasts", True, False, True, 0, (0.1, 0.25, 0.6)),
    ("uint8 RGB, zscale + bias/contrast, three contrasts", True, True, True, 0, (0.1, 0.25, 0.6)),
    ("uint8 RGB, bias/contrast alone", False, True, True, 0, (0.25, 0.25, 0.25)),
    ("float32 RGB, zscale + bias/contrast, three contrasts", True, True, True, 1, (0.1, 0.25, 0.6)),
    ("float32 RGB, no stretch", False, False, True, 1, (0.25, 0.25, 0.25)),
    ("gray, zscale + bias/contrast, normalised", True, True, True, 2, (0.25, 0.25, 0.25)),
    ("gray, normalised, no stretch", False, False, True, 2, (0.25, 0.25, 0.25)),
]


def synth_tile(size, seed=3):
    """[size, size] float32: unit noise around zero, a Gaussian blob per 128 x 128 cell, about 1 % NaN."""
    rng = np.random.RandomState(seed)
    img = rng.normal(0.0, 1.0, (size, size)).astype(np.float32)
    r = 16
    yy, xx = np.mgrid[-r:r + 1, -r:r + 1]
    for _ in range(max(1, (size // 128) ** 2)):
        cy, cx = rng.randint(r, size - r, 2)
        img[cy - r:cy + r + 1, cx - r:cx + r + 1] += (rng.uniform(10.0, 200.0) * np.exp(-0.5 * (yy ** 2 + xx ** 2) / rng.uniform(4.0, 30.0))).astype(np.float32)
    img[rng.uniform(size=img.shape) < 0.01] = np.nan
    return img


def flag_kwargs(stretch, bc, normalize, out_kind):
    return dict(stretch=stretch, stretch_biascontrast=bc, normalize=normalize, convertToRGB=out_kind != 2, to_uint8=out_kind == 0,
                bias=0.5, contrast=1)


def bench_read_fits(args, res):
    import warnings
    import torch
    from caesar_mrcnn_amd import fits
    dev = torch.device("cuda:0")
    fits.DEVICE_LIGHT_CHAIN_MIN_PIXELS = 0      # measure the device branch at every size: that threshold comes from these rows
    tmp = tempfile.mkdtemp(prefix="fits_flags_bench_")
    rows = []
    for size in [int(v) for v in args.sizes.split(",")]:
        path = os.path.join(tmp, "tile_%d.fits" % size)
        fits.write_fits(path, synth_tile(size))
        combos = [c + (EQUAL_CONTRASTS,) for c in itertools.product((False, True), (False, True), (False, True), (0, 1, 2))]
        combos.append((True, False, True, 0, DISTINCT_CONTRASTS))      # the run.py flags, no channel shared
        for stretch, bc, normalize, out_kind, zc in combos:
            kw = dict(flag_kwargs(stretch, bc, normalize, out_kind), zscale_contrasts=list(zc))
            chain, why = fits.device_chain(stretch, normalize, kw["convertToRGB"], kw["to_uint8"], bc, zc, 1, 0.5)
            row = {"size": size, "stretch": stretch, "stretch_biascontrast": bc, "normalize": normalize,
                   "output": ("uint8_rgb", "float32_rgb", "float32_gray")[out_kind], "zscale_contrasts": list(zc)}
            if chain is None:
                row["refused"] = why
                rows.append(row)
                continue
            t = {"host": [], "device": []}
            with warnings.catch_warnings(), np.errstate(all="ignore"):
                warnings.simplefilter("ignore")
                for rep in range(args.reps + 1):                        # the first repetition warms both
                    for which in ("host", "device"):
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        fits.read_fits(path, device=dev if which == "device" else None, **kw)
                        torch.cuda.synchronize()
                        if rep:
                            t[which].append(time.perf_counter() - t0)
            h, d = float(np.median(t["host"])), float(np.median(t["device"]))
            row.update(host_ms=round(1e3 * h, 3), device_ms=round(1e3 * d, 3), host_over_device=round(h / d, 2))
            rows.append(row)
            sys.stderr.write("%s\n" % json.dumps(row))
        os.remove(path)
    res["read_fits"] = {"reps": args.reps, "bias": 0.5, "contrast": 1, "rows": rows}


def kernels_only():
    import torch
    from caesar_mrcnn_amd import fits, ops
    dev = torch.device("cuda:0")
    raw = torch.from_numpy(synth_tile(KERNEL_SIZE)).to(dev)
    for _, zscale, bc, normalize, out_kind, zc in KERNEL_GROUPS:
        for _ in range(KERNEL_WARM + KERNEL_TIMED):
            ops.fits_to_image(raw, KERNEL_SIZE, KERNEL_SIZE, fits.DeviceChain(zscale, bc, normalize, out_kind, zc, 0.5, 1.0))
            torch.cuda.synchronize()


def read_kernel_trace(path, res):
    with open(path) as f:
        rows = [r for r in csv.DictReader(f) if "fits_image_kernel" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    per = KERNEL_WARM + KERNEL_TIMED
    assert len(rows) == per * len(KERNEL_GROUPS), "%d pixel-kernel launches in the trace, %d expected" % (len(rows), per * len(KERNEL_GROUPS))
    n = KERNEL_SIZE * KERNEL_SIZE
    out = []
    for k, (label, zscale, bc, normalize, out_kind, zc) in enumerate(KERNEL_GROUPS):
        group = rows[k * per + KERNEL_WARM:(k + 1) * per]
        names = set(r["Kernel_Name"] for r in group)
        assert len(names) == 1, (label, names)
        us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in group]
        nbytes = n * (4 + OUT_BYTES[out_kind])
        med = float(np.median(us))
        out.append({"group": label, "kernel": list(names)[0].split("(")[0], "launches": len(us), "median_us": round(med, 2),
                    "min_us": round(min(us), 2), "max_us": round(max(us), 2), "bytes": nbytes,
                    "tb_per_s": round(nbytes / (med * 1e-6) / 1e12, 3), "fraction_of_copy_rate": round(nbytes / (med * 1e-6) / HBM_COPY_RATE, 3)})
    res["kernels"] = {"tile": [KERNEL_SIZE, KERNEL_SIZE], "copy_rate_tb_per_s": HBM_COPY_RATE / 1e12, "bias": 0.5, "contrast": 1.0,
                      "timed_launches_per_group": KERNEL_TIMED, "groups": out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256,2048")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--kernels-only", action="store_true", help="issue the pixel-kernel groups and exit (run under rocprofv3)")
    ap.add_argument("--kernel-trace", default=None, help="kernel trace (csv) of a --kernels-only run: add the kernel table to --out")
    ap.add_argument("--sfinder-tiles", default=None, help="JSON of tools/sfinder_tiles_bench.py --bias-contrast: add it to --out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fits_flags_bench.json"))
    args = ap.parse_args()
    if args.kernels_only:
        return kernels_only()
    if args.kernel_trace or args.sfinder_tiles:
        with open(args.out) as f:
            res = json.loads(f.read())
        if args.kernel_trace:
            read_kernel_trace(args.kernel_trace, res)
        if args.sfinder_tiles:
            with open(args.sfinder_tiles) as f:
                res["sfinder_tiles_bias_contrast"] = json.loads(f.read())
    else:
        import torch
        assert torch.cuda.is_available(), "needs a GPU: a CPU run gives no time"
        res = {"device": torch.cuda.get_device_name(0)}
        bench_read_fits(args, res)
    line = json.dumps(res)
    print(line)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
