"""Analyzer.draw_results, host statement (draw.render_host: NumPy passes over the canvas per box, mask and character) against the
device form (csrc/draw.hip: one ops.draw_overlay launch per frame), on the same host; prints one JSON object and writes it
(default profiles/draw_bench.json).

    python tools/draw_bench.py [--d 1,10,100] [--sizes 256,512] [--reps 5] [--out FILE]

The frame: D blob-shaped masks (the generator of tools/outline_bench.py) on a size x size frame of seeded noise, one ground-truth
box per mask, score captions, the default scale (3 at 256, 1 at 512), shading off and on.  Per case, on the same Analyzer state,
in the same process, host and device runs alternating, medians of --reps (at least 5) runs after a warm-up, the device
synchronised before every clock reading:
  host       draw.render_host, and the PNG encoding (zlib level 1, the writer's, and level 6, with the file sizes);
  device     render_results(device=True) with the frame's bit planes resident (as extract_det_masks_device leaves them) and once
             more from the host masks (one upload + pack), split as Analyzer.draw_timing splits it: planes / render (tables,
             image upload, launch, synchronise) / download;
  kernel     the device time of 50 back-to-back launches over 50 (events), and the canvas bytes over it as a share of the HBM
             bandwidth of MI355X (8.0 TB/s by specification, 6.29 TB/s measured for a float4 copy).
The two canvases are compared first and nothing is written unless they are equal.  `min_masks_device_ahead`: the smallest D from
which on the device form (planes resident, PNG encoding excluded: it is the same code on both sides) was ahead in every case --
the value of Analyzer.DRAW_DEVICE_MIN_MASKS; 0 when it was ahead throughout.  The reference's matplotlib figure is timed only where
matplotlib can be imported."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

HBM_SPEC_TBS, HBM_COPY_TBS = 8.0, 6.29
KERNEL_LAUNCHES = 50


def med(v):
    return round(float(np.median(v)), 3)


def timed(f, sync=None):
    if sync:
        sync()
    t0 = time.perf_counter()
    out = f()
    if sync:
        sync()
    return 1e3 * (time.perf_counter() - t0), out


def planted(D, size, shaded, seed):
    """An Analyzer holding D final masks as predict would leave them."""
    import outline_bench as OB
    res = OB.blobs(D, size, seed)
    an = OB.analyzer(res)
    rng = np.random.default_rng(seed + 1)
    an.image = rng.integers(0, 256, (size, size, 3)).astype(np.uint8)
    an.masks_final = [np.ascontiguousarray(res["masks"][:, :, i]).astype(np.uint8) for i in range(D)]
    an.class_ids_final = [int(c) for c in res["class_ids"]]
    an.scores_final = [float(s) for s in res["scores"]]
    an.bboxes = [b.astype(np.int32) for b in res["rois"]]
    an.captions = ["{} {:.2f}".format(OB.CLASS_NAMES[c], s) for c, s in zip(an.class_ids_final, an.scores_final)]
    an.bboxes_gt = [np.array([max(b[0] - 2, 0), max(b[1] - 2, 0), min(b[2] + 2, size), min(b[3] + 2, size)]) for b in res["rois"]]
    an.class_ids_gt_merged = list(an.class_ids_final)
    an.draw_shaded_masks = shaded
    return an


def kernel_time(an, planes):
    """Device milliseconds of one render launch: KERNEL_LAUNCHES back-to-back launches between two events."""
    import torch
    from caesar_mrcnn_amd import _hip, draw, ops
    scene = an._draw_scene()
    H, W = scene["image"].shape[:2]
    dev = planes.words.device
    d, items, texts, glyphs, palette, shade = ops._draw_desc(H, W, planes.n, draw.device_tables(scene), scene["scale"])
    host = [a.ctypes.data_as(ctypes.c_void_p) for a in (items, texts, glyphs)]
    up = [torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).to(dev) if a is not None else None for a in (items, texts, glyphs, palette, shade)]
    image = torch.from_numpy(scene["image"]).to(dev)
    Hc, Wc, _ = draw.canvas_shape(H, W, scene["scale"])
    canvas = torch.empty((Hc, Wc, 3), dtype=torch.uint8, device=dev)
    L, stream = _hip.lib(), _hip.current_stream()

    def launch():
        rc = L.mrcnn_draw_overlay(ctypes.byref(d), host[0], host[1], host[2], image.data_ptr(), planes.words.data_ptr(), planes.box.data_ptr(),
                                  up[0].data_ptr(), up[1].data_ptr(), up[2].data_ptr(), up[3].data_ptr(),
                                  up[4].data_ptr() if up[4] is not None else None, canvas.data_ptr(), stream)
        assert rc == 0, rc
    for _ in range(5):
        launch()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    torch.cuda.synchronize()
    ev[0].record()
    for _ in range(KERNEL_LAUNCHES):
        launch()
    ev[1].record()
    ev[1].synchronize()
    return ev[0].elapsed_time(ev[1]) / KERNEL_LAUNCHES, 3 * Hc * Wc, canvas.cpu().numpy()


def matplotlib_figure(an, tmp):
    """The reference-style figure (a 16 x 16 inch canvas, patches and texts, savefig), where matplotlib is there; else None."""
    try:
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
        from matplotlib import patches
    except Exception:
        return None
    scene = an._draw_scene()

    def figure():
        fig, ax = plt.subplots(1, figsize=(16, 16))
        H, W = scene["image"].shape[:2]
        ax.set_ylim(H + 2, -2)
        ax.set_xlim(-2, W + 2)
        ax.axis('off')
        for (y1, x1, y2, x2), c in zip(scene["boxes"], scene["colours"]):
            ax.add_patch(patches.Rectangle((x1, y1), x2 - x1, y2 - y1, linewidth=2, alpha=0.7, edgecolor=c, facecolor='none'))
        for text, xa, ya, _ in scene["texts"]:
            ax.text(xa, ya, text, color="darkturquoise", size=30, backgroundcolor="none")
        ax.imshow(scene["image"])
        fig.savefig(os.path.join(tmp, "figure.png"))
        plt.close(fig)
    figure()
    return med([timed(figure)[0] for _ in range(5)])


def case(D, size, shaded, reps, seed, tmp):
    import torch
    from caesar_mrcnn_amd import draw, ops
    sync = torch.cuda.synchronize
    an = planted(D, size, shaded, seed)
    stack = np.ascontiguousarray(np.stack([m != 0 for m in an.masks_final], axis=-1))
    planes = ops.mask_planes_pack(torch.from_numpy(stack.view(np.uint8)).to(an._device()))

    def device_form(resident):
        an._final_planes = (planes, an.masks_final) if resident else None
        return an.render_results(device=True)
    want = an.render_results(device=False)
    for resident in (True, False):                                         # equality first (and warm-up)
        assert np.array_equal(device_form(resident), want), "canvases differ at D = %d, size %d" % (D, size)
    t_host, t_dev, t_up, stages = [], [], [], []
    for _ in range(reps):                                                  # alternating
        t_host.append(timed(lambda: an.render_results(device=False))[0])
        t_dev.append(timed(lambda: device_form(True), sync)[0])
        stages.append(dict(an.draw_timing))
        t_up.append(timed(lambda: device_form(False), sync)[0])
    k_ms, canvas_bytes, k_canvas = kernel_time(an, planes)
    assert np.array_equal(k_canvas, want)
    enc = {}
    for level in (1, 6):
        path = os.path.join(tmp, "bench_%d.png" % level)
        enc["level_%d_ms" % level] = med([timed(lambda: draw.write_png(path, want, level))[0] for _ in range(reps)])
        enc["level_%d_bytes" % level] = os.path.getsize(path)
    out = {"masks": D, "frame": [size, size], "scale": an._draw_scene()["scale"], "canvas": list(want.shape), "shaded": shaded,
           "identical": True, "runs": reps,
           "render_host_ms": med(t_host), "render_device_ms": med(t_dev), "render_device_with_upload_ms": med(t_up),
           "host_over_device": round(med(t_host) / med(t_dev), 2),
           "device_stages_ms": {k: med([s[k] for s in stages]) for k in ("planes_ms", "render_ms", "download_ms")},
           "png_encode": enc,
           "kernel": {"device_ms": round(k_ms, 5), "launches": KERNEL_LAUNCHES, "canvas_bytes": canvas_bytes,
                      "canvas_gbs": round(canvas_bytes / (k_ms * 1e-3) / 1e9, 1),
                      "share_of_hbm_spec": round(canvas_bytes / (k_ms * 1e-3) / (HBM_SPEC_TBS * 1e12), 4),
                      "share_of_hbm_copy_rate": round(canvas_bytes / (k_ms * 1e-3) / (HBM_COPY_TBS * 1e12), 4)}}
    if D == 10 and not shaded:
        ms = matplotlib_figure(an, tmp)
        out["matplotlib_figure_ms"] = ms if ms is not None else "not measured"
    sys.stderr.write(json.dumps(out) + "\n")
    sys.stderr.flush()
    return out


def main():
    import tempfile
    ap = argparse.ArgumentParser()
    ap.add_argument("--d", default="1,10,100")
    ap.add_argument("--sizes", default="256,512")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "draw_bench.json"))
    args = ap.parse_args()
    assert args.reps >= 5, "medians of at least 5 runs"
    import logging
    logging.getLogger("mrcnn").setLevel(logging.ERROR)
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda", torch.cuda.current_device())
    from caesar_mrcnn_amd import draw
    with tempfile.TemporaryDirectory() as tmp:
        cases = [case(int(d), int(size), shaded, args.reps, args.seed, tmp)
                 for size in args.sizes.split(",") for d in args.d.split(",") for shaded in (False, True)]
    behind = [c["masks"] for c in cases if c["render_device_ms"] >= c["render_host_ms"]]
    counts = sorted({c["masks"] for c in cases})
    ahead_from = [n for n in counts if not behind or n > max(behind)]
    result = {"device": torch.cuda.get_device_name(dev), "generator": "tools/outline_bench.py blobs on seeded noise, seed %d" % args.seed,
              "png_level": draw.PNG_LEVEL, "hbm_tbs": {"spec": HBM_SPEC_TBS, "float4_copy": HBM_COPY_TBS}, "frames": cases,
              "min_masks_device_ahead": (0 if not behind else (ahead_from[0] if ahead_from else None))}
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
