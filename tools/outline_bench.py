"""Analyzer.make_json_results, host statement (find_contours + np.argwhere per final mask, in Python) against the device form
(csrc/outline.hip: one ops.mask_plane_outlines call per frame), the host split of Analyzer._accept, and the merged-source outlines
of SFinder.merge_edge_sources_device; prints one JSON object and writes it (default profiles/outline_bench.json).

    python tools/outline_bench.py [--d 1,4,10,30,100] [--size 512] [--reps 5] [--grid 16] [--no-merge] [--out FILE]

The frame: D blob-shaped masks (discs of radius 4 - 22 px on a jittered grid, so that none merges with another; ragged rims, every
third with a hole) on a size x size frame.  Per D, on the same Analyzer state, in the same process:
  host       make_json_results_host;
  device     make_json_results_device with the frame's bit planes already on the device (as extract_det_masks_device leaves
             them), and once more from the host masks (one upload + pack); device synchronised before and after;
  kernels    the device time of the two launch groups of one call (events), and the call's stages (results_timing);
  accept     the host split of Analyzer._accept at this D: extract_det_masks (host statement, one run from D >= 30; and the
             device path), the pixel lists (np.argwhere ... tolist), the contours (pad, find_contours, tolist), json.dump, and the
             region lines + file.
Host and device runs alternate; medians of --reps (at least 5) runs.  The two `results` are compared first and nothing is
written unless they are equal.  `min_masks_device_ahead` is the smallest D at which the device form (planes resident) was ahead --
the value of Analyzer.RESULTS_DEVICE_MIN_MASKS -- or null.
The merged sources: the catalogue of tools/sfinder_bench.py (same generator, --grid 16: 895 merged components);
merge_edge_sources_device with results_device off and on, alternating, the catalogues compared first; and the contour stage
alone: find_contours over all unions as _merged_source runs it, against SFinder._union_outlines + the list building."""
import argparse
import copy
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

CLASS_NAMES = ["bkg", "spurious", "compact", "extended"]


def blobs(n, size, seed):
    """The detect() result of n blobs that do not touch: rois, class_ids, scores in [0.7, 1), masks [size, size, n] bool."""
    rng = np.random.default_rng(seed)
    side = int(np.ceil(np.sqrt(n)))
    cell = size // side
    rmax = max(3, min(22, cell // 2 - 2))
    yy, xx = np.mgrid[0:size, 0:size]
    masks = np.zeros((size, size, n), bool)
    rois = np.zeros((n, 4), np.int32)
    for i in range(n):
        r = int(rng.integers(min(4, rmax), rmax + 1))
        gy, gx = divmod(i, side)
        cy = gy * cell + int(rng.integers(r + 1, max(cell - r, r + 2)))
        cx = gx * cell + int(rng.integers(r + 1, max(cell - r, r + 2)))
        d2 = (yy - cy) ** 2 + (xx - cx) ** 2
        m = d2 <= r * r
        rim = m & (d2 > (r - 1.5) ** 2)
        m &= ~(rim & (rng.uniform(size=m.shape) < 0.35))                  # a ragged edge
        if i % 3 == 2 and r >= 5:
            m &= d2 > (r // 3) ** 2                                         # a hole
        masks[:, :, i] = m
        ys, xs = np.nonzero(m)
        rois[i] = (ys.min(), xs.min(), ys.max() + 1, xs.max() + 1)
    return {"rois": rois, "masks": masks, "class_ids": rng.integers(2, len(CLASS_NAMES), size=n).astype(np.int32),
            "scores": rng.uniform(0.7, 1.0, size=n).astype(np.float32)}


def analyzer(res):
    from caesar_mrcnn_amd import analyze
    from caesar_mrcnn_amd.config import run_py_config
    cfg = run_py_config(num_classes=len(CLASS_NAMES), imgsize=64, mode="inference")
    cfg.CLASS_NAMES = list(CLASS_NAMES)
    an = analyze.Analyzer(None, cfg)
    an.image = np.zeros(res["masks"].shape[:2] + (3,), np.uint8)
    an.image_id = "bench"
    an.masks, an.boxes, an.class_ids, an.scores = res["masks"], res["rois"], res["class_ids"], res["scores"]
    an.nobjects = an.masks.shape[-1]
    return an


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


def frame_case(D, size, reps, seed, tmp):
    import torch
    from caesar_mrcnn_amd import analyze, ops
    sync = torch.cuda.synchronize
    res = blobs(D, size, seed)
    an = analyzer(res)
    # extract_det_masks: the device path (it leaves the planes the device form of the results reuses), then the host statement
    an.postprocess_device = True
    an.masks_device = an.masks_device_host = None
    an.extract_det_masks_device()                                          # warm-up
    t_ext_dev = [timed(an.extract_det_masks_device, sync)[0] for _ in range(reps)]
    planes_state = an._final_planes
    final_dev = [np.asarray(m).copy() for m in an.masks_final]
    t_ext_host = [timed(an.extract_det_masks_host)[0] for _ in range(1 if D >= 30 else reps)]
    assert len(final_dev) == len(an.masks_final) and all(np.array_equal(a, b) for a, b in zip(final_dev, an.masks_final))
    n_final = len(an.masks_final)
    host_masks = an.masks_final

    def device_form(resident):
        an._final_planes = (planes_state[0], an.masks_final) if resident else None
        an.make_json_results_device()
        return an.results
    an.make_json_results_host()
    want = an.results
    for resident in (True, False):                                         # equality first (and warm-up)
        got = device_form(resident)
        assert got == want and json.dumps(got, sort_keys=True) == json.dumps(want, sort_keys=True), "results differ at D = %d" % D
    t_host, t_dev, t_up, stages = [], [], [], []
    for _ in range(reps):                                                  # alternating
        t_host.append(timed(an.make_json_results_host)[0])
        t_dev.append(timed(lambda: device_form(True), sync)[0])
        stages.append(dict(an.results_timing))
        t_up.append(timed(lambda: device_form(False), sync)[0])
    kern = []
    for _ in range(reps):
        k = {}
        ops.mask_plane_outlines(planes_state[0], timing=k)
        kern.append(k)
    # the host split of _accept's remaining steps
    xmin, ymin = an.image_xmin, an.image_ymin

    def pixel_lists():
        return [(np.argwhere(np.asarray(m) == 1) + np.array([ymin, xmin])).tolist() for m in host_masks]

    def contours():
        out = []
        for m in host_masks:
            m = np.asarray(m)
            padded = np.zeros((m.shape[0] + 2, m.shape[1] + 2), dtype=np.uint8)
            padded[1:-1, 1:-1] = m
            out.append([(np.fliplr(v) - 1 + np.array([xmin, ymin])).tolist() for v in analyze.find_contours(padded, 0.5)])
        return out
    an.make_json_results_host()
    t_pix = [timed(pixel_lists)[0] for _ in range(reps)]
    t_con = [timed(contours)[0] for _ in range(reps)]
    t_dump = [timed(lambda: an.write_json_results(os.path.join(tmp, "bench.json")))[0] for _ in range(reps)]

    def regions():
        an.make_ds9_regions(an.use_polygon_regions)
        an.write_ds9_regions(os.path.join(tmp, "bench.reg"))
    t_reg = [timed(regions)[0] for _ in range(reps)]
    out = {"detections": D, "final_masks": n_final, "frame": [size, size], "identical": True, "runs": reps,
           "segments": kern[0]["segments"], "pixels": kern[0]["pixels"],
           "make_json_results_host_ms": med(t_host), "make_json_results_device_ms": med(t_dev),
           "make_json_results_device_with_upload_ms": med(t_up), "host_over_device": round(med(t_host) / med(t_dev), 2),
           "device_stages_ms": {k: med([s[k] for s in stages]) for k in stages[0] if k.endswith("_ms")},
           "kernels_ms": {k: med([s[k] for s in kern]) for k in ("count_kernels_ms", "emit_kernels_ms")},
           "accept_host_split_ms": {"extract_det_masks_host": med(t_ext_host), "extract_det_masks_host_runs": len(t_ext_host),
                                    "extract_det_masks_device": med(t_ext_dev), "pixel_lists": med(t_pix), "contours": med(t_con),
                                    "json_dump": med(t_dump), "regions": med(t_reg)}}
    sys.stderr.write(json.dumps(out) + "\n")
    sys.stderr.flush()
    return out


def merge_case(grid, reps, seed):
    import torch
    import sfinder_bench as SB
    from caesar_mrcnn_amd import analyze, ops
    from caesar_mrcnn_amd.sfinder import pack_sources, unpack_bitmap
    sync = torch.cuda.synchronize
    size = (grid + 1) * 512 // 2
    labels, n = SB.plant(size, 900 * grid * grid // 256, seed)
    sf = SB.tile_catalogue(labels, 512, 0.5)
    pristine = sf.tile_sources

    def merge(on):
        sf.tile_sources = copy.deepcopy(pristine)
        sf.results_device = on
        ms, _ = timed(sf.merge_edge_sources_device, sync)
        return ms, sf.sources["sources"]
    _, off_out = merge(False)
    _, on_out = merge(True)
    assert len(off_out) == len(on_out) and all(SB._key(a) == SB._key(b) for a, b in zip(on_out, off_out)), "catalogues differ"
    t_off, t_on = [], []
    for _ in range(reps):
        t_off.append(merge(False)[0])
        t_on.append(merge(True)[0])
    # the contour stage alone, on the unions of the same components
    sf.tile_sources = copy.deepcopy(pristine)
    todo = sf._split_edge_sources()
    pairs = sf.candidate_pairs(todo)
    pool, desc = pack_sources([sf._edge_source(t)["pixels"] for t in todo])
    pool_t, desc_t = ops.tile_upload(pool, desc, sf._device())
    adj = ops.tile_adjacency(pool_t, desc_t, pairs).cpu().numpy()
    cc = [c for c in analyze.connected_components(len(todo), [tuple(p) for p in pairs[adj != 0].tolist()]) if len(c) > 1]
    comp_offsets = np.concatenate([[0], np.cumsum([len(c) for c in cc])]).astype(np.int32)
    u = ops.tile_union(pool_t, desc_t, desc, comp_offsets, np.concatenate(cc).astype(np.int32))
    out_desc = u["out_desc"].cpu().numpy()
    out_pool = u["out_pool"].cpu().numpy().view(np.uint32)
    unions = []
    for x0, y0, w, h, off, wpr in out_desc.tolist():
        unions.append((unpack_bitmap(out_pool[off:off + h * wpr], h, w, wpr).astype(np.uint8), x0, y0))

    def host_stage():
        out = []
        for mask, xmin, ymin in unions:
            dy, dx = mask.shape
            padded = np.zeros((dy + 20, dx + 20), dtype=np.uint8)
            padded[10:10 + dy, 10:10 + dx] = mask
            vertexes = []
            for verts in analyze.find_contours(padded, 0.5):
                verts = np.fliplr(verts).tolist()
                for v in verts:
                    v[0] += xmin - 10
                    v[1] += ymin - 10
                vertexes.append(verts)
            out.append(vertexes)
        return out

    def device_stage():
        got = sf._union_outlines(u, out_desc)
        return [[(c + np.array([x0, y0])).tolist() for c in got[k]] for k, (_, x0, y0) in enumerate(unions)]
    assert host_stage() == device_stage(), "merged-source contours differ"
    t_h, t_d, kern = [], [], []
    for _ in range(reps):
        t_h.append(timed(host_stage)[0])
        t_d.append(timed(device_stage, sync)[0])
        k = {}
        ops.bitmap_outlines(u["out_pool"], u["out_desc"], out_desc, timing=k)
        kern.append(k)
    out = {"mosaic": [size, size], "planted_sources": n, "edge_sources": len(todo), "components_merged": len(cc), "identical": True, "runs": reps,
           "segments": kern[0]["segments"],
           "merge_edge_sources_device_ms": {"results_device_off": med(t_off), "results_device_on": med(t_on)},
           "contour_stage_ms": {"host_find_contours": med(t_h), "device_union_outlines": med(t_d),
                                "host_over_device": round(med(t_h) / med(t_d), 2)},
           "kernels_ms": {k_: med([s[k_] for s in kern]) for k_ in ("count_kernels_ms", "emit_kernels_ms")}}
    sys.stderr.write(json.dumps(out) + "\n")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--d", default="1,4,10,30,100")
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--grid", type=int, default=16)
    ap.add_argument("--no-merge", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "outline_bench.json"))
    args = ap.parse_args()
    assert args.reps >= 5, "medians of at least 5 runs"
    import logging
    logging.getLogger("mrcnn").setLevel(logging.ERROR)
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda", torch.cuda.current_device())
    with tempfile.TemporaryDirectory() as tmp:
        cases = [frame_case(int(v), args.size, args.reps, args.seed, tmp) for v in args.d.split(",")]
    ahead = [c["final_masks"] for c in cases if c["make_json_results_device_ms"] < c["make_json_results_host_ms"]]
    behind = [c["final_masks"] for c in cases if c["make_json_results_device_ms"] >= c["make_json_results_host_ms"]]
    result = {"device": torch.cuda.get_device_name(dev), "generator": "ragged discs of radius 4-22 px on a jittered grid, seed %d" % args.seed,
              "frames": cases,
              # ahead at this count and at every larger one measured
              "min_masks_device_ahead": min([a for a in ahead if not behind or a > max(behind)], default=None)}
    if not args.no_merge:
        result["merged_sources"] = merge_case(args.grid, args.reps, args.seed)
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
