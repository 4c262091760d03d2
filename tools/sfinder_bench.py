"""The tile-merge stage of the tiled source finder (caesar_mrcnn_amd.sfinder) on a seeded synthetic mosaic catalogue; prints one
JSON object (and writes it with --out).

    python tools/sfinder_bench.py [--grid 16] [--tile 512] [--sources 900] [--reps 3] [--out FILE] [--host-only]

The catalogue: a square mosaic cut into 512-tiles at step 0.5 (--grid 16: spans 0, 256, .. so that 16 full tiles fit per axis),
--sources planted ellipses of 50-5000 pixels, kept apart; a fixed share of them (1 in 5) carries a thin ring three pixels
outside it -- a second source whose box contains the ellipse's box and whose pixels never touch it, the case in which the
reference's pixel loops run their full product.  Every tile reports what it sees of every planted source, so at step 0.5 most
sources arrive two to four times and have to be merged.
Timed: (a) SFinder.merge_edge_sources_host -- the literal statement of the reference's algorithm, the baseline; (b)
SFinder.merge_edge_sources_device end to end (candidate pairs, packing, upload, both launches, downloads, component search,
pixel lists, contours), device synchronised before and after, with its stages; (c) the two kernels alone (device events, inputs
resident).  The two catalogues are compared first; nothing is reported unless they are equal."""
import argparse
import copy
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def plant(size, n_sources, seed):
    """Label map [size, size] int32 and the number of sources planted (ellipses; every fifth with a ring around it)."""
    rng = np.random.RandomState(seed)
    labels = np.zeros((size, size), np.int32)
    blocked = np.zeros((size, size), bool)
    n = tries = 0
    while n < n_sources and tries < 50 * n_sources:
        tries += 1
        a, b, th = rng.uniform(4, 40), rng.uniform(4, 40), rng.uniform(0, np.pi)
        ring = (n % 5 == 4)
        r = int(max(a, b)) + (10 if ring else 4)
        cy, cx = rng.randint(r, size - r), rng.randint(r, size - r)
        if blocked[cy - r:cy + r + 1, cx - r:cx + r + 1].any():
            continue
        yy, xx = np.mgrid[-r:r + 1, -r:r + 1]
        u = xx * np.cos(th) + yy * np.sin(th)
        v = -xx * np.sin(th) + yy * np.cos(th)
        q = np.sqrt((u / a) ** 2 + (v / b) ** 2)
        m = q <= 1.0
        if m.sum() < 50:
            continue
        win = labels[cy - r:cy + r + 1, cx - r:cx + r + 1]
        n += 1
        win[m] = n
        if ring and n < n_sources:
            s = min(a, b)
            band = (q > 1.0 + 3.5 / s) & (q <= 1.0 + 5.5 / s)        # at least three pixels off the ellipse
            n += 1
            win[band] = n
        blocked[cy - r:cy + r + 1, cx - r:cx + r + 1] = True
    return labels, n


def tile_catalogue(labels, tile, step):
    """An SFinder whose tile_sources hold what every tile sees of the label map, edge flags set by find_sources_at_edge."""
    from caesar_mrcnn_amd.config import SDetectorConfig
    from caesar_mrcnn_amd.sfinder import SFinder
    cfg = SDetectorConfig()
    cfg.IMG_PATH = "synthetic.fits"
    cfg.MAX_NTASKS_PER_WORKER = 1 << 30
    sf = SFinder(None, cfg)
    size = labels.shape[0]
    sf.xmin, sf.xmax, sf.ymin, sf.ymax = 0, size - 1, 0, size - 1
    sf.tileSizeX = sf.tileSizeY = tile
    sf.tileStepSizeX = sf.tileStepSizeY = step
    assert sf.create_tile_tasks() == 0
    for j, t in enumerate(sf.tasks_per_worker[0]):
        crop = labels[t.iy_min:t.iy_max, t.ix_min:t.ix_max]
        ys, xs = np.nonzero(crop)
        ids = crop[ys, xs]
        order = np.argsort(ids, kind="stable")
        ys, xs, ids = ys[order], xs[order], ids[order]
        objs = []
        cuts = np.flatnonzero(np.diff(ids)) + 1
        for k, (y, x) in enumerate(zip(np.split(ys, cuts), np.split(xs, cuts))):
            if y.size == 0:
                continue
            y, x = y + t.iy_min, x + t.ix_min
            objs.append({"name": "S%d_t%d" % (k + 1, t.tid), "x1": int(x.min()), "x2": int(x.max()) + 1, "y1": int(y.min()),
                         "y2": int(y.max()) + 1, "class_id": 1, "class_name": "source", "score": 0.9, "edge": False,
                         "pixels": np.stack([y, x], axis=1).tolist(), "vertexes": []})
        if objs:
            t.det_sources = {"image_id": "synthetic", "objs": objs, "workerId": 0, "tileId": t.tid, "neighborTileIds": t.neighborTaskId,
                             "xmin": t.ix_min, "xmax": t.ix_max, "ymin": t.iy_min, "ymax": t.iy_max}
            sf.find_sources_at_edge(j)
    sf.tile_sources = {"sources": [t.det_sources for t in sf.tasks_per_worker[0] if t.det_sources]}
    return sf


def _key(s):
    return (s["name"], s["x1"], s["x2"], s["y1"], s["y2"], s["edge"], s["merged"], s["class_id"], s["score"],
            tuple(map(tuple, s["pixels"])), json.dumps(s["vertexes"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=16)
    ap.add_argument("--tile", type=int, default=512)
    ap.add_argument("--sources", type=int, default=900)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--host-only", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import logging
    logging.getLogger("mrcnn").setLevel(logging.ERROR)
    size = (args.grid + 1) * args.tile // 2
    labels, n = plant(size, args.sources, args.seed)
    sf = tile_catalogue(labels, args.tile, 0.5)
    pristine = sf.tile_sources
    objs = [s for t in pristine["sources"] for s in t["objs"]]
    npix = np.array([len(s["pixels"]) for s in objs if s["edge"]])
    res = {"mosaic": [size, size], "tile": args.tile, "step": 0.5, "tiles": len(sf.tasks_per_worker[0]), "planted_sources": n,
           "tile_detections": len(objs), "edge_sources": int(npix.size),
           "edge_source_pixels": {"min": int(npix.min()), "median": int(np.median(npix)), "max": int(npix.max())}}

    def run(method):
        times, out = [], None
        for _ in range(args.reps):
            sf.tile_sources = copy.deepcopy(pristine)
            if not args.host_only:
                torch.cuda.synchronize()
            t0 = time.perf_counter()
            getattr(sf, method)()
            if not args.host_only:
                torch.cuda.synchronize()
            times.append(1e3 * (time.perf_counter() - t0))
            out = sf.sources["sources"]
        return times, out

    if not args.host_only:
        import torch
        from caesar_mrcnn_amd import ops
        from caesar_mrcnn_amd.sfinder import pack_sources
        assert torch.cuda.is_available(), "needs a GPU (or --host-only)"
        sf.tile_sources = copy.deepcopy(pristine)
        sf.merge_edge_sources_device()                     # warm-up: library load, allocator
        dev_ms, dev_out = run("merge_edge_sources_device")
        stages = dict(sf.merge_timing)
    host_ms, host_out = run("merge_edge_sources_host")
    res["host_ms"] = [round(v, 1) for v in host_ms]
    res["catalogue_sources"] = len(host_out)
    res["merged_sources"] = sum(1 for s in host_out if s["merged"])
    if not args.host_only:
        assert len(dev_out) == len(host_out) and all(_key(a) == _key(b) for a, b in zip(dev_out, host_out)), "catalogues differ"
        res["identical"] = True
        res["device_end_to_end_ms"] = [round(v, 1) for v in dev_ms]
        res["device_stages_last_run"] = stages
        res["host_over_device"] = round(min(host_ms) / min(dev_ms), 2)
        # the kernels alone
        sf.tile_sources = copy.deepcopy(pristine)
        todo = sf._split_edge_sources()
        pairs = sf.candidate_pairs(todo)
        pool, desc = pack_sources([sf._edge_source(t)["pixels"] for t in todo])
        pool_t, desc_t = ops.tile_upload(pool, desc, sf._device())
        pairs_t = torch.from_numpy(pairs).to(pool_t.device)
        adj = ops.tile_adjacency(pool_t, desc_t, pairs_t).cpu().numpy()
        from caesar_mrcnn_amd import analyze
        cc = [c for c in analyze.connected_components(len(todo), [tuple(p) for p in pairs[adj != 0].tolist()]) if len(c) > 1]
        comp_offsets = np.concatenate([[0], np.cumsum([len(c) for c in cc])]).astype(np.int32)
        member_ids = np.concatenate(cc).astype(np.int32)

        def kernel_us(f, reps=20):
            out = []
            for _ in range(reps):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                keep = f()
                b.record()
                b.synchronize()
                out.append(1e3 * a.elapsed_time(b))
                del keep
            return round(float(np.median(out)), 1)
        res["kernel_us"] = {"tile_adjacency": kernel_us(lambda: ops.tile_adjacency(pool_t, desc_t, pairs_t)),
                            "tile_union_with_its_uploads_and_clears": kernel_us(lambda: ops.tile_union(pool_t, desc_t, desc, comp_offsets, member_ids)),
                            "pairs": int(len(pairs)), "components": len(cc), "members": int(len(member_ids))}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
