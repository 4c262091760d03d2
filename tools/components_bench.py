"""Analyzer.components_device: the host statement (analyze.label_components / are_mask_connected / count_islands / min_area_rect
on full frames) against the device form (csrc/components.hip: ops.mask_components, mask_components_split, mask_row_extents on
bit planes), on the same machine, for the three places that ask for connected components; prints one JSON object and writes it
(default profiles/components_bench.json).

    python tools/components_bench.py [--d 1,4,10,30,100] [--size 512] [--reps 5] [--step-timeout 900] [--out FILE]

Workloads, each with D masks on a size x size frame:
  gt      extract_gt_masks with split_gtmasks: D true masks (the discs of tools/tester_bench.py), every second one with a second
          island, classes compact / extended (never split) / spurious;
  pars    compute_det_mask_pars on the tester's device path (eval_device on for both): count_islands + min_area_rect per final mask
          on the host, against one mask_components(8) + mask_row_extents call and one download;
  split   extract_det_masks with split_masks and postprocess_device (the blobs of tools/outline_bench.py, ragged rims: several
          pieces each), the masks resident on the device as MaskRCNN keeps them: labelling + upload of the pieces on the host,
          against mask_components(4) + mask_components_split.
Every (workload, D) is one step: a child process of its own under --step-timeout seconds, so that a step that hangs or faults
ends there; the first step that fails ends the run (what was measured until then is written, with `failed_step`).  In a step the
two forms are compared first (`equal`; nothing is timed unless they agree), warmed up, then timed alternately, --reps runs each
(the host form once where one run takes seconds); medians.  `kernels_ms`: the device time of the count and emit launches of one
call on the step's planes (events).  `min_masks_device_ahead[workload]`: the smallest D at which the device form was ahead, or
null."""
import argparse
import contextlib
import io
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

WORKLOADS = ("gt", "pars", "split")


def med(v):
    return round(float(np.median(v)), 3)


def timed(f):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = f()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0), out


def kernel_times(planes, connectivity, first_only, reps):
    """Device time (events) of the labelling launch and of the emit launch on these planes."""
    import torch
    from caesar_mrcnn_amd import ops
    boxes = planes.box.cpu().numpy()
    count, emit = [], []
    for _ in range(reps + 1):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        ev[0].record()
        handle = ops.mask_components(planes, connectivity, boxes_host=boxes)
        ev[1].record()
        handle.ncomp.cpu()
        ev[2].record()
        pieces, _ = ops.mask_components_split(handle, first_only=first_only)
        ev[3].record()
        ev[3].synchronize()
        count.append(ev[0].elapsed_time(ev[1]))
        emit.append(ev[2].elapsed_time(ev[3]))
    return {"count_ms": med(count[1:]), "emit_ms": med(emit[1:]), "pieces": int(pieces.n)}


def same_lists(a, b):
    return len(a) == len(b) and all(np.asarray(x).dtype == np.asarray(y).dtype and np.array_equal(x, y) for x, y in zip(a, b))


def step_gt(D, size, reps):
    import tester_bench as TB
    from caesar_mrcnn_amd import analyze
    sc = TB.scene(D, 1, size, 100 + D)
    extra = TB.scene(D, 1, size, 200 + D)["gt"]
    names = ["bkg", "spurious", "compact", "extended"]
    masks = np.stack([m | (extra[k] if k % 2 else 0) for k, m in enumerate(sc["gt"])], axis=-1)

    def make(on):
        cfg = TB.types.SimpleNamespace(NUM_CLASSES=len(names), CLASS_NAMES=list(names))
        an = analyze.Analyzer(None, cfg, TB.types.SimpleNamespace(nclasses=len(names), consider_sources_near_mixed_sidelobes=True), [], [])
        an.class_names = an.class_names_gt = list(names)
        an.masks_gt, an.class_ids_gt = masks, list(sc["gt_ids"])
        an.labels_gt = [names[c] for c in an.class_ids_gt]
        an.sidelobes_mixed_or_near_gt = [k % 3 == 0 for k in range(D)]
        an.split_gtmasks, an.components_device = True, on
        return an

    def run(on):
        an = make(on)
        an.extract_gt_masks()
        return an
    t_first, host = timed(lambda: run(False))
    dev = run(True)
    equal = same_lists(dev.masks_gt_merged, host.masks_gt_merged) and same_lists(dev.bboxes_gt, host.bboxes_gt) and \
        dev.class_ids_gt_merged == host.class_ids_gt_merged and dev.captions_gt == host.captions_gt and \
        dev.sidelobes_mixed_or_near_gt_merged == host.sidelobes_mixed_or_near_gt_merged and "gt_masks_ms" in dev.components_timing
    out = {"true_masks": D, "list_entries": dev.components_timing.get("gt_entries"), "merged": len(host.masks_gt_merged), "equal": bool(equal)}
    if not equal:
        return out
    host_runs = 1 if t_first > 2000 else reps
    t_host, t_dev = [t_first] if host_runs == 1 else [], []
    for k in range(reps):
        if host_runs > 1:
            t_host.append(timed(lambda: run(False))[0])
        t_dev.append(timed(lambda: run(True))[0])
    planes, _ = make(True)._planes_of([masks[:, :, k] for k in range(D)])
    out.update(host_ms=med(t_host), host_runs=len(t_host), device_ms=med(t_dev), kernels_ms=kernel_times(planes, 4, True, reps))
    return out


def step_pars(D, size, reps):
    import tester_bench as TB
    from caesar_mrcnn_amd import fits
    sc = TB.scene(max(D // 3, 1), D, size, 300 + D)
    extra = TB.scene(1, D, size, 400 + D)["det"]
    sc["det"] = [m | (extra[k] if k % 2 else False) for k, m in enumerate(sc["det"])]              # every second mask: two islands
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "bench.fits")
        fits.write_fits(path, sc["img"])

        def run(on):
            an = TB.make_analyzer(sc, path, True)
            an.components_device = on
            with contextlib.redirect_stdout(io.StringIO()):
                assert an.compute_det_mask_pars() == 0
            return an
        host, dev = run(False), run(True)
        equal = dev.det_obj_pars == host.det_obj_pars and dev.components_timing.get("det_mask_shape_downloads") == 1 and \
            "det_mask_pars_ms" in host.eval_timing
        out = {"final_masks": D, "islands": int(sum(p.get("nislands", 0) for p in host.det_obj_pars)), "equal": bool(equal)}
        if not equal:
            return out
        t_host, t_dev = [], []
        for _ in range(reps):
            t_host.append(timed(lambda: run(False))[0])
            t_dev.append(timed(lambda: run(True))[0])
        planes = run(True)._eval_planes["final"][0]
    out.update(host_ms=med(t_host), host_runs=reps, device_ms=med(t_dev), kernels_ms=kernel_times(planes, 8, True, reps))
    return out


def step_split(D, size, reps):
    import torch
    import outline_bench as OB
    res = OB.blobs(D, size, 500 + D)
    kept = torch.from_numpy(np.ascontiguousarray(res["masks"]).view(np.uint8)).cuda()

    def run(on):
        an = OB.analyzer(res)
        an.postprocess_device, an.split_masks, an.components_device = True, True, on
        an.masks_device, an.masks_device_host = kept, an.masks
        an.extract_det_masks()
        return an
    host, dev = run(False), run(True)
    equal = same_lists(dev.masks_final, host.masks_final) and same_lists(dev.bboxes, host.bboxes) and dev.captions == host.captions and \
        dev.class_ids_final == host.class_ids_final and dev.scores_final == host.scores_final and \
        dev.postprocess_timing["mask_uploads"] == 0 and host.postprocess_timing["mask_uploads"] == 1
    out = {"detections": D, "pieces": dev.components_timing.get("split_pieces"), "final_masks": len(host.masks_final), "equal": bool(equal)}
    if not equal:
        return out
    t_host, t_dev = [], []
    for _ in range(reps):
        t_host.append(timed(lambda: run(False))[0])
        t_dev.append(timed(lambda: run(True))[0])
    from caesar_mrcnn_amd import ops
    out.update(host_ms=med(t_host), host_runs=reps, device_ms=med(t_dev), kernels_ms=kernel_times(ops.mask_planes_pack(kept), 4, False, reps))
    return out


def run_step(spec, size, reps):
    workload, D = spec.split(":")
    out = {"workload": workload, "masks": int(D), "frame": [size, size]}
    out.update({"gt": step_gt, "pars": step_pars, "split": step_split}[workload](int(D), size, reps))
    if "host_ms" in out:
        out["host_over_device"] = round(out["host_ms"] / out["device_ms"], 2)
    print(json.dumps(out))
    return 0 if out["equal"] else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--d", default="1,4,10,30,100")
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--step-timeout", type=int, default=900)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "components_bench.json"))
    ap.add_argument("--step", default=None, help="(internal) one step, workload:D, in this process")
    args = ap.parse_args()
    if args.step:
        return run_step(args.step, args.size, max(args.reps, 1))
    counts = [int(v) for v in args.d.split(",")]
    steps, failed = [], None
    for workload in WORKLOADS:
        for D in counts:
            spec = "%s:%d" % (workload, D)
            cmd = [sys.executable, os.path.abspath(__file__), "--step", spec, "--size", str(args.size), "--reps", str(args.reps)]
            try:
                done = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=args.step_timeout)
                lines = [l for l in done.stdout.decode().splitlines() if l.startswith("{")]
                if lines:
                    steps.append(json.loads(lines[-1]))
                    sys.stderr.write(lines[-1] + "\n")
                if done.returncode != 0 or not lines:
                    failed = {"step": spec, "returncode": done.returncode, "stderr_tail": done.stderr.decode()[-600:]}
            except subprocess.TimeoutExpired:
                failed = {"step": spec, "returncode": None, "stderr_tail": "timed out after %d s" % args.step_timeout}
            if failed:
                break
        if failed:
            break
    ahead = {}
    for workload in WORKLOADS:
        mine = [s for s in steps if s["workload"] == workload and "host_ms" in s]
        wins = [s["masks"] for s in mine if s["device_ms"] < s["host_ms"]]
        ahead[workload] = min(wins) if wins else None
    import torch
    out = {"tool": "tools/components_bench.py", "device": torch.cuda.get_device_name(0) if torch.cuda.is_available() else None,
           "frame": [args.size, args.size], "reps": args.reps, "equal": bool(steps) and all(s["equal"] for s in steps),
           "min_masks_device_ahead": ahead, "steps": steps}
    if failed:
        out["failed_step"] = failed
    text = json.dumps(out, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
