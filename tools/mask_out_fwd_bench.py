#!/usr/bin/env python3
"""The mask head's output stage alone (14 x 14 x 256 per ROI, 4 classes), at 2048 and 672 ROIs: the transposed convolution's GEMM
as ops.deconv2x2 launches it, the mrcnn_mask 1 x 1 convolution + sigmoid, their sum, and the single launch of ops.deconv2x2_mask
with and without the store of `up`.  HIP events around every launch, 3 warm-up + 20 timed, median [min - max] in ms; one JSON
line per ROI count to stdout and, with an argument, appended to that file (profiles/mask_out_fwd_isolated.jsonl)."""
import json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from caesar_mrcnn_amd import _hip, ops
dev = torch.device("cuda:0")
WARM, REPS = 3, 20


def timed(fn):
    ts = []
    for i in range(WARM + REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); torch.cuda.synchronize()
        if i >= WARM:
            ts.append(e0.elapsed_time(e1))
    return ts


def stat(ts):
    return {"median": round(statistics.median(ts), 4), "min": round(min(ts), 4), "max": round(max(ts), 4)}


out_path = sys.argv[1] if len(sys.argv) > 1 else None
for rois in (2048, 672):
    g = torch.Generator(device="cpu").manual_seed(rois)
    x = torch.randn(rois, 14, 14, 256, generator=g).to(dev)
    wg = (torch.randn(256, 1024, generator=g) * 0.05).to(dev)
    b = (torch.randn(256, generator=g) * 0.1).to(dev)
    wm = (torch.randn(256, 4, generator=g) * 0.1).to(dev)
    bm = (torch.randn(4, generator=g) * 0.1).to(dev)
    up = torch.empty(rois, 28, 28, 256, device=dev)
    m = torch.empty(rois, 28, 28, 4, device=dev)
    lib, p, st = _hip.lib(), ops.ptr, ops.current_stream()

    def fused(upbuf):
        _hip.check(lib.mrcnn_deconv2x2_mask_gemm(p(x), p(wg), p(b), p(upbuf), p(wm), p(bm), p(m), rois, 14, 14, 256, 256, 4, ops.ACT_RELU, st),
                   "mrcnn_deconv2x2_mask_gemm")
    t_dc = timed(lambda: ops.deconv2x2(x, wg, b, ops.ACT_RELU, out=up))
    t_mk = timed(lambda: ops.conv2d(up, wm.view(1, 1, 256, 4), bm, act=ops.ACT_SIGMOID, out=m))
    t_pair = timed(lambda: (ops.deconv2x2(x, wg, b, ops.ACT_RELU, out=up), ops.conv2d(up, wm.view(1, 1, 256, 4), bm, act=ops.ACT_SIGMOID, out=m)))
    t_f = timed(lambda: fused(up))
    t_fn = timed(lambda: fused(None))
    rec = {"rois": rois, "launches": "%d+%d" % (WARM, REPS), "unit": "ms", "deconv_gemm": stat(t_dc), "mask_1x1_sigmoid": stat(t_mk),
           "sum_of_medians": round(statistics.median(t_dc) + statistics.median(t_mk), 4), "pair_back_to_back": stat(t_pair),
           "fused": stat(t_f), "fused_no_up_store": stat(t_fn)}
    line = json.dumps(rec)
    print(line, flush=True)
    if out_path:
        with open(out_path, "a") as f:
            f.write(line + "\n")
