#!/usr/bin/env python3
"""The output transform of a Winograd data gradient (mrcnn_winograd_output_bwd_zmask_g: epilogue backward of the layer below,
channel-sum partials) against its forward twin (mrcnn_winograd_output_g with the z store), which moves the same bytes: per tile
group of the mixed 14 x 14 tiling, C = 256, at 2048 ROIs (dense) and 672 (the positive-quota step).  HIP events around every
launch, 3 warm-up + 20 timed; one JSON line per (N, group) with the median [min, max] in us, the algorithmic bytes and TB/s,
and one line per N for the layer's one channel-sum launch over the partials of all four groups (tools only).
usage: wino_output_bwd_bench.py [ROIs ...]"""
import ctypes as C
import json
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from caesar_mrcnn_amd import ops

H = W = 14
CH = 256
WARM, REPS = 3, 20


def timed(fn):
    for _ in range(WARM):
        assert fn() == 0
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(REPS + 1)]
    ev[0].record()
    for k in range(REPS):
        fn()
        ev[k + 1].record()
    torch.cuda.synchronize()
    us = sorted(ev[k].elapsed_time(ev[k + 1]) * 1e3 for k in range(REPS))
    return {"us": round((us[REPS // 2 - 1] + us[REPS // 2]) / 2, 1), "min": round(us[0], 1), "max": round(us[-1], 1)}


def bwd_launch(lib, Mt, dz, z, scale, shift, mean, rstd, part, N, g):
    """one group's launch of the kernel under test (its partial rows go to `part`)"""
    P, st = ops.ptr, ops.current_stream
    return lambda: lib.mrcnn_winograd_output_bwd_zmask_g(P(Mt), P(dz), P(z), P(scale), P(shift), P(mean), P(rstd), P(part), N, H, W, CH,
                                                         C.byref(g), st())


def main(argv, bwd_launch=bwd_launch, sums=True):
    lib = ops._hip.lib()
    dev = torch.device("cuda:0")
    P, st = ops.ptr, ops.current_stream
    gen = torch.Generator(device=dev).manual_seed(1)
    for N in [int(a) for a in argv] or [2048, 672]:
        z = torch.randn((N, H, W, CH), device=dev, generator=gen)
        out, zf, dz = torch.empty_like(z), torch.empty_like(z), torch.empty_like(z)
        scale = torch.rand(CH, device=dev, generator=gen) + 0.5
        shift = torch.rand(CH, device=dev, generator=gen) * 0.6 - 0.3
        mean, rstd, bias = torch.zeros(CH, device=dev), torch.ones(CH, device=dev), torch.zeros(CH, device=dev)
        groups = ops.winograd_groups(H, W, ops.TILE_MIXED)
        rows = [lib.mrcnn_winograd_output_bwd_rows(C.byref(g), N, CH) for g in groups] if sums else [0] * len(groups)
        part = torch.zeros(max(sum(rows), 1) * 3 * CH, device=dev)
        for gi, g in enumerate(groups):
            nm = lib.mrcnn_winograd_group_floats(C.byref(g), N, CH)
            Mt = torch.randn(nm, device=dev, generator=gen)
            tiles = N * g.th_n * g.tw_n
            nbytes = 4 * CH * tiles * ((g.oth + 2) * (g.otw + 2) + 2 * g.oth * g.otw)     # Mt read + two map-sized streams
            fwd = lambda: lib.mrcnn_winograd_output_g(P(Mt), P(out), P(zf), P(bias), P(scale), P(shift), N, H, W, CH, ops.ACT_RELU,
                                                      C.byref(g), st())
            f = timed(fwd)
            bwd = bwd_launch(lib, Mt, dz, z, scale, shift, mean, rstd, part[sum(rows[:gi]) * 3 * CH:], N, g)
            b = timed(bwd)
            f["TBps"], b["TBps"] = round(nbytes / f["us"] / 1e6, 2), round(nbytes / b["us"] / 1e6, 2)
            print(json.dumps({"N": N, "group": "%dx%d" % (g.oth, g.otw), "tiles": tiles, "bytes": nbytes, "output_fwd_z": f,
                              "output_bwd_zmask": b, "bwd_over_fwd": round(b["us"] / f["us"], 2)}), flush=True)
        if sums:
            dg, db, dbi = (torch.zeros(CH, device=dev) for _ in range(3))
            s = timed(lambda: lib.mrcnn_winograd_output_bwd_sums(P(part), sum(rows), CH, P(dg), P(db), P(dbi), st()))
            print(json.dumps({"N": N, "kernel": "output_bwd_sums (once per layer)", "rows": sum(rows), "bytes": sum(rows) * 3 * CH * 4,
                              "us": s}), flush=True)


if __name__ == "__main__":
    main(sys.argv[1:])
