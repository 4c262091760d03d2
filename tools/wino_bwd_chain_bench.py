#!/usr/bin/env python3
"""The backward chain launch (mrcnn_winograd_bwd_chain: four output transforms with the epilogue backward, and the input and dy
transforms of that dz, dz kept in LDS) against the 12 launches it replaces (4 x mrcnn_winograd_output_bwd_zmask_g,
4 x mrcnn_winograd_input_g, 4 x mrcnn_winograd_dy_g, here one after the other on one stream), and against its yardstick, the forward
chain launch (mrcnn_winograd_chain) on the same shapes in the same run: mixed 14 x 14 tiling, C = 256, at 2048 ROIs (dense) and 672
(the positive-quota step).  HIP events around every launch (or group of 12), 3 warm-up + 20 timed; one JSON line per N with the
median [min, max] in us, the algorithmic bytes and TB/s of each, and the backward launch's time against the forward's scaled by
bytes.
usage: wino_bwd_chain_bench.py [ROIs ...]"""
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


def main(argv):
    lib = ops._hip.lib()
    dev = torch.device("cuda:0")
    P, st = ops.ptr, ops.current_stream
    gen = torch.Generator(device=dev).manual_seed(1)
    for N in [int(a) for a in argv] or [2048, 672]:
        z = torch.randn((N, H, W, CH), device=dev, generator=gen)
        dz, zf = torch.empty_like(z), torch.empty_like(z)
        scale = torch.rand(CH, device=dev, generator=gen) + 0.5
        shift = torch.rand(CH, device=dev, generator=gen) * 0.6 - 0.3
        mean, rstd, bias = torch.zeros(CH, device=dev), torch.ones(CH, device=dev), torch.zeros(CH, device=dev)
        groups = ops.winograd_groups(H, W, ops.TILE_MIXED)
        nms = [lib.mrcnn_winograd_group_floats(C.byref(g), N, CH) for g in groups]
        rows = [lib.mrcnn_winograd_output_bwd_rows(C.byref(g), N, CH) for g in groups]
        Mt = torch.randn(sum(nms), device=dev, generator=gen)
        V, dM = torch.empty(sum(nms), device=dev), torch.empty(sum(nms), device=dev)
        part = torch.zeros(max(sum(rows), N) * 3 * CH, device=dev)
        # algorithmic bytes: the matrices' first T rows of every group, the map-sized streams
        mt_bytes = 4 * CH * sum(N * g.th_n * g.tw_n * (g.oth + 2) * (g.otw + 2) for g in groups)
        map_bytes = 4 * CH * N * H * W
        chain_bytes = {"bwd_chain": 3 * mt_bytes + map_bytes, "separate_12": 3 * mt_bytes + 4 * map_bytes, "fwd_chain": 2 * mt_bytes + map_bytes}

        def separate():
            off = done = 0
            for g, nm, r in zip(groups, nms, rows):
                rc = lib.mrcnn_winograd_output_bwd_zmask_g(P(Mt) + off * 4, P(dz), P(z), P(scale), P(shift), P(mean), P(rstd),
                                                           P(part) + done * 3 * CH * 4, N, H, W, CH, C.byref(g), st())
                assert rc == 0
                off += nm
                done += r
            off = 0
            for g, nm in zip(groups, nms):
                assert lib.mrcnn_winograd_input_g(P(dz), P(V) + off * 4, N, H, W, CH, C.byref(g), st()) == 0
                assert lib.mrcnn_winograd_dy_g(P(dz), P(dM) + off * 4, N, H, W, CH, C.byref(g), st()) == 0
                off += nm
            return 0

        res = {
            "separate_12": timed(separate),
            "bwd_chain": timed(lambda: lib.mrcnn_winograd_bwd_chain(P(Mt), P(z), P(scale), P(shift), P(mean), P(rstd), P(part), P(V), P(dM), None,
                                                                    N, H, W, CH, ops.TILE_MIXED, st())),
            "fwd_chain": timed(lambda: lib.mrcnn_winograd_chain(P(Mt), P(zf), P(bias), P(scale), P(shift), P(V), N, H, W, CH, ops.ACT_RELU,
                                                                ops.TILE_MIXED, st())),
        }
        for k, r in res.items():
            r["bytes"] = chain_bytes[k]
            r["TBps"] = round(chain_bytes[k] / r["us"] / 1e6, 2)
        yard = res["fwd_chain"]["us"] * chain_bytes["bwd_chain"] / chain_bytes["fwd_chain"]
        print(json.dumps(dict(res, N=N, fwd_chain_scaled_by_bytes_us=round(yard, 1), bwd_over_scaled_fwd=round(res["bwd_chain"]["us"] / yard, 3),
                              bwd_over_separate=round(res["bwd_chain"]["us"] / res["separate_12"]["us"], 3))), flush=True)


if __name__ == "__main__":
    main(sys.argv[1:])
