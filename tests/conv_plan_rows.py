"""Rows of tests/golden/conv_plan_table.json and their replay through mrcnn_conv2d_fwd_plan / mrcnn_conv2d_fwd_workspace.

A row is the inputs of one float32 convolution launch (descriptor, operand addresses, workspace, backward epilogue, tuning keys,
tail-split switch) plus what the library answered: status, every field of the plan, the workspace query.  The table is written
from a library whose selection is the one to keep (`python tests/conv_plan_rows.py <libmrcnn_hip.so> <table.json>`) and replayed
against the built tree by test_conv_plan_cpu.py.  No GPU: the query looks at nullness and alignment of addresses only.

Rows: every convolution of the benchmarked workloads (ResNet-101 + FPN at 256 x 256: the training step with four images, detect
with one and eight) as forward, data gradient and data gradient with the backward epilogue -- enumerated from the architecture;
both sides of every numeric rule of the planner (1 x 1 convolutions on 1 x 1 x M maps give any M); one row at least per pair of
kernel and reduction; every refusal."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

DESC_FIELDS = ("N", "H", "W", "Cin", "Cout", "KH", "KW", "stride", "pad_t", "pad_l", "OH", "OW", "act", "res_mode", "out_mode", "cmod",
               "out_n_stride", "out_h_stride", "out_w_stride")
OPERANDS = ("x", "w", "bias", "scale", "shift", "res", "out", "z_out")
EP_POINTERS = ("out", "z", "scale", "mean", "rstd", "dgamma", "dbeta", "dbias", "dy")
PLAN_FIELDS = ("kernel", "bm", "bn", "ksplit", "ksteps", "grid", "reduce", "mt_full", "tail_ksplit", "tail_ksteps", "slab_bytes")
# fake addresses, 16-byte aligned and apart; + 4 misaligns one
ADDR = {n: 0x10000000 * (i + 1) for i, n in enumerate(OPERANDS + ("workspace",) + tuple("ep_" + n for n in EP_POINTERS))}


def _same(size, k, stride):
    out = -(-size // stride)
    return out, max((out - 1) * stride + k - size, 0) // 2


def desc(N, H, W, Cin, Cout, k=1, stride=1, pad="valid", act=0, res_mode=0):
    if pad == "same":
        (OH, pt), (OW, pl) = _same(H, k, stride), _same(W, k, stride)
    elif pad == "valid":
        OH, OW, pt, pl = (H - k) // stride + 1, (W - k) // stride + 1, 0, 0
    else:
        OH, OW, pt, pl = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1, pad, pad
    return dict(N=N, H=H, W=W, Cin=Cin, Cout=Cout, KH=k, KW=k, stride=stride, pad_t=pt, pad_l=pl, OH=OH, OW=OW, act=act,
                res_mode=res_mode, out_mode=0, cmod=Cout, out_n_stride=OH * OW * Cout, out_h_stride=OW * Cout, out_w_stride=Cout)


def row(name, d, have=(), misaligned=(), null=(), ep=None, workspace="query", sk16=0, sk64=-1, tail=0, query=True, **desc_changes):
    """have: optional operands that are given (bias, scale, shift, res, z_out); ep: None, or a dict: act, `have` (its optional
    pointers; out, z, scale, mean, rstd are given unless listed in `null`).  workspace: "query" (the workspace query's answer at an
    aligned address), None, or bytes (negative: that many bytes short of the query's answer).  query False: the workspace query
    is not asked (a descriptor whose K overflows an int, which only the launch refuses)."""
    r = dict(name=name, desc=pack_desc(dict(d, **desc_changes)) if d is not None else None)
    opts = dict(have=list(have), mis=list(misaligned), null=list(null), ep=ep and dict(act=ep.get("act", 1), have=list(ep.get("have", ()))),
                ws=workspace, sk16=sk16, sk64=sk64, tail=tail, query=query)
    r.update({k: v for k, v in opts.items() if v != DEFAULTS[k]})        # the table keeps what differs from the defaults
    return r


DEFAULTS = dict(have=[], mis=[], null=[], ep=None, ws="query", sk16=0, sk64=-1, tail=0, query=True)


def _dense(base):
    """The descriptor fields a row leaves out: no activation, residual or deconvolution, dense NHWC output."""
    d = dict(zip(DESC_FIELDS[:12], base))
    return dict(act=0, res_mode=0, out_mode=0, cmod=d["Cout"], out_n_stride=d["OH"] * d["OW"] * d["Cout"], out_h_stride=d["OW"] * d["Cout"],
                out_w_stride=d["Cout"])


def pack_desc(d):
    """[N, H, W, Cin, Cout, KH, KW, stride, pad_t, pad_l, OH, OW] (+ a dict of the other fields where they are not _dense's)."""
    base = [d[f] for f in DESC_FIELDS[:12]]
    extra = {f: d[f] for f, v in _dense(base).items() if d[f] != v}
    return base + [extra] if extra else base


def unpack_desc(p):
    d = dict(zip(DESC_FIELDS[:12], p[:12]))
    d.update(_dense(p[:12]))
    d.update(p[12] if len(p) > 12 else {})
    return d


def operands(r):
    """(operand addresses, epilogue fields or None, workspace address) a row stands for."""
    have = r.get("have", ())
    ptr = {n: ADDR[n] if n in ("x", "w", "out") or n in have else None for n in OPERANDS}
    e = None
    if r.get("ep") is not None:
        e = {n: ADDR["ep_" + n] if n in ("out", "z", "scale", "mean", "rstd") or n in r["ep"]["have"] else None for n in EP_POINTERS}
        e["act"] = r["ep"]["act"]
    ws_addr = ADDR["workspace"]
    for n in r.get("mis", ()):
        if n == "workspace":
            ws_addr += 4
        elif n.startswith("ep_"):
            e[n[3:]] += 4
        else:
            ptr[n] += 4
    for n in r.get("null", ()):
        if n.startswith("ep_"):
            e[n[3:]] = None
        else:
            ptr[n] = None
    return ptr, e, ws_addr


def flat(M, Cin, Cout, **kw):
    """1 x 1 convolution on a 1 x 1 x M map: M output rows exactly."""
    return desc(1, 1, M, Cin, Cout, **kw)


def _trunk_layers(N, rois, mask_rois):
    """(tag, N, H, W, Cin, Cout, k, stride, pad) of ResNet-101 + FPN + RPN + heads at 256 x 256."""
    L = [("stem", N, 256, 256, 3, 64, 7, 2, 3)]
    size, cin = 64, 64
    for stage, (mid, blocks) in enumerate(((64, 3), (128, 4), (256, 23), (512, 3)), 2):
        for b in range(min(blocks, 2)):                     # later blocks repeat the second one's shapes
            s = 2 if (b == 0 and stage > 2) else 1
            t = "res%d%s" % (stage, "ab"[b])
            L.append((t + "_2a", N, size, size, cin, mid, 1, s, "valid"))
            if b == 0:
                L.append((t + "_1", N, size, size, cin, 4 * mid, 1, s, "valid"))
            size //= s
            L += [(t + "_2b", N, size, size, mid, mid, 3, 1, "same"), (t + "_2c", N, size, size, mid, 4 * mid, 1, 1, "valid")]
            cin = 4 * mid
    for lvl, (sz, c) in enumerate(((64, 256), (32, 512), (16, 1024), (8, 2048)), 2):
        L += [("fpn_c%dp%d" % (lvl, lvl), N, sz, sz, c, 256, 1, 1, "valid"), ("fpn_p%d" % lvl, N, sz, sz, 256, 256, 3, 1, "same")]
    for sz in (64, 32, 16, 8, 4):
        L += [("rpn_shared_%d" % sz, N, sz, sz, 256, 512, 3, 1, "same"), ("rpn_class_%d" % sz, N, sz, sz, 512, 6, 1, 1, "valid"),
              ("rpn_bbox_%d" % sz, N, sz, sz, 512, 12, 1, 1, "valid")]
    L += [("class_conv1", rois, 7, 7, 256, 1024, 7, 1, "valid"), ("class_conv2", rois, 1, 1, 1024, 1024, 1, 1, "valid"),
          ("class_logits", rois, 1, 1, 1024, 4, 1, 1, "valid"), ("class_bbox", rois, 1, 1, 1024, 16, 1, 1, "valid"),
          ("mask_conv", mask_rois, 14, 14, 256, 256, 3, 1, "same"), ("mask_deconv", mask_rois, 14, 14, 256, 1024, 1, 1, "valid"),
          ("mask_logits", mask_rois, 28, 28, 256, 4, 1, 1, "valid")]
    return L


def workload_rows():
    rows = []
    for wl, N, rois, mask_rois, sk16 in (("train4", 4, 2048, 2048, 0), ("detect1", 1, 1000, 100, 1), ("detect8", 8, 8000, 800, 1)):
        for tag, n, H, W, Cin, Cout, k, s, pad in _trunk_layers(N, rois, mask_rois):
            name = "%s/%s" % (wl, tag)
            d = desc(n, H, W, Cin, Cout, k, s, pad, act=1)
            rows.append(row(name + "/fwd", d, have=("bias", "scale", "shift", "z_out"), sk16=sk16))
            if "_2c" in tag:
                rows.append(row(name + "/fwd_res", d, have=("bias", "scale", "shift", "z_out", "res"), sk16=sk16, res_mode=1))
            if tag == "mask_deconv":
                rows.append(row(name + "/fwd_deconv2", d, have=("bias",), out_mode=1, cmod=Cout // 4, out_n_stride=28 * 28 * 256,
                                out_h_stride=2 * 28 * 256, out_w_stride=2 * 256))
            if wl != "train4" or s != 1 or tag == "stem":
                continue
            # data gradient (stride 1): the same map, channels swapped, padding k - 1 - pad
            g = desc(n, d["OH"], d["OW"], Cout, Cin, k, 1, "same" if pad == "same" else k - 1 if k > 1 else "valid")
            rows.append(row(name + "/dgrad", g))
            rows.append(row(name + "/dgrad_ep", g, ep=dict(act=1, have=("dgamma", "dbeta"))))
            if "_2a" in tag:        # the block input's gradient: shortcut gradient added, second output for the block below
                rows.append(row(name + "/dgrad_ep_res_dy", g, have=("res",), ep=dict(act=1, have=("dgamma", "dbeta", "dy")), res_mode=1))
    return rows


def rule_rows():
    R = []
    both = lambda name, lo, hi, f, **kw: R.extend([row("%s/%d" % (name, v), f(v), **kw) for v in (lo, hi)])
    # 128-row tiles from CONV_BIG_TILE_MIN_BLOCKS tiles of 128 x 128 on; with K long enough, the DMA split just below
    both("big_tile_blocks", 639, 640, lambda t: flat(t * 128, 64, 128))
    both("big_tile_blocks_k512", 639, 640, lambda t: flat(t * 128, 512, 128))
    both("big_tile_blocks_2cols", 319, 320, lambda t: flat(t * 128, 64, 256))
    # Cout <= 64 / <= 32: 128-row tiles from 256 row tiles on
    both("row_tiles_c64", 255, 256, lambda t: flat(t * 128, 64, 64))
    both("row_tiles_c32", 255, 256, lambda t: flat(t * 128, 64, 32))
    both("row_tiles_c64_ragged", 255 * 128, 255 * 128 + 1, lambda m: flat(m, 64, 64))
    # fewer than 128 tiles of 64 x 128: 64 x 64 tiles
    both("small_bn", 63, 64, lambda t: flat(t * 64, 64, 256))
    both("small_bn_1col", 127, 128, lambda t: flat(t * 64, 64, 128))
    # DMA split: from 96 tiles on, nk16 >= 32 (Cin % 32 == 0 makes nk16 even: 30 / 32), slices towards 768 workgroups capped by
    # nk16 / 16 (the target alone never gives fewer than 2 below 640 tiles)
    both("dma_min_tiles", 95, 96, lambda t: flat(t * 128, 512, 128))
    both("dma_nk16", 480, 512, lambda c: flat(96 * 128, c, 128))
    both("dma_target_2_3", 383, 384, lambda t: flat(t * 128, 2048, 128))
    both("dma_target_cap_nk16", 1024, 2048, lambda c: flat(96 * 128, c, 128))
    both("dma_target_8", 96, 110, lambda t: flat(t * 128, 4096, 128))
    R.append(row("dma_3x3_odd_steps", desc(64, 14, 14, 96, 256, 3, 1, "same")))
    R.append(row("dma_cin_not_32", flat(96 * 128, 528, 128)))
    R.append(row("dma_65_taps", desc(4, 64, 64, 32, 128, 9, 1, "same")))
    # split K below 768 blocks towards 512 workgroups (so: from 511 blocks down), nk >= 8, at most nk / 4 and 16 slices
    both("splitk_blocks", 767, 768, lambda t: flat(t * 128, 256, 64))
    both("splitk_target", 511, 512, lambda t: flat(t * 128, 256, 64))
    both("splitk_nk", 224, 256, lambda c: flat(1024, c, 96))
    both("splitk_nk_ragged", 225, 257, lambda c: flat(1024, c, 96))
    both("splitk_cap_nk4", 1024, 1056, lambda c: flat(64, c, 64))
    both("splitk_cap_16", 2048, 4096, lambda c: flat(64, c, 64))
    both("splitk_want", 170, 171, lambda t: flat(t * 64, 1024, 48))
    # conv_fwd_sk_kernel: 192 .. 512 tiles of 32 x 32, nk >= 16
    for sk16 in (0, 1):
        both("sk_min_tiles/sk16=%d" % sk16, 191, 192, lambda t: flat(t * 32, 512, 32), sk16=sk16)
        both("sk_max_tiles/sk16=%d" % sk16, 512, 513, lambda t: flat(t * 32, 512, 32), sk16=sk16)
        both("sk_min_steps/sk16=%d" % sk16, 480, 512, lambda c: flat(256 * 32, c, 32), sk16=sk16)
        both("sk_3x3/sk16=%d" % sk16, 16, 32, lambda s: desc(1, s, s, 256, 256, 3, 1, "same"), sk16=sk16)
        # conv_fwd_sk16_kernel: 64 .. 2048 tiles of 16 x 16 (Cout % 32 == 0 makes the count even), Ktot >= 256
        both("sk16_min_tiles/sk16=%d" % sk16, 31, 32, lambda t: flat(t * 16, 512, 32), sk16=sk16)
        both("sk16_max_tiles/sk16=%d" % sk16, 1024, 1025, lambda t: flat(t * 16, 256, 32), sk16=sk16)
        both("sk16_max_tiles_k512/sk16=%d" % sk16, 1024, 1025, lambda t: flat(t * 16, 512, 32), sk16=sk16)
        both("sk16_min_k/sk16=%d" % sk16, 224, 256, lambda c: flat(512, c, 64), sk16=sk16)
        R.append(row("sk16_with_epilogue/sk16=%d" % sk16, flat(512, 512, 64), ep=dict(act=1), sk16=sk16))
    # conv_fwd_sk64_kernel: a two-slice plan, 64 .. 512 workgroups unless the key is 1
    for sk64 in (-1, 0, 1):
        both("sk64_min_wgs/sk64=%d" % sk64, 63, 64, lambda t: flat(t * 64, 256, 64), sk64=sk64)
        both("sk64_max_wgs/sk64=%d" % sk64, 32, 33, lambda t: flat(t * 64, 256, 1024), sk64=sk64)
        R.append(row("sk64_513_wgs/sk64=%d" % sk64, flat(27 * 64, 256, 1216), sk64=sk64))
        both("sk64_nk/sk64=%d" % sk64, 480, 512, lambda c: flat(1024, c, 1024), sk64=sk64)
        R.append(row("sk64_three_slices/sk64=%d" % sk64, flat(1024, 384, 1024), sk64=sk64))
        R.append(row("sk64_cout_96/sk64=%d" % sk64, flat(1024, 256, 96), sk64=sk64))
        R.append(row("sk64_stride2/sk64=%d" % sk64, desc(4, 16, 16, 256, 512, 1, 2, "valid"), sk64=sk64))
        R.append(row("sk64_3x3/sk64=%d" % sk64, desc(1, 16, 16, 32, 256, 3, 1, "same"), sk64=sk64))
        R.append(row("sk64_deconv/sk64=%d" % sk64, flat(1024, 256, 1024), sk64=sk64, out_mode=1, cmod=256))
        R.append(row("sk64_epilogue/sk64=%d" % sk64, flat(1024, 1024, 256), have=("res",), ep=dict(act=1, have=("dgamma", "dbeta", "dy")),
                     sk64=sk64, res_mode=1))
        R.append(row("sk64_sk16/sk64=%d" % sk64, flat(256, 256, 1024), sk64=sk64, sk16=1))
    # tail split of the unsplit LDS-DMA kernel, switch on and off
    for tail in (0, 1):
        R.append(row("tail_full_rounds/tail=%d" % tail, flat(1280 * 128, 512, 128), tail=tail))
        R.append(row("tail_short_k/tail=%d" % tail, flat(700 * 128, 480, 256), tail=tail))
        for name, d in (("tail_457", desc(457, 14, 14, 64, 256, 3, 1, "same")), ("tail_200704", desc(1024, 14, 14, 256, 256, 3, 1, "same"))):
            R.append(row("%s/tail=%d" % (name, tail), d, have=("bias", "scale", "shift", "res", "z_out"), tail=tail, res_mode=1))
            R.append(row("%s_ep/tail=%d" % (name, tail), d, ep=dict(act=1, have=("dgamma", "dbeta")), tail=tail))
            R.append(row("%s_ep_dy/tail=%d" % (name, tail), d, ep=dict(act=1, have=("dy",)), tail=tail))
            R.append(row("%s_scalar/tail=%d" % (name, tail), d, have=("bias",), misaligned=("bias",), tail=tail))
            R.append(row("%s_no_ws/tail=%d" % (name, tail), d, workspace=None, tail=tail))
            R.append(row("%s_short_ws/tail=%d" % (name, tail), d, workspace=-16, tail=tail))
            R.append(row("%s_not_dense/tail=%d" % (name, tail), d, tail=tail, out_w_stride=d["Cout"] + 32))
            for m in ("workspace", "out", "ep_out", "ep_z", "ep_scale", "ep_mean", "ep_rstd"):
                R.append(row("%s_ep_misaligned_%s/tail=%d" % (name, m, tail), d, ep=dict(act=1), misaligned=(m,), tail=tail))
    # the other kernel x reduction pairs
    R.append(row("tile_scalar_cout6", desc(1, 8, 8, 512, 6)))
    R.append(row("tile_scalar_ws", flat(1024, 512, 96), misaligned=("workspace",)))
    R.append(row("tile_vec", flat(1024, 512, 96)))
    R.append(row("tile_bwd", flat(1024, 96, 128), ep=dict(act=1)))
    R.append(row("tile_generic_gather", desc(2, 64, 64, 3, 64, 7, 2, 3)))
    R.append(row("tile_x_misaligned", flat(1024, 512, 256), misaligned=("x",)))
    R.append(row("tile_w_misaligned", flat(1024, 512, 256), misaligned=("w",)))
    R.append(row("blds_splitk_vec", flat(96 * 128, 512, 128)))
    R.append(row("blds_splitk_scalar", flat(96 * 128, 512, 128), have=("bias",), misaligned=("bias",)))
    R.append(row("blds_splitk_bwd", flat(96 * 128, 512, 128), ep=dict(act=1, have=("dy",))))
    R.append(row("blds_splitk_x_misaligned", flat(96 * 128, 512, 128), misaligned=("x",)))
    R.append(row("blds", flat(640 * 128, 64, 128)))
    R.append(row("blds_ep", flat(640 * 128, 64, 128), ep=dict(act=1)))
    R.append(row("blds_w_misaligned", flat(640 * 128, 64, 128), misaligned=("w",)))
    R.append(row("glds_x_range", flat(1 << 20, 512, 128)))
    R.append(row("glds_x_range_ep", flat(1 << 20, 512, 128), ep=dict(act=1)))
    R.append(row("glds_shift_range", desc(1, 1023, 1024, 512, 128, 3, 1, "same")))
    R.append(row("dma_split_x_range", desc(1, 1, 96 * 128, 43712, 128, 1, 1, "valid")))
    R.append(row("sk", flat(8192, 512, 32)))
    R.append(row("sk_ep", flat(8192, 512, 32), ep=dict(act=1, have=("dy",))))
    R.append(row("sk_up2", desc(1, 64, 64, 512, 64), have=("res",), res_mode=2))
    R.append(row("sk_strided_out", flat(8192, 512, 32), out_w_stride=64))
    return R


def refusal_rows():
    R = []
    ok = flat(1024, 512, 256)
    R.append(row("arg/no_desc", None))
    for n in ("x", "w", "out"):
        R.append(row("arg/no_" + n, ok, null=(n,)))
    for f in ("N", "H", "W", "Cin", "Cout", "KH", "KW", "stride", "OH", "OW", "cmod"):
        R.append(row("arg/%s_0" % f, ok, **{f: 0}))
        R.append(row("arg/%s_negative" % f, ok, **{f: -1}))
    R.append(row("arg/res_mode_without_res", ok, res_mode=1))
    R.append(row("arg/scale_without_shift", ok, have=("scale",)))
    R.append(row("arg/deconv2_cout", ok, out_mode=1, cmod=128))
    R.append(row("arg/deconv2_res", ok, have=("res",), out_mode=1, cmod=64, res_mode=1))
    R.append(row("arg/up2_odd_oh", desc(1, 7, 8, 64, 64), have=("res",), res_mode=2))
    R.append(row("arg/up2_odd_ow", desc(1, 8, 7, 64, 64), have=("res",), res_mode=2))
    R.append(row("arg/oh_past_input", desc(1, 8, 8, 64, 64), OH=9))
    R.append(row("arg/ow_past_input", desc(1, 8, 8, 64, 64), OW=9))
    R.append(row("arg/m_2_31", desc(1 << 15, 1 << 8, 1 << 8, 32, 32)))
    R.append(row("arg/k_2_31", desc(1, 1, 1, 1, 32), KH=1 << 16, KW=1 << 16, pad_t=1 << 15, pad_l=1 << 15, workspace=None, query=False))
    # backward epilogue: MRCNN_ERR_UNSUPPORTED before MRCNN_ERR_ARG
    split, big = flat(1024, 512, 256), flat(640 * 128, 64, 128)
    R.append(row("ep/no_split_no_dma", desc(4, 14, 14, 128, 256), ep=dict(act=1)))
    R.append(row("ep/cout_96", flat(1024, 512, 96), ep=dict(act=1)))
    R.append(row("ep/cout_8", flat(1024, 512, 8), ep=dict(act=1)))
    R.append(row("ep/dma_dy", big, ep=dict(act=1, have=("dy",))))
    R.append(row("ep/dma_x_misaligned", big, ep=dict(act=1), misaligned=("x",)))
    for name, d in (("split", split), ("dma", big)):
        R.append(row("ep/%s_ok" % name, d, ep=dict(act=1, have=("dgamma", "dbeta", "dbias"))))
        R.append(row("ep/%s_no_workspace" % name, d, ep=dict(act=1), workspace=None))
        R.append(row("ep/%s_short_workspace" % name, d, ep=dict(act=1), workspace=-4))
        R.append(row("ep/%s_not_dense" % name, d, ep=dict(act=1), out_w_stride=d["Cout"] + 4))
        R.append(row("ep/%s_bias" % name, d, have=("bias",), ep=dict(act=1)))
        R.append(row("ep/%s_scale" % name, d, have=("scale", "shift"), ep=dict(act=1)))
        R.append(row("ep/%s_z_out" % name, d, have=("z_out",), ep=dict(act=1)))
        R.append(row("ep/%s_act" % name, d, ep=dict(act=1), act=1))
        R.append(row("ep/%s_res_up2" % name, desc(1, 32, 32, 512, 256) if name == "split" else desc(5, 128, 128, 64, 128), have=("res",),
                     ep=dict(act=1), res_mode=2))
        for m in ("out", "res", "ep_out", "ep_z", "ep_scale", "ep_mean", "ep_rstd", "w", "workspace"):
            R.append(row("ep/%s_misaligned_%s" % (name, m), d, have=("res",), ep=dict(act=1), misaligned=(m,), res_mode=1))
        R.append(row("ep/%s_arg_act_sigmoid" % name, d, ep=dict(act=2)))
        R.append(row("ep/%s_arg_act_negative" % name, d, ep=dict(act=-1)))
        R.append(row("ep/%s_arg_relu_without_out" % name, d, ep=dict(act=1), null=("ep_out",)))
        R.append(row("ep/%s_act_none_without_out" % name, d, ep=dict(act=0), null=("ep_out",)))
        for n in ("z", "mean", "rstd"):
            R.append(row("ep/%s_arg_dgamma_without_%s" % (name, n), d, ep=dict(act=1, have=("dgamma",)), null=("ep_" + n,)))
        R.append(row("ep/%s_arg_dy_misaligned" % name, d, ep=dict(act=1, have=("dy",)), misaligned=("ep_dy",)))
        R.append(row("ep/%s_unsupported_before_arg" % name, d, have=("bias",), ep=dict(act=2)))
    # one operand misaligned at a time: sk, sk64, sk16
    for name, d, kw in (("sk", flat(8192, 512, 32), {}), ("sk64", flat(1024, 256, 1024), {}), ("sk16", flat(512, 512, 64), dict(sk16=1))):
        for m in ("x", "w", "bias", "scale", "shift", "res", "out", "z_out", "workspace"):
            R.append(row("misaligned/%s_%s" % (name, m), d, have=("bias", "scale", "shift", "res", "z_out"), misaligned=(m,), res_mode=1, **kw))
        if name == "sk16":
            continue
        for m in ("ep_out", "ep_z", "ep_scale", "ep_mean", "ep_rstd", "ep_dgamma", "ep_dbeta", "ep_dbias"):
            R.append(row("misaligned/%s_%s" % (name, m), flat(1024, 1024, 256) if name == "sk64" else d, ep=dict(act=1, have=("dgamma", "dbeta", "dbias", "dy")),
                         misaligned=(m,), **kw))
    # workspace: short for a DMA-split plan (planned again without it) and for a plain split plan (runs unsplit), NULL, size 0
    for name, d in (("dma_split", flat(96 * 128, 512, 128)), ("dma_split_k4096", flat(96 * 128, 4096, 128)), ("split", flat(1024, 512, 96)),
                    ("sk", flat(8192, 512, 32)), ("sk64", flat(1024, 256, 1024)), ("unsplit", flat(640 * 128, 64, 128))):
        R.append(row("workspace/%s_short" % name, d, workspace=-4))
        R.append(row("workspace/%s_null" % name, d, workspace=None))
        R.append(row("workspace/%s_zero_bytes" % name, d, workspace=0))
        R.append(row("workspace/%s_of_the_64_row_plan" % name, d, workspace=4 * d["W"] * d["Cout"] * 4))
        R.append(row("workspace/%s_sk16_short" % name, d, workspace=-4, sk16=1))
    return R


def all_rows():
    rows = workload_rows() + rule_rows() + refusal_rows()
    names = [r["name"] for r in rows]
    assert len(set(names)) == len(names), [n for n in names if names.count(n) > 1]
    return rows


# ------------------------------------------------------------------------------------------------
def load(lib_path):
    from caesar_mrcnn_amd import _hip
    lib = C.CDLL(lib_path)
    for name in ("mrcnn_conv2d_fwd_plan", "mrcnn_conv2d_fwd_workspace", "mrcnn_tuning_set"):
        f = getattr(lib, name)
        f.restype, f.argtypes = _hip._SIGNATURES[name]
    return lib


def replay(lib, r):
    """(status, plan fields or None, workspace query) of row r; sets the tuning keys and the tail switch the row names (the caller
    restores them)."""
    from caesar_mrcnn_amd import _hip
    r = dict(DEFAULTS, **r)
    lib.mrcnn_tuning_set(b"sk16", r["sk16"])
    lib.mrcnn_tuning_set(b"sk64", r["sk64"])
    if r["tail"]:
        os.environ["MRCNN_CONV_TAIL_SPLIT"] = "1"
    else:
        os.environ.pop("MRCNN_CONV_TAIL_SPLIT", None)
    d = None
    if r["desc"] is not None:
        d = _hip.ConvDesc()
        for f, v in unpack_desc(r["desc"]).items():
            setattr(d, f, v)
    query = lib.mrcnn_conv2d_fwd_workspace(C.byref(d) if d is not None else None) if r["query"] else 0
    ws = r["ws"]
    ptr, epf, ws_addr = operands(r)
    nbytes = query if ws == "query" else 0 if ws is None else max(query + ws, 0) if ws < 0 else ws
    addr = None if ws is None or (ws == "query" and not query) else ws_addr
    ep = None
    if epf is not None:
        ep = _hip.BwdEpilogue()
        for n in EP_POINTERS + ("act",):
            setattr(ep, n, epf[n])
    plan = _hip.ConvPlan()
    rc = lib.mrcnn_conv2d_fwd_plan(C.byref(d) if d is not None else None, *[ptr[n] for n in OPERANDS], addr, nbytes,
                                   C.byref(ep) if ep is not None else None, C.byref(plan))
    return rc, ({f: getattr(plan, f) for f in PLAN_FIELDS} if rc == 0 else None), query


def read_table(path):
    """The table's rows as row() makes them, with the answers: status, wsq (the workspace query), plan (PLAN_FIELDS in order)."""
    return [dict(opts, name=name, desc=d, status=status, wsq=wsq, plan=plan) for name, d, opts, status, wsq, plan in json.load(open(path))]


def main():
    lib = load(os.path.abspath(sys.argv[1]))
    rows = all_rows()
    for r in rows:
        r["status"], plan, r["wsq"] = replay(lib, r)
        r["plan"] = plan and [plan[f] for f in PLAN_FIELDS]
    os.environ.pop("MRCNN_CONV_TAIL_SPLIT", None)
    with open(sys.argv[2], "w") as f:      # one array per row: name, descriptor, options, then the answers
        f.write("[\n" + ",\n".join(json.dumps([r["name"], r["desc"], {k: r[k] for k in DEFAULTS if k in r}, r["status"], r["wsq"], r["plan"]],
                                              separators=(",", ":")) for r in rows) + "\n]\n")
    by = {}
    for r in rows:
        key = (r["status"], r["plan"] and (r["plan"][0], r["plan"][6]))
        by[key] = by.get(key, 0) + 1
    print(len(rows), "rows;", sorted(by.items(), key=str))


if __name__ == "__main__":
    main()
