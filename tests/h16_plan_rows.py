"""Rows of tests/golden/h16_plan_table.json and their replay through mrcnn_conv2d_fwd_h16_plan / mrcnn_conv2d_wgrad_h16_plan.

A row is the inputs of one 16-bit convolution launch -- forward / data gradient (op "fwd": mrcnn_conv2d_fwd_h16_res, or
mrcnn_conv2d_dgrad_ep_h16 where it has a backward epilogue) or weight gradient (op "wgrad") -- descriptor, operand addresses,
workspace, switches, plus what the library answered: status, the plan's fields, the workspace query.  No GPU: only nullness and
alignment of addresses count.

The committed table was NOT written by the planner it pins.  It was recorded from the launch code as it stood before planning
and launching were separated: in a copy of that tree, hipLaunchKernelGGL inside the three host functions was replaced by a
record (kernel name with its template arguments, grid, block, and the ptiles / mtile0 / ep_vec / dense / fb_act / dbg, resp.
splits / chunk / nk / itiles / ntiles / xcd_order / slab address it passes), read back through one added entry point,
mrcnn_h16_records(buf) -> count, records of {char kernel[96]; unsigned grid, block; long long v[8]}:
    python tests/h16_plan_rows.py <that libmrcnn_hip.so> <table.json> --recorded
`records_to_plan` below turns the records into plan fields.  Without --recorded the table is written from the plan queries of the
library given.  Switches read once per process (MRCNN_H16_SLAB, MRCNN_H16S_EP_VEC, MRCNN_WGRAD_XCD) are asked in child processes.

Rows: every 16-bit convolution of the ResNet-101 + FPN training step with 4 images at 512 x 512 and at 256 x 256 in the widest
mode, enumerated from the architecture, as forward, data gradient, data gradient with epilogue and weight gradient; every case of
tests/test_h16_gpu.py under its switches; both sides of every numeric rule (1 x 1 convolutions on 1 x 1 x M maps give any M);
every refusal; every value of every switch on a shape where it changes the answer and on one where it must not."""
import ctypes as C
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

from conv_plan_rows import desc, flat, pack_desc, unpack_desc  # noqa: E402

OPERANDS = {"fwd": ("x", "w", "bias", "scale", "shift", "res", "out", "z_out"), "wgrad": ("x", "dy", "dw", "workspace")}
REQUIRED = {"fwd": ("x", "w", "out"), "wgrad": ("x", "dy", "dw", "workspace")}
EP_POINTERS = ("out", "z", "scale", "mean", "rstd", "dgamma", "dbeta", "dbias", "dy")
FIELDS = {"fwd": ("kernel", "zout", "grid", "threads", "ptiles", "mtile0", "rem_grid", "rem_mtile0", "ep_vec", "dense", "fused_ep", "trace"),
          # slab_offset: where the slabs start in the (256-byte aligned) workspace = the pixel table's bytes rounded up to 256
          "wgrad": ("kernel", "splits", "chunk", "nk", "itiles", "ntiles", "grid", "reduce", "reduce_grid", "xcd_order", "slab_offset")}
# fake addresses, 256-byte aligned and apart; + 4 misaligns one
ADDR = {n: 0x10000000 * (i + 1) for i, n in enumerate(("x", "w", "bias", "scale", "shift", "res", "out", "z_out", "dy", "dw", "workspace") +
                                                      tuple("ep_" + n for n in EP_POINTERS))}
PER_CALL = ("MRCNN_H16_SMALL", "MRCNN_H16_TILE", "MRCNN_H16_RING", "MRCNN_H16P_NO_SPLIT", "MRCNN_H16P_GRID", "MRCNN_H16W_DBG", "MRCNN_H16P_TRACE",
            "MRCNN_WGRAD_H16_PHASE")
ONCE = ("MRCNN_H16_SLAB", "MRCNN_H16S_EP_VEC", "MRCNN_WGRAD_XCD")
# env: environment switches (PER_CALL and ONCE names); phase / slab: the tuning keys h16_phase / h16_slab
DEFAULTS = dict(op="fwd", dtype=0, have=[], mis=[], null=[], ep=None, ws="query", env={}, phase=1, slab=-1)
TRACE = "0x7f0000001000"


def row(name, d, op="fwd", dtype=0, have=(), misaligned=(), null=(), ep=None, workspace="query", env=None, phase=1, slab=-1, **desc_changes):
    """have: optional operands given (bias, scale, shift, res, z_out); ep: None or dict(act, have): out, z, scale, mean, rstd are
    given unless listed in `null` as ep_<name>.  workspace (wgrad): "query" (the query's answer), bytes, or negative: that many
    bytes short of the query's answer."""
    r = dict(name=name, desc=pack_desc(dict(d, **desc_changes)) if d is not None else None)
    opts = dict(op=op, dtype=dtype, have=list(have), mis=list(misaligned), null=list(null),
                ep=ep and dict(act=ep.get("act", 1), have=list(ep.get("have", ()))), ws=workspace, env=dict(env or {}), phase=phase, slab=slab)
    assert all(k in PER_CALL + ONCE for k in opts["env"]), opts["env"]
    r.update({k: v for k, v in opts.items() if v != DEFAULTS[k]})
    return r


def operands(r):
    op = r.get("op", "fwd")
    have = r.get("have", ())
    ptr = {n: ADDR[n] if n in REQUIRED[op] or n in have else None for n in OPERANDS[op]}
    e = None
    if r.get("ep") is not None:
        e = {n: ADDR["ep_" + n] if n in ("out", "z", "scale", "mean", "rstd") or n in r["ep"]["have"] else None for n in EP_POINTERS}
        e["act"] = r["ep"]["act"]
    for n in r.get("mis", ()):
        if n.startswith("ep_"):
            e[n[3:]] += 4
        else:
            ptr[n] += 4
    for n in r.get("null", ()):
        if n.startswith("ep_"):
            e[n[3:]] = None
        else:
            ptr[n] = None
    return ptr, e


# ---- rows ---------------------------------------------------------------------------------------------------------------------
def dgrad_of(d, k, pad):
    """The data gradient of a stride-1 layer as the forward launch the engine issues: the same map, channels swapped, padding
    k - 1 - pad; a VALID k x k layer on a k x k map (the class head's FC) as one 1 x 1 GEMM over the flattened window."""
    if pad == "valid" and k > 1:
        return desc(d["N"], 1, 1, d["Cout"], k * k * d["Cin"])
    return desc(d["N"], d["OH"], d["OW"], d["Cout"], d["Cin"], k, 1, "same" if pad == "same" else "valid")


def _layers(size, N=4, rois=2048, mask_rois=(2048, 672)):
    """(tag, kind, N, H, W, Cin, Cout, k, stride, pad) of the 16-bit convolutions of ResNet-101 + FPN + RPN + heads on size x size
    images.  kind: 2a / 2b / 2c / c1 (bottleneck), plain (bias only), bn (mask and class heads), deconv."""
    L = []
    s, cin = size // 4, 64
    for stage, (mid, blocks) in enumerate(((64, 3), (128, 4), (256, 23), (512, 3)), 2):
        for b in range(min(blocks, 2)):                     # later blocks repeat the second one's shapes
            st = 2 if (b == 0 and stage > 2) else 1
            t = "res%d%s" % (stage, "ab"[b])
            L.append((t + "_2a", "2a", N, s, s, cin, mid, 1, st, "valid"))
            if b == 0:
                L.append((t + "_1", "c1", N, s, s, cin, 4 * mid, 1, st, "valid"))
            s //= st
            L += [(t + "_2b", "2b", N, s, s, mid, mid, 3, 1, "same"), (t + "_2c", "2c", N, s, s, mid, 4 * mid, 1, 1, "valid")]
            cin = 4 * mid
    for lvl, sz in enumerate((size // 4, size // 8, size // 16, size // 32), 2):
        L.append(("fpn_p%d" % lvl, "plain", N, sz, sz, 256, 256, 3, 1, "same"))
    for sz in (size // 4, size // 8, size // 16, size // 32, size // 64):
        L.append(("rpn_shared_%d" % sz, "plain", N, sz, sz, 256, 512, 3, 1, "same"))
    L += [("class_conv1", "bn", rois, 7, 7, 256, 1024, 7, 1, "valid"), ("class_conv2", "bn", rois, 1, 1, 1024, 1024, 1, 1, "valid")]
    for m in mask_rois:
        L += [("mask_conv_%d" % m, "bn", m, 14, 14, 256, 256, 3, 1, "same"), ("mask_deconv_%d" % m, "deconv", m, 14, 14, 256, 1024, 1, 1, "valid")]
    return L


def engine_rows():
    R = []
    ep = lambda *more: dict(act=1, have=("dgamma", "dbeta", "dbias") + more)
    for size in (512, 256):
        for tag, kind, n, H, W, Cin, Cout, k, st, pad in _layers(size):
            name = "r101_%d/%s" % (size, tag)
            d = desc(n, H, W, Cin, Cout, k, st, pad, act=0 if kind == "c1" else 1)
            if kind == "deconv":
                R.append(row(name + "/fwd", d, have=("bias",), out_mode=1, cmod=Cout // 4, out_w_stride=Cout // 4, out_h_stride=2 * W * Cout // 4,
                             out_n_stride=4 * H * W * Cout // 4))
            elif kind == "plain":
                R.append(row(name + "/fwd", d, have=("bias",)))
            elif kind == "2c":
                R.append(row(name + "/fwd", d, have=("bias", "scale", "shift", "z_out", "res"), res_mode=1))
            else:
                R.append(row(name + "/fwd", d, have=("bias", "scale", "shift", "z_out")))
            R.append(row(name + "/wgrad", desc(n, H, W, Cin, Cout, k, st, pad), op="wgrad"))
            if st != 1:                                      # 1 x 1, stride 2: the product scattered to the even pixels of a zeroed tensor
                g = desc(n, d["OH"], d["OW"], Cout, Cin)
                strides = dict(out_n_stride=H * W * Cin, out_h_stride=2 * W * Cin, out_w_stride=2 * Cin)
                R.append(row(name + "/dgrad_strided", g, **strides))
                R.append(row(name + "/dgrad_strided_res", g, have=("res",), res_mode=1, **strides))
                continue
            g = dgrad_of(d, k, pad)
            R.append(row(name + "/dgrad", g))
            R.append(row(name + "/dgrad_res", g, have=("res",), res_mode=1))
            R.append(row(name + "/dgrad_ep", g, ep=ep()))
            R.append(row(name + "/dgrad_ep_dy", g, ep=ep("dy")))
            R.append(row(name + "/dgrad_ep_res", g, have=("res",), ep=ep(), res_mode=1))
            R.append(row(name + "/dgrad_ep_res_dy", g, have=("res",), ep=ep("dy"), res_mode=1))
    return R


def _tile_switches(tile):
    """What test_h16_gpu's h16_tile fixture sets."""
    return dict(env={"MRCNN_H16_TILE": "phase" if tile == "slab" else tile}, slab=1 if tile == "slab" else 0)


def gpu_case_rows():
    """Every launch of tests/test_h16_gpu.py's kernel tests, with that test's switches.  The combinations test_conv_fwd_h16 and
    test_deconv_and_mask_output_stage_h16 skip are rows too (test_h16_plan_cpu.py looks at what they would take)."""
    import test_h16_gpu as T
    R = []
    fwd_have = lambda bn, z=True: ("bias",) + (("z_out",) if z else ()) + (("scale", "shift") if bn else ())
    for dtype, dn in ((0, "f16"), (1, "bf16")):
        for tile in ("small", "big", "phase", "slab", "wave128"):
            sw = _tile_switches(tile)
            for i, (N, H, W, Cin, Cout, k, pad, act, bn) in enumerate(T.H16_CASES):
                name = "gpu/fwd_h16/%d/%s/%s" % (i, tile, dn)
                d = desc(N, H, W, Cin, Cout, k, 1, pad, act)
                R.append(row(name, d, dtype=dtype, have=fwd_have(bn), **sw))
                if (pad == "same" or k == 1) and Cin % 128 == 0 and not (tile in ("big", "phase", "slab") and Cin % 256):
                    R.append(row(name + "/dgrad", dgrad_of(d, k, pad), dtype=dtype, **sw))
            M, Cd = 37, 256
            R.append(row("gpu/deconv/%s/%s" % (tile, dn), desc(M, 14, 14, 256, 4 * Cd, act=1), dtype=dtype, have=("bias",), out_mode=1, cmod=Cd,
                         out_w_stride=Cd, out_h_stride=2 * 14 * Cd, out_n_stride=4 * 14 * 14 * Cd, **sw))
        for i, (N, H, W, Cin, Cout, act, bn, grid) in enumerate(T.SLAB_CASES):
            env = {"MRCNN_H16_TILE": "phase"}
            if grid:
                env["MRCNN_H16P_GRID"] = str(grid)
            d = desc(N, H, W, Cin, Cout, 3, 1, "same", act)
            R.append(row("gpu/slab/%d/%s" % (i, dn), d, dtype=dtype, have=fwd_have(bn), env=env, slab=1))
            if Cin % 256 == 0 and Cout % 128 == 0:
                R.append(row("gpu/slab/%d/%s/dgrad" % (i, dn), dgrad_of(d, 3, "same"), dtype=dtype, env=env, slab=1))
        for N, H, W, Cin, Cout in ((2048, 14, 14, 256, 256), (4, 128, 128, 256, 256)):
            for tile in ("small", "phase"):
                name = "gpu/full_size/%dx%d/%s/%s" % (N, H, tile, dn)
                R.append(row(name + "/bias_z", desc(N, H, W, Cin, Cout, 3, 1, "same", 1), dtype=dtype, have=("bias", "z_out"), env={"MRCNN_H16_TILE": tile}))
                R.append(row(name + "/plain", desc(N, H, W, Cin, Cout, 3, 1, "same", 0), dtype=dtype, env={"MRCNN_H16_TILE": tile}))
        for mode in ("0", "1"):
            R.append(row("gpu/full_size/wgrad/%s/%s" % (mode, dn), desc(2048, 14, 14, 256, 256, 3, 1, "same"), op="wgrad", dtype=dtype,
                         env={"MRCNN_WGRAD_H16_PHASE": mode}))
        for i, (N, H, W, Cin, Cout, k, pad) in enumerate(T.WGRAD_H16_CASES):
            for kernel, mode in (("table", "0"), ("phase", "2")):
                R.append(row("gpu/wgrad/%d/%s/%s" % (i, kernel, dn), desc(N, H, W, Cin, Cout, k, 1, pad), op="wgrad", dtype=dtype,
                             env={"MRCNN_WGRAD_H16_PHASE": mode}))
        small = {"MRCNN_H16_SMALL": "1"}
        for i, (N, H, W, Cin, Cout, k, st, pad, act, bn, res) in enumerate(T.SMALL_CASES):
            d = desc(N, H, W, Cin, Cout, k, st, pad, act, 1 if res else 0)
            R.append(row("gpu/small/%d/%s" % (i, dn), d, dtype=dtype, have=fwd_have(bn) + (("res",) if res else ()), env=small))
            if k == 1 and st == 2:
                R.append(row("gpu/small/%d/%s/dgrad_strided" % (i, dn), desc(N, d["OH"], d["OW"], Cout, Cin), dtype=dtype, env=small,
                             out_n_stride=H * W * Cin, out_h_stride=2 * W * Cin, out_w_stride=2 * Cin))
        for k, cin, cout, res in ((1, 1024, 256, False), (3, 256, 256, False), (1, 256, 1024, True), (3, 64, 64, False)):
            d = desc(3, 13, 11, cin, cout, k, 1, "same" if k > 1 else "valid", 0, 1 if res else 0)
            have = ("res",) if res else ()
            R.append(row("gpu/dgrad_ep/%d_%d_%d/%s" % (k, cin, cout, dn), d, dtype=dtype, have=have, env=small, ep=dict(act=1, have=("dgamma", "dbeta", "dbias", "dy"))))
            R.append(row("gpu/dgrad_ep/%d_%d_%d/%s/two_launches" % (k, cin, cout, dn), d, dtype=dtype, have=have, env=small))
    return R


def both(R, name, lo, hi, f, **kw):
    R.extend([row("%s/%d" % (name, v), f(v), **kw) for v in (lo, hi)])


def rule_rows():
    """Both sides of every numeric rule; the planner sees 256 CUs without a device."""
    R = []
    # large tiles from 384 workgroups of 256 x 128 on, where both tile classes can take the shape
    both(R, "large_wgs", 383, 384, lambda t: flat(t * 256, 64, 128))
    both(R, "large_wgs_2cols", 191, 192, lambda t: flat(t * 256, 64, 256))
    both(R, "large_wgs_ragged", 383 * 256, 383 * 256 + 1, lambda m: flat(m, 64, 128))
    # the phased kernel from one full round of 256 x 256 tiles on
    both(R, "big_tiles", 255, 256, lambda t: flat(t * 256, 64, 256))
    both(R, "big_tiles_2cols", 127, 128, lambda t: flat(t * 256, 64, 512))
    both(R, "big_tiles_ragged", 255 * 256, 255 * 256 + 1, lambda m: flat(m, 64, 256))
    # a partial last round of at most half the CUs goes to the small tile; the deconvolution never splits
    both(R, "split_half_round", 384, 385, lambda t: flat(t * 256, 64, 256))
    both(R, "split_half_round_2cols", 192, 193, lambda t: flat(t * 256, 64, 512))
    both(R, "split_one_tile", 256, 257, lambda t: flat(t * 256, 64, 256))
    both(R, "split_second_round", 512 + 128, 512 + 129, lambda t: flat(t * 256, 64, 256))
    both(R, "split_ragged_rows", 384 * 256 - 255, 384 * 256 + 1, lambda m: flat(m, 64, 256))
    both(R, "split_deconv", 96, 97, lambda t: flat(t * 256, 256, 1024, act=1), have=("bias",), out_mode=1, cmod=256)
    both(R, "split_no_split_switch", 384, 385, lambda t: flat(t * 256, 64, 256), env={"MRCNN_H16P_NO_SPLIT": "1"})
    # phased: Cout <= 512 (the deconvolution: cmod <= 512), Cin % 64, at most 31 taps, activation none / ReLU, output below 4 GiB
    both(R, "phase_cout", 512, 768, lambda c: flat(256 * 256, 64, c))
    for c in (512, 640):
        R.append(row("phase_deconv_cmod/%d" % c, flat(64 * 256, 64, 4 * c), out_mode=1, cmod=c))
    for t in (31, 32):
        R.append(row("phase_taps/%d" % t, flat(256 * 256, 64, 256), env={"MRCNN_H16_TILE": "phase"}, KW=t, pad_l=t // 2))
    R.append(row("taps/64", flat(1024, 64, 128), KH=8, KW=8, pad_t=4, pad_l=4))
    R.append(row("taps/65", flat(1024, 64, 128), KH=5, KW=13, pad_t=2, pad_l=6))
    both(R, "phase_act", 1, 2, lambda a: flat(256 * 256, 64, 256, act=a))
    both(R, "phase_out_bytes", (1 << 23) - 256, 1 << 23, lambda m: flat(m, 64, 256))
    # channel gates: Cin % 32 / 64 / 128 / 256 and Cout % 64 / 128 / 256, below and above the large-tile threshold, by the rules and
    # with the phased / slab / big / wave128 tiles asked for
    for cin in (32, 48, 64, 96, 128, 192, 256):
        for cout in (64, 96, 128, 192, 256, 384):
            R.append(row("gate/few_rows/%d_%d" % (cin, cout), flat(1024, cin, cout)))
            R.append(row("gate/many_rows/%d_%d" % (cin, cout), flat(256 * 256, cin, cout)))
            for tile in ("phase", "slab", "big", "wave128"):
                R.append(row("gate/%s/%d_%d" % (tile, cin, cout), desc(64, 14, 14, cin, cout, 3, 1, "same"), **_tile_switches(tile)))
    # slab form: maps no wider than 14 pixels, 3 x 3 / stride 1 / pad 1
    sl = dict(env={"MRCNN_H16_TILE": "phase"}, slab=1)
    both(R, "slab_width", 14, 15, lambda w: desc(64, 14, w, 256, 256, 3, 1, "same"), **sl)
    R.append(row("slab_5x5", desc(64, 14, 14, 256, 256, 5, 1, "same"), **sl))
    R.append(row("slab_1x1", desc(64, 14, 14, 256, 256), **sl))
    R.append(row("slab_valid", desc(64, 14, 14, 256, 256, 3, 1, "valid"), **sl))
    R.append(row("slab_stride2", desc(64, 14, 14, 256, 256, 3, 2, "same"), **sl))
    R.append(row("slab_cout_768", desc(64, 14, 14, 256, 768, 3, 1, "same"), **sl))
    R.append(row("slab_z_out", desc(64, 14, 14, 256, 256, 3, 1, "same"), have=("bias", "z_out"), **sl))
    # byte ranges of the forward: rows below 2^31, x (with the padding shift) and w below 0x7FFFFFF0 bytes
    both(R, "range_x", (1 << 22) - 1, 1 << 22, lambda m: flat(m, 256, 128))
    both(R, "range_x_shift", 1022, 1023, lambda h: desc(1, h, 1024, 1024, 128, 3, 1, "same"))
    both(R, "range_w", 32640, 32768, lambda c: flat(64, 32768, c))
    R.append(row("range_m", desc(1 << 15, 1 << 8, 1 << 8, 32, 128)))
    # weight gradient, phased kernel: chunk >= 2048 rows, tiles * splits * 2 >= CUs, at most 64 splits
    wg = dict(op="wgrad")
    both(R, "wgrad/phase_chunk", 64 * 2048 - 64 * 64, 64 * 2048, lambda m: flat(m, 512, 256), **wg)
    both(R, "wgrad/phase_half_chip", 256, 512, lambda c: flat(64 * 2048, c, 256), **wg)
    both(R, "wgrad/phase_half_chip_forced", 256, 512, lambda c: flat(64 * 2048, c, 256), env={"MRCNN_WGRAD_H16_PHASE": "2"}, **wg)
    both(R, "wgrad/phase_split_cap", 1024, 1280, lambda c: flat(1 << 18, c, 256), **wg)                 # 256 / 4 = 64 splits, 256 / 5 = 51
    both(R, "wgrad/phase_ragged_split", 64 * 2048 + 1, 64 * 2048 + 64 * 64 + 1, lambda m: flat(m, 512, 256), **wg)
    R.append(row("wgrad/phase_many_tiles", desc(2048, 14, 14, 512, 512, 3, 1, "same"), **wg))            # 36 tiles: 7 splits
    R.append(row("wgrad/phase_more_tiles_than_cus", desc(2048, 14, 14, 1024, 1024, 5, 1, "same"), **wg))
    R.append(row("wgrad/phase_stride2", desc(64, 28, 28, 256, 256, 1, 2, "valid"), **wg))
    R.append(row("wgrad/phase_valid_3x3", desc(2048, 14, 14, 256, 256, 3, 1, "valid"), **wg))
    R.append(row("wgrad/phase_cout_128", flat(64 * 2048, 512, 128), **wg))
    R.append(row("wgrad/phase_pad_past_kernel", desc(2048, 14, 14, 512, 256, 3, 1, "same"), pad_t=3, **wg))
    R.append(row("wgrad/phase_negative_pad", desc(2048, 14, 14, 512, 256, 3, 1, "same"), pad_l=-1, **wg))
    # table kernel: splits towards 768 workgroups (12 tiles: 64 splits), at most 64, at most one per 512 rows
    for a, b in ((11, 1), (3, 4), (13, 1), (1, 1), (40, 8)):
        R.append(row("wgrad/table_tiles_%d" % (a * b), flat(1 << 16, 256 * a, 128 * b), env={"MRCNN_WGRAD_H16_PHASE": "0"}, **wg))
    both(R, "wgrad/table_rows_cap", 512 * 10, 512 * 10 + 1, lambda m: flat(m, 512, 128), **wg)
    both(R, "wgrad/table_one_split", 1, 513, lambda m: flat(m, 256, 128), **wg)
    # the 16-byte reduction needs n % 4 == 0 (always: Cin % 256 == 0) and dw aligned
    R.append(row("wgrad/reduce_scalar_table", flat(4096, 512, 128), misaligned=("dw",), **wg))
    R.append(row("wgrad/reduce_scalar_not_phased", flat(64 * 2048, 512, 256), misaligned=("dw",), **wg))
    R.append(row("wgrad/workspace_misaligned", flat(64 * 2048, 512, 256), misaligned=("workspace",), **wg))
    # byte ranges: rows below 2^30, x (with the shift) and dy below 0x7FFFFF00 bytes
    both(R, "wgrad/range_x", (1 << 22) - 1, 1 << 22, lambda m: flat(m, 256, 128), **wg)
    both(R, "wgrad/range_dy", (1 << 20) - 1, 1 << 20, lambda m: flat(m, 256, 1024), **wg)
    both(R, "wgrad/range_x_shift", 1022, 1023, lambda h: desc(1, h, 1024, 1024, 128, 3, 1, "same"), **wg)
    R.append(row("wgrad/range_m", desc(1 << 14, 1 << 8, 1 << 8, 256, 128), **wg))
    return R


def refusal_rows():
    R = []
    ok = flat(4096, 256, 256)
    R.append(row("arg/no_desc", None))
    for n in ("x", "w", "out"):
        R.append(row("arg/no_" + n, ok, null=(n,)))
    R.append(row("arg/dtype_2", ok, dtype=2))
    R.append(row("arg/dtype_negative", ok, dtype=-1))
    for f in ("N", "H", "W", "Cin", "Cout", "KH", "KW", "stride", "OH", "OW"):
        R.append(row("arg/%s_0" % f, ok, **{f: 0}))
        R.append(row("arg/%s_negative" % f, ok, **{f: -1}))
    R.append(row("arg/res_up2", ok, have=("res",), res_mode=2))
    R.append(row("arg/res_mode_without_res", ok, res_mode=1))
    R.append(row("arg/res_without_res_mode", ok, have=("res",)))
    R.append(row("arg/cin_48", flat(4096, 48, 256)))
    R.append(row("arg/cout_96", flat(4096, 64, 96)))
    R.append(row("arg/cin_32_cout_64", flat(4096, 32, 64)))
    R.append(row("arg/large_with_res", flat(4096, 32, 128), have=("res",), res_mode=1))
    R.append(row("arg/large_strided", flat(4096, 32, 128), out_w_stride=256))
    R.append(row("arg/small_switched_off", flat(4096, 64, 64), env={"MRCNN_H16_SMALL": "0"}))
    R.append(row("arg/deconv2_cout", ok, out_mode=1, cmod=128))
    R.append(row("arg/deconv2_cmod_64", ok, out_mode=1, cmod=64))
    R.append(row("arg/deconv2_z_out", flat(4096, 256, 512), have=("z_out",), out_mode=1, cmod=128))
    R.append(row("arg/out_mode_2", ok, out_mode=2))
    R.append(row("arg/cmod", ok, cmod=128))
    R.append(row("arg/cmod_small", flat(4096, 64, 64), cmod=32))
    R.append(row("arg/scale_without_shift", ok, have=("scale",)))
    R.append(row("ok/shift_without_scale", ok, have=("shift",)))
    for n in ("x", "w"):
        R.append(row("arg/misaligned_" + n, ok, misaligned=(n,)))
    # the other operands may be misaligned: the 16-byte epilogue (and the wave128 tile) then stay off
    for name, d, kw in (("small", flat(4096, 64, 64), {}), ("large", flat(256 * 256, 256, 256), {}),
                        ("wave128", flat(256 * 256, 256, 256), dict(env={"MRCNN_H16_TILE": "wave128"}))):
        for n in ("bias", "scale", "shift", "res", "out", "z_out"):
            have = ("bias", "scale", "shift", "z_out") + (("res",) if name == "small" else ())
            if n in have:
                R.append(row("ok/%s_misaligned_%s" % (name, n), d, have=have, misaligned=(n,), res_mode=1 if name == "small" else 0, **kw))
    for f in ("out_n_stride", "out_h_stride", "out_w_stride"):
        R.append(row("ok/small_%s_not_8" % f, flat(4096, 64, 64), **{f: 64 * 4096 + 4 if f != "out_w_stride" else 68}))
    # backward epilogue: its own argument checks first, then MRCNN_ERR_ARG of the call, then MRCNN_ERR_UNSUPPORTED
    for name, d in (("small", flat(4096, 256, 64)), ("large", flat(256 * 256, 256, 256))):
        e = dict(act=1, have=("dgamma", "dbeta", "dbias"))
        R.append(row("ep/%s_ok" % name, d, ep=e))
        R.append(row("ep/%s_act_none_without_out" % name, d, ep=dict(act=0), null=("ep_out",)))
        R.append(row("ep/%s_arg_act_sigmoid" % name, d, ep=dict(act=2)))
        R.append(row("ep/%s_arg_act_negative" % name, d, ep=dict(act=-1)))
        R.append(row("ep/%s_arg_relu_without_out" % name, d, ep=dict(act=1), null=("ep_out",)))
        for n in ("z", "mean", "rstd"):
            R.append(row("ep/%s_arg_dgamma_without_%s" % (name, n), d, ep=dict(act=1, have=("dgamma",)), null=("ep_" + n,)))
        R.append(row("ep/%s_arg_before_unsupported" % name, d, ep=dict(act=2), stride=2))
        R.append(row("ep/%s_arg_no_x" % name, d, ep=e, null=("x",)))
        R.append(row("ep/%s_arg_misaligned_w" % name, d, ep=e, misaligned=("w",)))
        R.append(row("ep/%s_unsupported_not_dense" % name, d, ep=e, out_w_stride=2 * d["Cout"]))
        R.append(row("ep/%s_unsupported_act" % name, d, ep=e, act=1))
        R.append(row("ep/%s_unsupported_stride" % name, desc(4, 32, 32, 256, d["Cout"], 1, 2), ep=e))
        for n in ("res", "out", "ep_out", "ep_z", "ep_dy"):
            R.append(row("ep/%s_misaligned_%s" % (name, n), d, have=("res",), ep=dict(act=1, have=("dy",)), misaligned=(n,), res_mode=1))
    R.append(row("ep/unsupported_cin_96", flat(256 * 256, 96, 128), ep=dict(act=1)))
    R.append(row("ep/unsupported_cin_32", flat(256 * 256, 32, 256), ep=dict(act=1)))
    R.append(row("ep/unsupported_deconv2", flat(4096, 256, 512), ep=dict(act=1), out_mode=1, cmod=128))
    # weight gradient
    wg = dict(op="wgrad")
    okw = flat(4096, 256, 128)
    R.append(row("wgrad/arg/no_desc", None, **wg))
    for n in ("x", "dy", "dw", "workspace"):
        R.append(row("wgrad/arg/no_" + n, okw, null=(n,), **wg))
    R.append(row("wgrad/arg/dtype_2", okw, dtype=2, **wg))
    for f in ("N", "H", "W", "Cin", "Cout", "KH", "KW", "stride", "OH", "OW"):
        R.append(row("wgrad/arg/%s_0" % f, okw, **dict(wg, **{f: 0})))
        R.append(row("wgrad/arg/%s_negative" % f, okw, **dict(wg, **{f: -1})))
    R.append(row("wgrad/arg/taps_65", okw, KH=5, KW=13, **wg))
    R.append(row("wgrad/ok/taps_64", okw, KH=8, KW=8, **wg))
    R.append(row("wgrad/arg/cin_128", flat(4096, 128, 128), **wg))
    R.append(row("wgrad/arg/cout_64", flat(4096, 256, 64), **wg))
    for n in ("x", "dy"):
        R.append(row("wgrad/arg/misaligned_" + n, okw, misaligned=(n,), **wg))
    for name, d in (("table", okw), ("phase", flat(64 * 2048, 512, 256))):
        R.append(row("wgrad/workspace/%s_short" % name, d, workspace=-1, **wg))
        R.append(row("wgrad/workspace/%s_zero_bytes" % name, d, workspace=0, **wg))
        R.append(row("wgrad/workspace/%s_exact" % name, d, **wg))
        R.append(row("wgrad/workspace/%s_ample" % name, d, workspace=1 << 40, **wg))
        # the requirement covers either kernel's slabs: with the phased kernel switched off it is the table kernel's alone
        R.append(row("wgrad/workspace/%s_short_phase_off" % name, d, workspace=-1, env={"MRCNN_WGRAD_H16_PHASE": "0"}, **wg))
        R.append(row("wgrad/workspace/%s_short_phase_forced" % name, d, workspace=-1, env={"MRCNN_WGRAD_H16_PHASE": "2"}, **wg))
    return R


def switch_rows():
    """Every value of every switch, on a shape where it changes the answer and on one where it must not."""
    R = []
    mask = desc(64, 14, 14, 256, 256, 3, 1, "same", 1)               # 49 tiles of 256 x 256: the 256 x 128 tile by the rules
    mask_full = desc(2048, 14, 14, 256, 256, 3, 1, "same", 1)        # 1568 tiles: phased by the rules, 32 of them left for the small tile
    trunk = desc(4, 32, 32, 256, 256, 3, 1, "same", 1)               # 16 x 2 large workgroups: the small tile by the rules
    narrow = flat(256 * 256, 32, 128)                                # large tiles only
    only_small = flat(4096, 64, 64)
    shapes = (("mask", mask), ("mask_full", mask_full), ("trunk", trunk), ("narrow", narrow), ("only_small", only_small))
    z = ("bias", "z_out")
    for sn, d in shapes:
        for v in (None, "0", "1", "2"):
            R.append(row("switch/small=%s/%s" % (v, sn), d, have=z, env={"MRCNN_H16_SMALL": v} if v else None))
        for v in ("big", "small", "ring", "phase", "wave128", "other", ""):
            R.append(row("switch/tile=%s/%s" % (v, sn), d, have=z, env={"MRCNN_H16_TILE": v}))
        R.append(row("switch/ring/%s" % sn, d, have=z, env={"MRCNN_H16_RING": "1"}))
        R.append(row("switch/ring_tile_small/%s" % sn, d, have=z, env={"MRCNN_H16_RING": "1", "MRCNN_H16_TILE": "small"}))
        R.append(row("switch/ring_tile_big/%s" % sn, d, have=z, env={"MRCNN_H16_RING": "0", "MRCNN_H16_TILE": "big"}))
        R.append(row("switch/no_split/%s" % sn, d, have=z, env={"MRCNN_H16P_NO_SPLIT": "1"}))
        R.append(row("switch/no_split_tile_phase/%s" % sn, d, have=z, env={"MRCNN_H16P_NO_SPLIT": "0", "MRCNN_H16_TILE": "phase"}))
        for g in ("1", "5", "256", "1000"):
            R.append(row("switch/grid=%s/%s" % (g, sn), d, have=z, env={"MRCNN_H16P_GRID": g}))
            R.append(row("switch/grid=%s_tile_phase/%s" % (g, sn), d, have=z, env={"MRCNN_H16P_GRID": g, "MRCNN_H16_TILE": "phase"}))
        for v in ("1", "2", "3"):
            R.append(row("switch/wave_dbg=%s/%s" % (v, sn), d, have=z, env={"MRCNN_H16W_DBG": v}))
            R.append(row("switch/wave_dbg=%s_wave128/%s" % (v, sn), d, have=z, env={"MRCNN_H16W_DBG": v, "MRCNN_H16_TILE": "wave128"}))
        R.append(row("switch/trace/%s" % sn, d, have=z, env={"MRCNN_H16P_TRACE": TRACE}))
        R.append(row("switch/trace_tile_phase/%s" % sn, d, have=z, env={"MRCNN_H16P_TRACE": TRACE, "MRCNN_H16_TILE": "phase"}))
        for key in (0, 1):
            R.append(row("switch/h16_phase=%d/%s" % (key, sn), d, have=z, phase=key))
            R.append(row("switch/h16_phase=%d_tile_phase/%s" % (key, sn), d, have=z, phase=key, env={"MRCNN_H16_TILE": "phase"}))
        for envv in (None, "0", "1"):
            for key in (-1, 0, 1):
                env = {"MRCNN_H16_SLAB": envv} if envv else {}
                R.append(row("switch/slab_env=%s_key=%d/%s" % (envv, key, sn), d, have=z, slab=key, env=env))
                R.append(row("switch/slab_env=%s_key=%d_tile_phase/%s" % (envv, key, sn), d, have=z, slab=key, env=dict(env, MRCNN_H16_TILE="phase")))
        for v in ("0", "1"):
            R.append(row("switch/ep_vec=%s/%s" % (v, sn), d, have=z, env={"MRCNN_H16S_EP_VEC": v}))
            R.append(row("switch/ep_vec=%s_out_misaligned/%s" % (v, sn), d, have=z, misaligned=("out",), env={"MRCNN_H16S_EP_VEC": v}))
    R.append(row("switch/ep_vec=0/dgrad_ep", trunk, ep=dict(act=1, have=("dy",)), env={"MRCNN_H16S_EP_VEC": "0"}, act=0))
    R.append(row("switch/slab_env=1/width_15", desc(2048, 15, 15, 256, 256, 3, 1, "same"), env={"MRCNN_H16_SLAB": "1"}))
    # weight gradient
    wg = dict(op="wgrad")
    wshapes = (("mask_full", mask_full), ("mask", mask), ("cout_128", desc(2048, 14, 14, 256, 128, 3, 1, "same")), ("refused", flat(4096, 128, 128)))
    for sn, d in wshapes:
        for v in (None, "0", "1", "2", "3"):
            R.append(row("switch/wgrad_phase=%s/%s" % (v, sn), d, env={"MRCNN_WGRAD_H16_PHASE": v} if v else None, **wg))
        for v in ("0", "1", "2"):
            R.append(row("switch/wgrad_xcd=%s/%s" % (v, sn), d, env={"MRCNN_WGRAD_XCD": v}, **wg))
            R.append(row("switch/wgrad_xcd=%s_table/%s" % (v, sn), d, env={"MRCNN_WGRAD_XCD": v, "MRCNN_WGRAD_H16_PHASE": "0"}, **wg))
    return R


def all_rows():
    rows = engine_rows() + gpu_case_rows() + rule_rows() + refusal_rows() + switch_rows()
    names = [r["name"] for r in rows]
    assert len(set(names)) == len(names), [n for n in names if names.count(n) > 1][:8]
    return rows


# ---- asking a library -----------------------------------------------------------------------------------------------------------
class Record(C.Structure):
    _fields_ = [("kernel", C.c_char * 96), ("grid", C.c_uint), ("block", C.c_uint), ("v", C.c_longlong * 8)]


def load(lib_path, recorded=False):
    from caesar_mrcnn_amd import _hip
    lib = C.CDLL(lib_path)
    names = ["mrcnn_conv2d_wgrad_h16_workspace", "mrcnn_tuning_set"]
    names += ["mrcnn_conv2d_fwd_h16_res", "mrcnn_conv2d_dgrad_ep_h16", "mrcnn_conv2d_wgrad_h16"] if recorded else \
        ["mrcnn_conv2d_fwd_h16_plan", "mrcnn_conv2d_wgrad_h16_plan"]
    for name in names:
        f = getattr(lib, name)
        f.restype, f.argtypes = _hip._SIGNATURES[name]
    if recorded:
        lib.mrcnn_h16_records.restype, lib.mrcnn_h16_records.argtypes = C.c_int, [C.POINTER(Record)]
    return lib


_FWD_KERNELS = {"conv_fwd_h16s_kernel<T>": (0, 0), "conv_fwd_h16_kernel<T,2,2,2>": (1, 0), "conv_fwd_h16_kernel<T,3,2,2>": (2, 0),
                "conv_fwd_h16_kernel<T,4,2,4>": (3, 0), "conv_fwd_h16_kernel<T,4,2,2,4>": (4, 0), "conv_fwd_h16p_kernel<T,false,false>": (5, 0),
                "conv_fwd_h16p_kernel<T,true,false>": (5, 1), "conv_fwd_h16p_kernel<T,false,true>": (6, 0), "conv_fwd_h16q_kernel<T,false>": (7, 0),
                "conv_fwd_h16q_kernel<T,true>": (7, 1)}             # -> (MRCNN_H16_*, ZOUT)


def _kernel_name(rec, dtype):
    k = rec.kernel.decode().replace(" ", "").strip("()")
    t = "_Float16" if dtype == 0 else "__bf16"
    assert t in k or "<" not in k, (k, dtype)
    return k.replace(t, "T")


def records_to_plan(op, recs, dtype, ws_addr):
    """Plan fields from the launch records of the code as it stood before the planner."""
    if op == "fwd":
        first, rest = recs[0], recs[1:]
        kernel, zout = _FWD_KERNELS[_kernel_name(first, dtype)]
        ptiles, mtile0, ep_vec, dense, fb_act, dbg = list(first.v)[:6]
        plan = dict(kernel=kernel, zout=zout, grid=first.grid, threads=first.block, ptiles=ptiles, mtile0=mtile0, rem_grid=0, rem_mtile0=0,
                    ep_vec=ep_vec, dense=dense, fused_ep=int(fb_act >= 0), trace=dbg)
        if rest:                                              # the small-tile launch for the partial last round: same arguments but mtile0
            (r,) = rest
            assert _kernel_name(r, dtype) == "conv_fwd_h16s_kernel<T>" and r.block == 256 and kernel in (5, 7), r.kernel
            assert [r.v[i] for i in (0, 2, 3, 4, 5)] == [first.v[i] for i in (0, 2, 3, 4, 5)]
            plan.update(rem_grid=r.grid, rem_mtile0=r.v[1])
        return plan
    names = [_kernel_name(r, dtype) for r in recs]
    assert names[-1] in ("wgrad_h16_reduce_kernel", "wgrad_h16_reduce_vec_kernel") and recs[-1].block == 256, names
    red, k = recs[-1], recs[-2]
    base = (ws_addr + 255) & ~255
    plan = dict(splits=red.v[1], chunk=k.v[1], grid=k.grid, reduce=int(names[-1] == "wgrad_h16_reduce_vec_kernel"), reduce_grid=red.grid,
                xcd_order=k.v[5], slab_offset=k.v[6] - base)
    assert red.v[2] == k.v[6]                                   # the reduction reads the slabs the kernel wrote
    if names[-2] == "conv_wgrad_h16p_kernel<T>":
        assert len(recs) == 2 and k.block == 512
        plan.update(kernel=1, nk=k.v[2], itiles=k.v[3], ntiles=k.v[4])
    else:
        assert names[:2] == ["pixel_table_kernel", "conv_wgrad_h16_kernel<T>"] and len(recs) == 3 and k.block == 256 and k.v[0] == red.v[1]
        assert k.v[7] == base
        plan.update(kernel=0, nk=0, itiles=0, ntiles=0)
    return plan


def replay(lib, r, recorded=False):
    """(status, plan fields or None, workspace query or None) of row r; sets the per-call switches and the tuning keys the row names
    (the caller restores them).  Switches read once per process must already be in the environment: see `answers`."""
    from caesar_mrcnn_amd import _hip
    r = dict(DEFAULTS, **r)
    op, dtype = r["op"], r["dtype"]
    for k in PER_CALL:
        if k in r["env"]:
            os.environ[k] = r["env"][k]
        else:
            os.environ.pop(k, None)
    assert all(os.environ.get(k) == r["env"].get(k) for k in ONCE), "once-per-process switches differ from the row's"
    lib.mrcnn_tuning_set(b"h16_phase", r["phase"])
    lib.mrcnn_tuning_set(b"h16_slab", r["slab"])
    d = None
    if r["desc"] is not None:
        d = _hip.ConvDesc()
        for f, v in unpack_desc(r["desc"]).items():
            setattr(d, f, v)
    dref = C.byref(d) if d is not None else None
    ptr, epf = operands(r)
    ep = None
    if epf is not None:
        ep = _hip.BwdEpilogueH16(grad_multiplier=1.0)
        for n in EP_POINTERS + ("act",):
            setattr(ep, n, epf[n])
    if op == "fwd":
        query = None
        if not recorded:
            plan = _hip.H16Plan()
            rc = lib.mrcnn_conv2d_fwd_h16_plan(dref, dtype, *[ptr[n] for n in OPERANDS["fwd"]], C.byref(ep) if ep is not None else None, C.byref(plan))
        elif ep is None:
            rc = lib.mrcnn_conv2d_fwd_h16_res(dref, dtype, *[ptr[n] for n in OPERANDS["fwd"]], None)
        else:
            assert not any(ptr[n] for n in ("bias", "scale", "shift", "z_out")), "mrcnn_conv2d_dgrad_ep_h16 has no such operand"
            rc = lib.mrcnn_conv2d_dgrad_ep_h16(dref, dtype, ptr["x"], ptr["w"], ptr["res"], ptr["out"], C.byref(ep), None)
    else:
        query = lib.mrcnn_conv2d_wgrad_h16_workspace(dref)
        ws = r["ws"]
        nbytes = query if ws == "query" else max(query + ws, 0) if ws < 0 else ws
        if not recorded:
            plan = _hip.H16WgradPlan()
            rc = lib.mrcnn_conv2d_wgrad_h16_plan(dref, dtype, ptr["x"], ptr["dy"], ptr["dw"], ptr["workspace"], nbytes, C.byref(plan))
        else:
            rc = lib.mrcnn_conv2d_wgrad_h16(dref, dtype, ptr["x"], ptr["dy"], ptr["dw"], ptr["workspace"], nbytes, 0, 1.0, None)
    if recorded:
        buf = (Record * 8)()
        recs = [buf[i] for i in range(lib.mrcnn_h16_records(buf))]
        assert bool(recs) == (rc == 0), (r["name"], rc, len(recs))
        return rc, (records_to_plan(op, recs, dtype, ptr.get("workspace")) if rc == 0 else None), query
    if rc != 0:
        return rc, None, query
    if op == "fwd":
        return rc, {f: getattr(plan, f) for f in FIELDS["fwd"]}, query
    assert plan.workspace_bytes == query and plan.slab_bytes == plan.splits * d.KH * d.KW * d.Cin * d.Cout * 4, r["name"]
    assert plan.table_bytes + plan.slab_bytes + 512 <= plan.workspace_bytes
    got = {f: getattr(plan, f) for f in FIELDS["wgrad"][:-1]}
    got["slab_offset"] = (plan.table_bytes + 255) & ~255
    return rc, got, query


def _once(r):
    return tuple(sorted((k, v) for k, v in r.get("env", {}).items() if k in ONCE))


def answers(lib_path, rows, recorded=False, lib=None):
    """[(status, plan, query)] of rows: in this process where a row names no once-per-process switch (they must be unset here), in
    one child process per setting of those otherwise."""
    assert not any(k in os.environ for k in ONCE), "unset %s" % (ONCE,)
    out = [None] * len(rows)
    groups = {}
    for i, r in enumerate(rows):
        groups.setdefault(_once(r), []).append(i)
    for once, idx in groups.items():
        if not once:
            lib = lib or load(lib_path, recorded)
            got = [replay(lib, rows[i], recorded) for i in idx]
        else:
            cmd = [sys.executable, os.path.abspath(__file__), "--child", lib_path] + (["--recorded"] if recorded else [])
            p = subprocess.run(cmd, input=json.dumps([rows[i] for i in idx]), env=dict(os.environ, **dict(once)), capture_output=True, text=True)
            assert p.returncode == 0, p.stderr[-3000:]
            got = [tuple(a) for a in json.loads(p.stdout)]
        for i, a in zip(idx, got):
            out[i] = a
    for k in PER_CALL:
        os.environ.pop(k, None)
    if lib is not None:
        lib.mrcnn_tuning_set(b"h16_phase", 1)
        lib.mrcnn_tuning_set(b"h16_slab", -1)
    return out


def read_table(path):
    """The table's rows as row() makes them, with the answers: status, plan (FIELDS[op] in order, or None), wsq."""
    return [dict(opts, name=name, desc=d, status=status, plan=plan, wsq=wsq) for name, d, opts, status, plan, wsq in json.load(open(path))]


def main():
    if sys.argv[1] == "--child":
        lib = load(sys.argv[2], "--recorded" in sys.argv)
        print(json.dumps([replay(lib, r, "--recorded" in sys.argv) for r in json.load(sys.stdin)]))
        return
    recorded = "--recorded" in sys.argv
    rows = all_rows()
    by = {}
    for r, (status, plan, wsq) in zip(rows, answers(os.path.abspath(sys.argv[1]), rows, recorded)):
        op = r.get("op", "fwd")
        r["status"], r["wsq"], r["plan"] = status, wsq, plan and [plan[f] for f in FIELDS[op]]
        key = (op, status, plan and (plan["kernel"], plan["reduce"] if op == "wgrad" else plan["rem_grid"] > 0))
        by[key] = by.get(key, 0) + 1
    with open(sys.argv[2], "w") as f:      # one array per row: name, descriptor, options, then the answers
        f.write("[\n" + ",\n".join(json.dumps([r["name"], r["desc"], {k: r[k] for k in DEFAULTS if k in r}, r["status"], r["plan"], r["wsq"]],
                                              separators=(",", ":")) for r in rows) + "\n]\n")
    print(len(rows), "rows;", sorted(by.items(), key=str))


if __name__ == "__main__":
    main()
