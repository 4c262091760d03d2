"""Rows of tests/golden/wgrad_plan_table.json and their replay through mrcnn_conv2d_wgrad_plan / mrcnn_conv2d_wgrad_multi_plan.

A row is the inputs of one float32 weight-gradient launch -- mrcnn_conv2d_wgrad (one descriptor) or mrcnn_conv2d_wgrad_multi (a
list of them) --: descriptors, operand addresses, workspace, the flat-addressing switch, plus what the library answered: status,
the plan's fields, the workspace query.  No GPU: only nullness and alignment of addresses count.

The committed table was NOT written by the planner it pins.  It was recorded from the launch code as it stood before planning and
launching were separated: in a copy of that tree, hipLaunchKernelGGL inside the host section of csrc/conv_wgrad.hip was replaced
by a record (kernel name with its template arguments, grid, block, dynamic LDS, and the arguments the kernel gets: out / table /
slab addresses, splits, chunk, fast, the first / rfirst prefixes), read back through one added entry point,
mrcnn_wgrad_records(buf) -> count, records of {char kernel[96]; unsigned grid, block; long long lds, v[160]}:
    python tests/wgrad_plan_rows.py <that libmrcnn_hip.so> <table.json> --recorded
with MRCNN_WGRAD_MIN_PIXELS and MRCNN_WGRAD_MULTI_TARGET (overrides that code still read) unset and the tuning key wgrad_lds_pad
at 0.  `records_to_plan` below turns the records into plan fields.  Without --recorded the table is written from the plan queries
of the library given.  MRCNN_CONV_FLAT_GLDS is read once per process: its rows are asked in a child process.

Rows: every weight gradient of the ResNet-101 + FPN training step with four images at 256 x 256, enumerated from the architecture,
as a single launch, the groups engine.wgrad_group forms and the transform-domain GEMM batches ops.conv2d_wgrad_winograd forms;
both sides of every numeric rule (1 x 1 convolutions on 1 x 1 maps give any M); every workspace and pointer state; every refusal."""
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

from conv_plan_rows import ADDR as _ADDR, _trunk_layers, desc, pack_desc, unpack_desc  # noqa: E402

# the address scheme of conv_plan_rows (256-byte aligned and apart; + 4 misaligns one); problem g of a multi launch 1 MiB further
ADDR = dict(x=_ADDR["x"], dy=_ADDR["res"], dw=_ADDR["out"], workspace=_ADDR["workspace"])
PROBLEM_STEP = 1 << 20
FIELDS = {"single": ("kernel", "bi", "bn", "fast", "splits", "chunk", "grid", "table_grid", "reduce", "reduce_grid", "lds_bytes",
                     # where the pixel table starts behind the workspace address given (-1: no table) = the slabs' bytes rounded up
                     "table_offset"),
          # per problem; slab_offset -1 where a problem has one split (it writes dw)
          "multi": ("grid", "reduce_grid", "splits", "chunk", "slab_offset", "first", "rfirst")}
MULTI_MAX = 16
# mis / null: operands ("x", "dy", "dw", "workspace"; a multi row: "<g>.x" ... and "workspace"); ws: "query" (the query's answer),
# None (no workspace), bytes, or negative: that many bytes short of the query's answer; flat: MRCNN_CONV_FLAT_GLDS set;
# query False: the workspace query is not asked (OH or OW <= 0: the code the table was recorded from divides by zero there)
DEFAULTS = dict(op="single", mis=[], null=[], ws="query", flat=False, query=True)


def row(name, d, op="single", misaligned=(), null=(), workspace="query", flat=False, query=True, **desc_changes):
    """d: a descriptor (single), a list of descriptors (multi), or None."""
    if d is None:
        packed = None
    elif op == "single":
        packed = pack_desc(dict(d, **desc_changes))
    else:
        assert not desc_changes
        packed = [pack_desc(q) for q in d]
    r = dict(name=name, desc=packed)
    opts = dict(op=op, mis=list(misaligned), null=list(null), ws=workspace, flat=flat, query=query)
    r.update({k: v for k, v in opts.items() if v != DEFAULTS[k]})
    return r


def gemm(M, Cin, Cout, **kw):
    """1 x 1 convolution on M maps of 1 x 1: M output pixels exactly, x of M * Cin floats (what the multi launch calls a pure GEMM)."""
    return desc(M, 1, 1, Cin, Cout, **kw)


def wide(M, Cin, Cout, **kw):
    """The same M pixels as one 1 x M map: no pure GEMM."""
    return desc(1, 1, M, Cin, Cout, **kw)


# ---- rows ---------------------------------------------------------------------------------------------------------------------
def _step_layers():
    return [(tag, desc(n, H, W, Cin, Cout, k, s, pad)) for tag, n, H, W, Cin, Cout, k, s, pad in _trunk_layers(4, 2048, 2048)]


def _wino_batches(d, tile):
    """[(nb, T)] per tile group of ops.winograd_groups(H, W, tile): nb transform-domain GEMMs of T rows each."""
    N, H, W = d["N"], d["H"], d["W"]
    if tile == 2:
        groups = [(2, 2, H // 2, W // 2)]
    elif tile == 4:
        groups = [(4, 4, (H + 3) // 4, (W + 3) // 4)]
    else:
        groups = [(4, 4, H // 4, W // 4), (4, 2, H // 4, 1), (2, 4, 1, W // 4), (2, 2, 1, 1)]
    return [((oth + 2) * (otw + 2), N * th * tw) for oth, otw, th, tw in groups]


def workload_rows():
    R = []
    layers = _step_layers()
    by_tag = dict(layers)
    for tag, d in layers:
        R.append(row("train4/%s" % tag, d))
    # engine.wgrad_group: a bottleneck block's 2c, 2b, 2a (and the first block's shortcut, stride 2 from res3 on); the FPN's four
    # smoothing and four lateral convolutions; _bwd_group's direct layers beside Winograd ones (two of a block)
    for stage in (2, 3, 4, 5):
        for b in "ab":
            t = "res%d%s" % (stage, b)
            group = [by_tag[t + "_2c"], by_tag[t + "_2b"], by_tag[t + "_2a"]] + ([by_tag[t + "_1"]] if b == "a" else [])
            R.append(row("train4/group/%s" % t, group, op="multi"))
            R.append(row("train4/group/%s_2c_2a" % t, [group[0], group[2]], op="multi"))
    R.append(row("train4/group/fpn_smooth", [by_tag["fpn_p%d" % l] for l in (5, 4, 3, 2)], op="multi"))
    R.append(row("train4/group/fpn_lateral", [by_tag["fpn_c%dp%d" % (l, l)] for l in (2, 3, 4, 5)], op="multi"))
    # ops.conv2d_wgrad_winograd: per tile group nb GEMMs [T, Cin]^T [T, Cout], 16 per launch for F(2x2), 12 for the others; a
    # batch the shared launch refuses goes one by one
    seen = set()
    for tag, d in layers:
        if not (d["KH"] == 3 and d["stride"] == 1 and d["pad_t"] == 1 and d["H"] % 2 == 0 and d["Cin"] % 16 == 0 and d["Cout"] % 128 == 0):
            continue
        tiles = (2, 4) + (("mixed",) if d["H"] % 4 == 2 and d["W"] % 4 == 2 and d["H"] > 4 else ())
        for tile in tiles:
            for gi, (nb, T) in enumerate(_wino_batches(d, tile)):
                per = 16 if nb == 16 else 12
                g = gemm(T, d["Cin"], d["Cout"])
                R.append(row("train4/winograd/%s/tile_%s/group_%d/%dx%d" % (tag, tile, gi, per, T), [g] * per, op="multi"))
                key = (T, d["Cin"], d["Cout"])
                if key not in seen:
                    seen.add(key)
                    R.append(row("train4/winograd_gemm/%d_%d_%d" % key, g))
    return R


def both(R, name, lo, hi, f, **kw):
    R.extend([row("%s/%d" % (name, v), f(v), **kw) for v in (lo, hi)])


def rule_rows():
    R = []
    # tile rows: 128 with Cin % 128 == 0, else 64, inside one tap (fast) with Cin % 64 == 0; tile columns 32 / 64 / 128 by Cout;
    # the LDS-DMA kernel with Cin % 128 == 0 and Cout % 128 == 0
    for cin in (128, 64, 192, 96, 32, 3, 256):
        for cout in (31, 32, 63, 64, 127, 128, 129, 192, 256):
            R.append(row("tile/%d_%d" % (cin, cout), wide(1024, cin, cout)))
            R.append(row("tile/%d_%d/3x3" % (cin, cout), desc(2, 9, 7, cin, cout, 3, 1, "same")))
    # pixel splits: 1024 workgroups over the tiles ...
    both(R, "split/target_2_1", 4096, 4224, lambda c: wide(4096, c, 2048))                  # 512 tiles: 2, 528 tiles: 1
    both(R, "split/target_3_2", 341 * 128, 342 * 128, lambda c: wide(4096, c, 128))
    R.append(row("split/more_tiles_than_target", wide(4096, 4224, 4096)))                   # 1056 tiles: one split, no reduction
    R.append(row("split/tile_kernel_target", wide(4096, 2048 + 64, 96)))                    # 33 x 2 tiles of 64 x 64
    # ... at least 128 pixels per split ...
    both(R, "split/pixel_cap_3_4", 384, 385, lambda m: gemm(m, 128, 128))
    both(R, "split/pixel_cap_1_2", 128, 129, lambda m: gemm(m, 128, 128))
    R.append(row("split/one_pixel", gemm(1, 128, 128)))
    R.append(row("split/pixel_cap_tile_kernel", wide(300, 64, 64)))
    # ... at most 64 ...
    both(R, "split/cap_64", 63 * 128, 64 * 128, lambda m: gemm(m, 128, 128))
    both(R, "split/cap_64_above", 64 * 128 + 1, 65 * 128, lambda m: gemm(m, 128, 128))
    # ... of whole 32-pixel steps, which can lower the count: 8256 pixels in 64 splits of 129 -> 52 chunks of 160
    R.append(row("split/chunk_rounding_64_52", gemm(64 * 129, 128, 128)))
    R.append(row("split/chunk_rounding_tile_kernel", wide(64 * 129, 64, 64)))
    both(R, "split/chunk_rounding_ragged", 429, 430, lambda m: gemm(m, 128, 128))
    # the pixel table: from 65536 pixels on, at most 64 taps, LDS-DMA shapes only
    both(R, "table/pixels", 65535, 65536, lambda m: wide(m, 128, 128))
    both(R, "table/pixels_gemm", 65535, 65536, lambda m: gemm(m, 128, 128))
    both(R, "table/pixels_cout_64", 65535, 65536, lambda m: wide(m, 128, 64))
    both(R, "table/pixels_cin_64", 65535, 65536, lambda m: wide(m, 64, 128))
    R.append(row("table/3x3", desc(459, 13, 11, 128, 128, 3, 1, "same")))
    R.append(row("table/stride2", desc(4, 256, 256, 128, 256, 1, 2, "valid")))
    for m in (1024, 65536):
        R.append(row("table/taps_64/%d" % m, wide(m, 128, 128), KH=8, KW=8, pad_t=4, pad_l=4))
        R.append(row("table/taps_65/%d" % m, wide(m, 128, 128), KH=5, KW=13, pad_t=2, pad_l=6))
    R.append(row("table/one_split", gemm(65536, 4224, 4096)))
    # buffer range: x bytes + padding shift + 16 pixel rows, and dy bytes, below 0x7FFFFFF0; else flat addressing
    both(R, "range/x", 4194287, 4194288, lambda m: gemm(m, 128, 128))                       # 512 m + 8192 against 2147483632
    both(R, "range/x_shift", 0, 1, lambda p: dict(gemm(4194287, 128, 128), pad_l=p))
    both(R, "range/x_shift_rows", 0, 1, lambda p: dict(gemm(4194287, 128, 128), pad_t=p))
    both(R, "range/dy", 2097151, 2097152, lambda m: gemm(m, 128, 256))
    both(R, "range/x_3x3", 240, 241, lambda h: desc(1, h, 1024, 128, 128, 3, 1, "same"))
    both(R, "range/x_tile_kernel", 4194287, 4194288, lambda m: gemm(m, 64, 128))           # no LDS-DMA shape: the range is not asked
    R.append(row("range/out_one_split", gemm(131072, 4224, 4096)))
    # pixels below 2^31
    both(R, "range/pixels", (1 << 15) - 1, 1 << 15, lambda n: desc(n, 1 << 8, 1 << 8, 32, 32))
    both(R, "range/pixels_dma_shape", (1 << 15) - 1, 1 << 15, lambda n: desc(n, 1 << 8, 1 << 8, 128, 128))
    # the shared launch: the pixel-table limit with its pure-GEMM exception, taps, range, shapes, problem counts
    ok = desc(4, 16, 16, 256, 256, 3, 1, "same")
    multi = dict(op="multi")
    both(R, "multi/pixels", 65535, 65536, lambda m: [ok, wide(m, 128, 128)], **multi)
    both(R, "multi/pixels_gemm", 65535, 65536, lambda m: [ok, gemm(m, 128, 128)], **multi)
    R.append(row("multi/gemm_3x3_taps", [ok, dict(gemm(70000, 128, 128), KH=3, KW=3)], **multi))
    R.append(row("multi/gemm_stride2", [ok, dict(gemm(70000, 128, 128), stride=2)], **multi))
    R.append(row("multi/gemm_h2", [ok, desc(35000, 2, 1, 128, 128)], **multi))
    both(R, "multi/range_x", 4194287, 4194288, lambda m: [ok, gemm(m, 128, 128)], **multi)
    both(R, "multi/range_dy", 2097151, 2097152, lambda m: [gemm(m, 128, 256), ok], **multi)
    R.append(row("multi/taps_64", [ok, dict(wide(1024, 128, 128), KH=8, KW=8, pad_t=4, pad_l=4)], **multi))
    R.append(row("multi/taps_65", [ok, dict(wide(1024, 128, 128), KH=5, KW=13, pad_t=2, pad_l=6)], **multi))
    for name, bad in (("cout_64", wide(1024, 128, 64)), ("cout_192", wide(1024, 128, 192)), ("cin_64", wide(1024, 64, 128)),
                      ("cin_192", wide(1024, 192, 128)), ("cin_3", desc(4, 32, 32, 3, 128, 7, 2, 3))):
        for pos in (0, 1, 2):
            group = [ok, ok]
            group.insert(pos, bad)
            R.append(row("multi/unfit_%s/at_%d" % (name, pos), group, **multi))
    for n in (0, 1, 2, 15, 16, 17):
        R.append(row("multi/n_%d" % n, [gemm(1024, 128, 128)] * n, **multi))
    R.append(row("multi/n_16_mixed", [ok, gemm(300, 256, 128), desc(4, 32, 32, 256, 512, 1, 2, "valid"), gemm(100, 128, 128)] * 4, **multi))
    R.append(row("multi/no_problems", None, **multi))
    # its splits: 1024 workgroups over the tiles of ALL problems, then per problem the rule above
    R.append(row("multi/split/one_each", [gemm(100, 128, 128), gemm(128, 256, 128)], **multi))
    R.append(row("multi/split/one_and_many", [gemm(100, 128, 128), gemm(5000, 256, 128)], **multi))
    R.append(row("multi/split/target_1", [gemm(5000, 4224, 2048), gemm(5000, 128, 128)], **multi))
    R.append(row("multi/split/target_2", [gemm(5000, 4096, 1024), gemm(5000, 4096, 1024)], **multi))
    R.append(row("multi/split/cap_64", [gemm(64 * 129, 128, 128), gemm(65 * 128, 128, 128)], **multi))
    R.append(row("multi/split/pixel_cap", [gemm(384, 128, 128), gemm(385, 128, 128), gemm(129, 128, 128)], **multi))
    return R


def state_rows():
    """Workspace and pointer states; every refusal."""
    R = []
    shapes = (("tile", wide(1024, 64, 64)), ("tile_cout_6", wide(1024, 512, 6)), ("tile_odd", wide(1024, 3, 6)),        # 18 floats of dW: no 16-byte sum
              ("tile_one_split", wide(100, 64, 64)), ("blds", gemm(1024, 128, 128)), ("blds_one_split", gemm(100, 128, 128)),
              ("table", wide(65536, 128, 128)), ("table_one_split", gemm(65536, 4224, 4096)),
              ("glds", gemm(4194288, 128, 128)), ("glds_one_split", gemm(131072, 4224, 4096)))
    for name, d in shapes:
        R.append(row("ws/%s/query" % name, d))
        R.append(row("ws/%s/null" % name, d, workspace=None))
        R.append(row("ws/%s/zero_bytes" % name, d, workspace=0))
        R.append(row("ws/%s/one_short" % name, d, workspace=-1))
        R.append(row("ws/%s/ample" % name, d, workspace=1 << 40))
        R.append(row("ws/%s/misaligned" % name, d, misaligned=("workspace",)))
        R.append(row("ws/%s/misaligned_ample" % name, d, misaligned=("workspace",), workspace=1 << 40))
        R.append(row("ptr/%s/dw_misaligned" % name, d, misaligned=("dw",)))
        R.append(row("ptr/%s/dw_and_workspace_misaligned" % name, d, misaligned=("dw", "workspace")))
        for n in ("x", "dy"):
            R.append(row("ptr/%s/%s_misaligned" % (name, n), d, misaligned=(n,)))
        for n in ("x", "dy", "dw"):
            R.append(row("ptr/%s/no_%s" % (name, n), d, null=(n,)))
    # 64 slabs of 128 x 128 floats = 4194304 bytes, then the table: exactly the slabs runs without the table, one byte less is refused
    R.append(row("ws/table/slabs_exactly", wide(65536, 128, 128), workspace=4194304))
    R.append(row("ws/table/slabs_one_short", wide(65536, 128, 128), workspace=4194303))
    R.append(row("ws/table/slabs_exactly_misaligned", wide(65536, 128, 128), workspace=4194304, misaligned=("workspace",)))
    ok = wide(1024, 128, 128)
    R.append(row("arg/no_desc", None))
    for f in ("N", "H", "W", "Cin", "Cout", "KH", "KW", "stride", "OH", "OW"):
        for v, vn in ((0, "0"), (-1, "negative")):
            R.append(row("arg/%s_%s" % (f, vn), ok, query=f not in ("OH", "OW"), **{f: v}))
            R.append(row("arg/%s_%s/tile_kernel" % (f, vn), wide(1024, 64, 64), query=f not in ("OH", "OW"), **{f: v}))
    R.append(row("arg/before_workspace", ok, null=("x",), workspace=None))
    R.append(row("arg/misaligned_before_workspace", ok, misaligned=("dy",), workspace=None))
    # the shared launch: workspace states, then per problem a missing pointer (MRCNN_ERR_ARG) or a misaligned one (unsupported),
    # the first problem in order decides
    multi = dict(op="multi")
    groups = (("splits", [gemm(1024, 128, 128), desc(4, 16, 16, 256, 256, 3, 1, "same"), gemm(100, 128, 128)]),
              ("one_split_each", [gemm(100, 128, 128), gemm(128, 256, 128)]))
    for name, g in groups:
        R.append(row("multi/ws/%s/query" % name, g, **multi))
        R.append(row("multi/ws/%s/null" % name, g, workspace=None, **multi))
        R.append(row("multi/ws/%s/zero_bytes" % name, g, workspace=0, **multi))
        R.append(row("multi/ws/%s/slabs_exactly" % name, g, workspace=-256, **multi))
        R.append(row("multi/ws/%s/slabs_one_short" % name, g, workspace=-257, **multi))
        R.append(row("multi/ws/%s/misaligned" % name, g, misaligned=("workspace",), **multi))
        for q in range(len(g)):
            for n in ("x", "dy", "dw"):
                R.append(row("multi/ptr/%s/no_%d.%s" % (name, q, n), g, null=("%d.%s" % (q, n),), **multi))
                R.append(row("multi/ptr/%s/misaligned_%d.%s" % (name, q, n), g, misaligned=("%d.%s" % (q, n),), **multi))
        R.append(row("multi/ptr/%s/misaligned_0_then_null_1" % name, g, misaligned=("0.dw",), null=("1.x",), **multi))
        R.append(row("multi/ptr/%s/null_0_then_misaligned_1" % name, g, null=("0.dy",), misaligned=("1.x",), **multi))
        R.append(row("multi/ptr/%s/null_after_short_workspace" % name, g, null=("0.x",), workspace=0, **multi))
    g = groups[0][1]
    for f in ("N", "H", "W", "Cin", "Cout", "KH", "KW", "stride", "OH", "OW"):
        for v, vn in ((0, "0"), (-1, "negative")):
            R.append(row("multi/arg/%s_%s" % (f, vn), [g[0], dict(g[1], **{f: v}), g[2]], **multi))
    return R


def flat_rows():
    """MRCNN_CONV_FLAT_GLDS: the LDS-DMA shapes take the flat-addressed kernel, the others what they took; the shared launch
    refuses while its query answers."""
    R = []
    kw = dict(flat=True)
    for name, d in (("gpu_script_shape", desc(90, 13, 11, 128, 256, 3, 1, "same")), ("blds", gemm(1024, 128, 128)), ("blds_one_split", gemm(100, 128, 128)),
                    ("table", wide(65536, 128, 128)), ("table_one_split", gemm(65536, 4224, 4096)), ("out_of_range", gemm(4194288, 128, 128)),
                    ("tile", wide(1024, 64, 64)), ("tile_cout_192", wide(1024, 128, 192))):
        R.append(row("flat/%s" % name, d, **kw))
        R.append(row("flat/%s/dw_misaligned" % name, d, misaligned=("dw",), **kw))
        R.append(row("flat/%s/no_workspace" % name, d, workspace=None, **kw))
    ok = desc(4, 16, 16, 256, 256, 3, 1, "same")
    R.append(row("flat/multi", [ok, gemm(1024, 128, 128)], op="multi", **kw))
    R.append(row("flat/multi_one_split_each", [gemm(100, 128, 128)] * 2, op="multi", **kw))
    R.append(row("flat/multi_unfit", [ok, wide(1024, 128, 64)], op="multi", **kw))
    R.append(row("flat/multi_no_x", [ok, ok], op="multi", null=("0.x",), **kw))
    return R


def all_rows():
    rows = workload_rows() + rule_rows() + state_rows() + flat_rows()
    names = [r["name"] for r in rows]
    assert len(set(names)) == len(names), [n for n in names if names.count(n) > 1][:8]
    return rows


# ---- asking a library -----------------------------------------------------------------------------------------------------------
class Record(C.Structure):
    _fields_ = [("kernel", C.c_char * 96), ("grid", C.c_uint), ("block", C.c_uint), ("lds", C.c_longlong), ("v", C.c_longlong * 160)]


def load(lib_path, recorded=False):
    from caesar_mrcnn_amd import _hip
    lib = C.CDLL(lib_path)
    names = ["mrcnn_conv2d_wgrad_workspace", "mrcnn_conv2d_wgrad_multi_workspace", "mrcnn_tuning_set"]
    names += ["mrcnn_conv2d_wgrad", "mrcnn_conv2d_wgrad_multi"] if recorded else ["mrcnn_conv2d_wgrad_plan", "mrcnn_conv2d_wgrad_multi_plan"]
    for name in names:
        f = getattr(lib, name)
        f.restype, f.argtypes = _hip._SIGNATURES[name]
    if recorded:
        lib.mrcnn_wgrad_records.restype, lib.mrcnn_wgrad_records.argtypes = C.c_int, [C.POINTER(Record)]
    return lib


_TILES = {"conv_wgrad_kernel<%d,%d,%d,%d>" % t: t for t in ((128, 128, 2, 2), (128, 64, 2, 2), (128, 32, 4, 1), (64, 128, 2, 2), (64, 64, 2, 2), (64, 32, 2, 1))}
_REDUCE = {"wgrad_reduce_kernel": 1, "wgrad_reduce_vec_kernel": 2}


def _name(rec):
    return rec.kernel.decode().replace(" ", "").strip("()").replace("WGRAD_BP", "16")


def records_to_plan(op, recs, ptr, ws_addr, n_floats):
    """Plan fields from the launch records of the code as it stood before the planner.  ptr: the operand addresses given;
    n_floats: KH*KW*Cin*Cout (per problem for a multi row)."""
    names = [_name(r) for r in recs]
    if op == "multi":
        k = recs[0]
        assert names[0] == "conv_wgrad_blds_multi_kernel<16>" and k.block == 256 and k.lds == 0 and k.v[159] == 0, names
        n = k.v[0]
        per = [list(k.v[1 + 6 * g:7 + 6 * g]) for g in range(n)]              # out, splits, chunk, x_shift, x_records, dw
        for g, (out, splits, chunk, _, _, dw) in enumerate(per):
            assert dw == ptr[g]["dw"] and (out == dw if splits == 1 else out >= ws_addr), (g, per[g])
        first, rfirst = list(k.v[97:114]), list(k.v[114:131])
        assert first[n] == k.grid
        plan = dict(grid=k.grid, reduce_grid=0, splits=[p[1] for p in per], chunk=[p[2] for p in per],
                    slab_offset=[p[0] - ws_addr if p[1] > 1 else -1 for p in per], first=first, rfirst=rfirst)
        if len(recs) > 1:
            (r,) = recs[1:]
            assert names[1] == "wgrad_reduce_multi_kernel" and r.block == 256 and r.lds == 0 and list(r.v) == list(k.v) and r.grid == rfirst[n]
            plan["reduce_grid"] = r.grid
        else:
            assert rfirst[n] == 0
        return plan
    plan = dict(table_grid=0, table_offset=-1, reduce=0, reduce_grid=0)
    if names[0] == "pixel_table_kernel":
        t, recs, names = recs[0], recs[1:], names[1:]
        assert t.block == 256 and t.lds == 0 and names[0] == "conv_wgrad_blds_kernel<16,true>" and t.v[0] == recs[0].v[1] and t.v[0] % 256 == 0
        plan.update(table_grid=t.grid, table_offset=t.v[0] - ws_addr)
    k = recs[0]
    out, table, splits, chunk, fast = list(k.v[:5])
    if names[0] in _TILES:
        bi, bn, wm, wn = _TILES[names[0]]
        assert k.block == wm * wn * 64 and k.lds == 0
        plan.update(kernel=0, bi=bi, bn=bn)
    else:
        kernel = {"conv_wgrad_blds_kernel<16,false>": 1, "conv_wgrad_blds_kernel<16,true>": 2, "conv_wgrad_glds_kernel<128,128,16>": 3}[names[0]]
        assert k.block == 256 and (table != 0) == (kernel == 2) == (plan["table_grid"] > 0), names
        plan.update(kernel=kernel, bi=128, bn=128)
    plan.update(fast=fast, splits=splits, chunk=chunk, grid=k.grid, lds_bytes=k.lds)
    assert out == (ptr["workspace"] if splits > 1 else ptr["dw"]), (out, splits)
    if splits > 1:
        (r,) = recs[1:]
        vec = _REDUCE[names[1]]
        assert r.block == 256 and r.lds == 0 and r.v[0] == ptr["workspace"] and r.v[1] == ptr["dw"] and r.v[3] == splits
        assert r.v[2] == (n_floats // 4 if vec == 2 else n_floats)
        plan.update(reduce=vec, reduce_grid=r.grid)
    else:
        assert len(recs) == 1
    return plan


def _desc(packed):
    from caesar_mrcnn_amd import _hip
    d = _hip.ConvDesc()
    for f, v in unpack_desc(packed).items():
        setattr(d, f, v)
    return d


def _workspace(r, query):
    ws = r["ws"]
    addr = None if ws is None else ADDR["workspace"] + (4 if "workspace" in r["mis"] else 0)
    nbytes = (query or 0) if ws == "query" else 0 if ws is None else max((query or 0) + ws, 0) if ws < 0 else ws
    return addr, nbytes


def replay(lib, r, recorded=False):
    """(status, plan fields or None, workspace query or None) of row r.  MRCNN_CONV_FLAT_GLDS must already be what the row says:
    see `answers`."""
    from caesar_mrcnn_amd import _hip
    r = dict(DEFAULTS, **r)
    assert ("MRCNN_CONV_FLAT_GLDS" in os.environ) == r["flat"], "the flat switch is read once per process"
    lib.mrcnn_tuning_set(b"wgrad_lds_pad", 0)
    op = r["op"]
    if op == "single":
        d = _desc(r["desc"]) if r["desc"] is not None else None
        dref = C.byref(d) if d is not None else None
        query = lib.mrcnn_conv2d_wgrad_workspace(dref) if r["query"] else None
        ptr = {n: ADDR[n] + (4 if n in r["mis"] else 0) for n in ("x", "dy", "dw")}
        ptr.update({n: None for n in r["null"]})
        ptr["workspace"], nbytes = _workspace(r, query)
        if recorded:
            rc = lib.mrcnn_conv2d_wgrad(dref, ptr["x"], ptr["dy"], ptr["dw"], ptr["workspace"], nbytes, 0, None)
        else:
            plan = _hip.WgradPlan()
            rc = lib.mrcnn_conv2d_wgrad_plan(dref, ptr["x"], ptr["dy"], ptr["dw"], ptr["workspace"], nbytes, C.byref(plan))
        n_floats = d.KH * d.KW * d.Cin * d.Cout if d is not None else 0
    else:
        n = len(r["desc"]) if r["desc"] is not None else 1
        arr = (_hip.WgradProblem * max(n, 1))()
        ptr = []
        for g in range(n if r["desc"] is not None else 0):
            q = arr[g]
            q.d = _desc(r["desc"][g])
            p = {k: ADDR[k] + g * PROBLEM_STEP + (4 if "%d.%s" % (g, k) in r["mis"] else 0) for k in ("x", "dy", "dw")}
            p.update({k: None for k in ("x", "dy", "dw") if "%d.%s" % (g, k) in r["null"]})
            q.x, q.dy, q.dw = p["x"], p["dy"], p["dw"]
            ptr.append(p)
        aref = arr if r["desc"] is not None else None
        n = len(r["desc"]) if r["desc"] is not None else 1
        query = lib.mrcnn_conv2d_wgrad_multi_workspace(aref, n)
        ws_addr, nbytes = _workspace(r, query)
        if recorded:
            rc = lib.mrcnn_conv2d_wgrad_multi(aref, n, ws_addr, nbytes, None)
        else:
            plan = _hip.WgradMultiPlan()
            rc = lib.mrcnn_conv2d_wgrad_multi_plan(aref, n, ws_addr, nbytes, C.byref(plan))
    if recorded:
        buf = (Record * 8)()
        recs = [buf[i] for i in range(lib.mrcnn_wgrad_records(buf))]
        assert bool(recs) == (rc == 0), (r["name"], rc, len(recs))
        if rc != 0:
            return rc, None, query
        if op == "single":
            return rc, records_to_plan(op, recs, ptr, ptr["workspace"], n_floats), query
        return rc, records_to_plan(op, recs, ptr, ws_addr, None), query
    if rc != 0:
        return rc, None, query
    if op == "single":
        assert query is None or plan.workspace_bytes == query, r["name"]
        assert plan.slab_bytes == (plan.splits * n_floats * 4 if plan.splits > 1 else 0) and plan.workspace_bytes == plan.slab_bytes + plan.table_bytes
        got = {f: getattr(plan, f) for f in FIELDS["single"][:-1]}
        got["table_offset"] = ((ptr["workspace"] + plan.slab_bytes + 255) & ~255) - ptr["workspace"] if plan.kernel == 2 else -1
        assert (plan.table_grid > 0) == (plan.kernel == 2) and (plan.kernel != 2 or plan.table_bytes > 0)
        return rc, got, query
    assert plan.n == n and plan.workspace_bytes == query and plan.slab_bytes + 256 == query and plan.grid == plan.first[n] and plan.reduce_grid == plan.rfirst[n]
    got = dict(grid=plan.grid, reduce_grid=plan.reduce_grid, splits=list(plan.splits[:n]), chunk=list(plan.chunk[:n]),
               slab_offset=[plan.slab_offset[g] if plan.splits[g] > 1 else -1 for g in range(n)], first=list(plan.first), rfirst=list(plan.rfirst))
    return rc, got, query


def answers(lib_path, rows, recorded=False, lib=None):
    """[(status, plan, query)] of rows: in this process where the flat switch is off (it must be unset here), in one child process
    for the rows that set it."""
    assert "MRCNN_CONV_FLAT_GLDS" not in os.environ, "unset MRCNN_CONV_FLAT_GLDS"
    out = [None] * len(rows)
    here = [i for i, r in enumerate(rows) if not r.get("flat")]
    there = [i for i, r in enumerate(rows) if r.get("flat")]
    if here:
        lib = lib or load(lib_path, recorded)
        for i in here:
            out[i] = replay(lib, rows[i], recorded)
    if there:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", lib_path] + (["--recorded"] if recorded else [])
        p = subprocess.run(cmd, input=json.dumps([rows[i] for i in there]), env=dict(os.environ, MRCNN_CONV_FLAT_GLDS="1"), capture_output=True, text=True)
        assert p.returncode == 0, p.stderr[-3000:]
        for i, a in zip(there, json.loads(p.stdout)):
            out[i] = tuple(a)
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
        op = r.get("op", "single")
        r["status"], r["wsq"], r["plan"] = status, wsq, plan and [plan[f] for f in FIELDS[op]]
        key = (op, status, plan and ((plan["kernel"], plan["reduce"]) if op == "single" else plan["reduce_grid"] > 0))
        by[key] = by.get(key, 0) + 1
    with open(sys.argv[2], "w") as f:      # one array per row: name, descriptor(s), options, then the answers
        f.write("[\n" + ",\n".join(json.dumps([r["name"], r["desc"], {k: r[k] for k in DEFAULTS if k in r}, r["status"], r["plan"], r["wsq"]],
                                              separators=(",", ":")) for r in rows) + "\n]\n")
    print(len(rows), "rows;", sorted(by.items(), key=str))


if __name__ == "__main__":
    main()
