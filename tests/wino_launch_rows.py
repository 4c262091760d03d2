"""Rows of tests/golden/wino_launch_rows.json and their replay: what the Winograd host code of ops.py launches, in which order and
with which buffers -- ops.winograd_weights, conv2d_winograd, conv2d_winograd_chain, conv2d_dgrad_ep_winograd, conv2d_wgrad_winograd.

A row is one call of one of those functions on CPU tensors, no GPU: ops._need_cuda is a no-op, ops.current_stream answers 0 and
_hip.lib answers a spy.  The spy forwards the pure host queries (every entry whose name matches _hip._NO_RECORD:
mrcnn_winograd_group_floats, mrcnn_winograd_output_bwd_rows, the weight gradient's workspace queries) to the built library; every
other entry is recorded, not called, and answers 0 or the status the case prescribes (a refusal: MRCNN_ERR_UNSUPPORTED).
ops.workspace and ops.empty are wrapped so that their requests are recorded too (the engine's step arena hands tensors out by
request order, and a recorded step holds the workspaces); ops._ws_cache is cleared before every row.  A row's events, in order:
    ["ws", tag, bytes]                     a workspace request
    ["empty", shape, dtype]                an ops.empty request
    [entry, status, argument, ...]         a launch: scalars by value; a mrcnn_wino_group as ["g", oth, otw, th_n, tw_n, oh0, ow0];
                                           a descriptor as ["d", fields ...]; the problems of mrcnn_conv2d_wgrad_multi as
                                           ["problems", [descriptor fields, x, dy, dw, accumulate], ...]; a pointer as
                                           "<buffer>+<byte offset>" (None: null; 0: the stream), found by address range
and what the function returned.  A buffer is an operand of the call by its name, "ws:<tag>", "new:<k>" (the k-th tensor taken from
ops.empty) or "ret" / "ret:<i>" (a returned tensor that is none of those).

The committed table was NOT written by the ops.py it pins: it was written by the ops.py of the commit before the Winograd host code
was reshaped (7bb1ab6), from a worktree of that commit, with the library of this tree (no kernel differs):
    git worktree add <dir> 7bb1ab6
    python tests/wino_launch_rows.py tests/golden/wino_launch_rows.json --tree <dir> --lib caesar-mrcnn_amd/libmrcnn_hip.so
Without --tree the table is written from this tree (to compare: the two files are equal byte for byte).

Cases: the smallest shapes at which the host code can go wrong -- maps (N, H = W) of (1, 6): one 4 x 4 tile, every mixed group
present; (3, 10): the uniform 4 x 4 tiling hangs over the edge; (9, 14): the mask head's map -- under the tilings 2, 4 and
TILE_MIXED, always given (the MRCNN_WINOGRAD_* variables do not matter), with 32 -> 128 channels (an offset into V taken for one
into Mt, or Cin for Cout, shows) or 128 -> 128; mt_ready with 64 channels, as the GPU test uses it."""
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

MIXED = 6                                                   # ops.TILE_MIXED
TILES = (2, 4, MIXED)
MAPS = ((1, 6), (3, 10), (9, 14))
UNSUPPORTED = -4                                            # ops.ERR_UNSUPPORTED
FUNCTIONS = ("winograd_weights", "conv2d_winograd", "conv2d_winograd_chain", "conv2d_dgrad_ep_winograd", "conv2d_wgrad_winograd")


# ---- cases ------------------------------------------------------------------------------------------------------------------------
def case(fn, what, tile, N=3, H=10, cin=32, cout=128, status=None, **opts):
    name = "%s/%s/tile_%d/%dx%dx%d/%d_%d" % (fn, what, tile, N, H, H, cin, cout)
    return dict(name=name, fn=fn, tile=tile, N=N, H=H, cin=cin, cout=cout, status=status or {}, opts=opts)


def all_cases():
    R = []
    for tile in TILES:
        R.append(case("winograd_weights", "new", tile))
        R.append(case("winograd_weights", "into_out", tile, out=True))
    # conv2d_winograd: bare on every map, then the epilogue operands, a kept V and a ready one
    for tile in TILES:
        for N, H in MAPS:
            R.append(case("conv2d_winograd", "bare", tile, N, H, 128, 128))
        R.append(case("conv2d_winograd", "bare", tile))
        R.append(case("conv2d_winograd", "epilogue", tile, ep=True, act=1, out=True, z_out=True))
        R.append(case("conv2d_winograd", "keep_v", tile, keep_v=True))
        R.append(case("conv2d_winograd", "v_ready", tile, keep_v=True, v_ready=True))
        R.append(case("conv2d_winograd", "v_ready_epilogue", tile, 9, 14, 128, 128, ep=True, act=1, z_out=True, keep_v=True, v_ready=True))
    # conv2d_winograd_chain: the one launch accepted (returns None) and refused (the separate launches, returns the output)
    refused = {"mrcnn_winograd_chain": UNSUPPORTED}
    for N, H in MAPS:
        R.append(case("conv2d_winograd_chain", "accepted", MIXED, N, H, 128, 128, ep=True, act=1, z_out=True, keep_v=True))
    R.append(case("conv2d_winograd_chain", "accepted", MIXED, ep=True, act=1, z_out=True, keep_v=True))
    R.append(case("conv2d_winograd_chain", "accepted_no_z", MIXED, ep=True, act=1))
    R.append(case("conv2d_winograd_chain", "accepted_v_ready", MIXED, ep=True, act=1, z_out=True, keep_v=True, v_ready=True))
    for tile in TILES:
        R.append(case("conv2d_winograd_chain", "refused", tile, ep=True, act=1, z_out=True, keep_v=True, status=refused))
    R.append(case("conv2d_winograd_chain", "refused_no_z", MIXED, 1, 6, 128, 128, ep=True, act=1, status=refused))
    R.append(case("conv2d_winograd_chain", "refused_v_ready", MIXED, 9, 14, 128, 128, ep=True, act=1, z_out=True, keep_v=True, v_ready=True,
                  status=refused))
    # conv2d_dgrad_ep_winograd, plain form: the mask from z or from the activated output, the channel sums, dz_out, a ready V
    z = dict(act=1, fwd_shift=True, sums="all")
    for tile in TILES:
        R.append(case("conv2d_dgrad_ep_winograd", "plain_zmask", tile, **z))
        R.append(case("conv2d_dgrad_ep_winograd", "plain_from_out", tile, act=1, sums="all"))
    for N, H in MAPS:
        R.append(case("conv2d_dgrad_ep_winograd", "plain_zmask", MIXED, N, H, 128, 128, **z))
    R.append(case("conv2d_dgrad_ep_winograd", "plain_act_none", MIXED, act=0, sums="all"))
    R.append(case("conv2d_dgrad_ep_winograd", "plain_act_none_shift_given", MIXED, act=0, fwd_shift=True, sums="all"))
    R.append(case("conv2d_dgrad_ep_winograd", "plain_no_sums", MIXED, act=1, fwd_shift=True, sums=None))
    R.append(case("conv2d_dgrad_ep_winograd", "plain_dbias_only", MIXED, act=1, fwd_shift=True, sums="dbias"))
    R.append(case("conv2d_dgrad_ep_winograd", "plain_dbias_only_from_out", 4, act=1, sums="dbias"))
    R.append(case("conv2d_dgrad_ep_winograd", "plain_dz_out", MIXED, dz_out=True, **z))
    R.append(case("conv2d_dgrad_ep_winograd", "plain_v_ready", MIXED, keep_v=True, v_ready=True, **z))
    R.append(case("conv2d_dgrad_ep_winograd", "plain_keep_v", 2, keep_v=True, **z))
    # the chain form: accepted, refused by status, and without the z mask (mrcnn_winograd_bwd_chain is not asked at all)
    refused = {"mrcnn_winograd_bwd_chain": UNSUPPORTED}
    for N, H in MAPS:
        R.append(case("conv2d_dgrad_ep_winograd", "chain_accepted", MIXED, N, H, 128, 128, next_v=True, next_dm=True, **z))
    R.append(case("conv2d_dgrad_ep_winograd", "chain_accepted", MIXED, next_v=True, next_dm=True, **z))
    R.append(case("conv2d_dgrad_ep_winograd", "chain_accepted_no_dm", MIXED, next_v=True, **z))
    R.append(case("conv2d_dgrad_ep_winograd", "chain_accepted_dz_out", MIXED, next_v=True, next_dm=True, dz_out=True, **z))
    R.append(case("conv2d_dgrad_ep_winograd", "chain_accepted_v_ready", MIXED, next_v=True, next_dm=True, keep_v=True, v_ready=True, **z))
    R.append(case("conv2d_dgrad_ep_winograd", "chain_accepted_no_sums", MIXED, next_v=True, next_dm=True, act=1, fwd_shift=True, sums=None))
    R.append(case("conv2d_dgrad_ep_winograd", "chain_accepted_dbias_only", MIXED, next_v=True, next_dm=True, act=1, fwd_shift=True, sums="dbias"))
    for tile in TILES:
        R.append(case("conv2d_dgrad_ep_winograd", "chain_refused", tile, next_v=True, next_dm=True, status=refused, **z))
    R.append(case("conv2d_dgrad_ep_winograd", "chain_refused_no_dm", MIXED, next_v=True, status=refused, **z))
    R.append(case("conv2d_dgrad_ep_winograd", "chain_refused_dz_out", MIXED, 9, 14, 128, 128, next_v=True, next_dm=True, dz_out=True, status=refused, **z))
    R.append(case("conv2d_dgrad_ep_winograd", "chain_refused_v_ready", MIXED, 1, 6, 128, 128, next_v=True, next_dm=True, keep_v=True, v_ready=True,
                  status=refused, **z))
    R.append(case("conv2d_dgrad_ep_winograd", "chain_refused_no_sums", MIXED, next_v=True, next_dm=True, act=1, fwd_shift=True, sums=None, status=refused))
    R.append(case("conv2d_dgrad_ep_winograd", "chain_without_zmask", MIXED, next_v=True, next_dm=True, act=1, sums="all"))
    R.append(case("conv2d_dgrad_ep_winograd", "chain_without_zmask_act_none", MIXED, next_v=True, act=0, fwd_shift=True, sums="all"))
    # mt_ready: the caller made the product; 64 channels, which the GEMM of the module does not take
    for tile in TILES:
        R.append(case("conv2d_dgrad_ep_winograd", "mt_ready_refused", tile, 3, 10, 32, 64, next_v=True, next_dm=True, mt_ready=True, status=refused, **z))
    R.append(case("conv2d_dgrad_ep_winograd", "mt_ready_accepted", MIXED, 3, 10, 32, 64, next_v=True, next_dm=True, mt_ready=True, **z))
    # conv2d_wgrad_winograd: 16 GEMMs per launch for tile 2, 12 for the others; the single launches where the shared one refuses
    # (by status, or -- 32 input channels -- by its workspace query)
    refused = {"mrcnn_conv2d_wgrad_multi": UNSUPPORTED}
    for tile in TILES:
        for acc in (False, True):
            R.append(case("conv2d_wgrad_winograd", "accumulate" if acc else "overwrite", tile, 3, 10, 128, 128, accumulate=acc))
        R.append(case("conv2d_wgrad_winograd", "overwrite", tile))
        R.append(case("conv2d_wgrad_winograd", "dm_ready", tile, 3, 10, 128, 128, dm_ready=True))
        R.append(case("conv2d_wgrad_winograd", "dm_ready", tile, accumulate=True, dm_ready=True))
        R.append(case("conv2d_wgrad_winograd", "multi_refused", tile, 1, 6, 128, 128, status=refused))
    for N, H in ((1, 6), (9, 14)):
        R.append(case("conv2d_wgrad_winograd", "overwrite", MIXED, N, H, 128, 128))
    R.append(case("conv2d_wgrad_winograd", "dz_tensor_beside_dm_ready", MIXED, 1, 6, 128, 128, dm_ready=True, dz_tensor=True))
    names = [r["name"] for r in R]
    assert len(set(names)) == len(names), [n for n in names if names.count(n) > 1]
    return R


# ---- the recorder -------------------------------------------------------------------------------------------------------------------
class _Ptr(int):
    """An address seen in a launch; becomes "<buffer>+<offset>" when the row is complete."""


class Patch(object):
    """monkeypatch.setattr for the script."""

    def __init__(self):
        self.saved = []

    def setattr(self, obj, name, value):
        self.saved.append((obj, name, getattr(obj, name)))
        setattr(obj, name, value)

    def undo(self):
        for obj, name, value in reversed(self.saved):
            setattr(obj, name, value)
        del self.saved[:]


def _fields(s):
    return [int(getattr(s, f)) for f, _ in s._fields_]


class Spy(object):
    def __init__(self, hip, real, status, events):
        self.hip, self.real, self.status, self.events = hip, real, status, events

    def __getattr__(self, name):
        hip = self.hip
        if any(k in name for k in hip._NO_RECORD):
            return getattr(self.real, name)
        argtypes = hip._SIGNATURES[name][1]

        def f(*args):
            assert len(args) == len(argtypes), name
            rc = self.status.get(name, 0)
            ev = [name, rc]
            for i, (t, a) in enumerate(zip(argtypes, args)):
                if t is C.c_void_p:
                    ev.append(None if a is None else _Ptr(a))
                elif t is C.POINTER(hip.WinoGroup):
                    ev.append(["g"] + _fields(a._obj))
                elif t is C.POINTER(hip.ConvDesc):
                    ev.append(["d"] + _fields(a._obj))
                elif t is C.POINTER(hip.WgradProblem):
                    ev.append(["problems"] + [[_fields(q.d)] + [None if p is None else _Ptr(p) for p in (q.x, q.dy, q.dw)] + [int(q.accumulate)]
                                              for q in a[:args[i + 1]]])
                else:
                    ev.append(int(a))
            self.events.append(ev)
            return rc
        return f


def _U(torch, tile, cin, cout):
    z = lambda nb: torch.zeros((nb, cin, cout), dtype=torch.float32)
    return [z(36), z(24), z(24), z(16)] if tile == MIXED else z((tile + 2) ** 2)


def _call(ops, torch, c):
    """(function, args, kwargs, {name: operand tensor}) of a case."""
    o, tile, N, H, cin, cout = c["opts"], c["tile"], c["N"], c["H"], c["cin"], c["cout"]
    t = lambda *shape: torch.zeros(shape, dtype=torch.float32)
    fn = getattr(ops, c["fn"])
    named = {}

    def op(name, tensor):
        named[name] = tensor
        return tensor

    def weights():
        U = _U(torch, tile, cin, cout)
        for i, u in enumerate(U if isinstance(U, list) else ()):
            named["U%d" % i] = u
        return U if isinstance(U, list) else op("U", U)

    xshape, oshape = (N, H, H, cin), (N, H, H, cout)
    nv, nm = ops.winograd_v_floats(xshape, tile), ops.winograd_v_floats(oshape, tile)
    opt = lambda key, name, *shape: op(name, t(*shape)) if o.get(key) else None
    if c["fn"] == "winograd_weights":
        out = None
        if o.get("out"):
            out = _U(torch, tile, cin, cout)
            for i, u in enumerate(out if isinstance(out, list) else ()):
                named["out%d" % i] = u
            if not isinstance(out, list):
                named["out"] = out
        return fn, (op("w", t(3, 3, cin, cout)),), dict(out=out, tile=tile), named
    if c["fn"] in ("conv2d_winograd", "conv2d_winograd_chain"):
        ep = [op(n, t(cout)) for n in ("bias", "scale", "shift")] if o.get("ep") else [None] * 3
        x = xshape if o.get("v_ready") else op("x", t(*xshape))
        kw = dict(bias=ep[0], scale=ep[1], shift=ep[2], act=o.get("act", 0), z_out=opt("z_out", "z_out", *oshape), keep_v=opt("keep_v", "keep_v", nv),
                  v_ready=bool(o.get("v_ready")))
        if c["fn"] == "conv2d_winograd":
            return fn, (x, weights()), dict(kw, out=opt("out", "out", *oshape)), named
        return fn, (x, weights(), op("next_v", t(nm))), kw, named
    if c["fn"] == "conv2d_dgrad_ep_winograd":
        ready = o.get("v_ready") or o.get("mt_ready")
        dz = xshape if ready else op("dz", t(*xshape))
        sums = {"all": ("dgamma", "dbeta", "dbias"), "dbias": ("dbias",), None: ()}[o.get("sums")]
        s = [op(n, t(cout)) if n in sums else None for n in ("dgamma", "dbeta", "dbias")]
        kw = dict(fwd_shift=opt("fwd_shift", "fwd_shift", cout), next_v=opt("next_v", "next_v", nm), next_dm=opt("next_dm", "next_dm", nm),
                  dz_out=opt("dz_out", "dz_out", *oshape), keep_v=opt("keep_v", "keep_v", nv), v_ready=bool(o.get("v_ready")),
                  mt_ready=opt("mt_ready", "mt_ready", nm))
        args = (dz, weights(), op("below_out", t(*oshape)), op("below_z", t(*oshape)), op("scale", t(cout)), op("mean", t(cout)), op("rstd", t(cout)),
                s[0], s[1], s[2], o["act"])
        return fn, args, kw, named
    assert c["fn"] == "conv2d_wgrad_winograd"
    dz = op("dz", t(*oshape)) if (not o.get("dm_ready") or o.get("dz_tensor")) else oshape
    kw = dict(accumulate=bool(o.get("accumulate")), tile=tile, dm_ready=opt("dm_ready", "dm_ready", nm))
    return fn, (op("V", t(nv)), xshape, dz, op("dw", t(3, 3, cin, cout))), kw, named


def record(c, patch, ops, hip):
    """[events, returned] of case c through `ops`.  patch: pytest's monkeypatch, or a Patch (the caller undoes it)."""
    import torch
    real = hip.lib()
    events, taken, spaces = [], [], []
    real_ws, real_empty = ops.workspace, ops.empty

    def workspace(nbytes, device, tag="default"):
        events.append(["ws", tag, int(nbytes)])
        buf = real_ws(nbytes, device, tag)
        if not any(b is buf for _, b in spaces):
            spaces.append(("ws:" + tag, buf))
        return buf

    def empty(shape, dtype, device):
        events.append(["empty", [int(s) for s in shape], str(dtype).replace("torch.", "")])
        taken.append(real_empty(shape, dtype, device))
        return taken[-1]

    patch.setattr(ops, "_need_cuda", lambda *ts: None)
    patch.setattr(ops, "current_stream", lambda: 0)
    patch.setattr(ops, "workspace", workspace)
    patch.setattr(ops, "empty", empty)
    patch.setattr(hip, "lib", lambda: Spy(hip, real, c["status"], events))
    ops._ws_cache.clear()
    fn, args, kw, named = _call(ops, torch, c)
    ret = fn(*args, **kw)
    # every buffer stays alive up to here, so an address names one buffer
    buffers = list(named.items()) + spaces + [("new:%d" % k, b) for k, b in enumerate(taken)]
    rets = ret if isinstance(ret, (list, tuple)) else [ret]
    for i, r in enumerate(rets):
        if r is not None and not any(b is r for _, b in buffers):
            buffers.append(("ret:%d" % i if isinstance(ret, (list, tuple)) else "ret", r))
    ranges = [(b.data_ptr(), b.data_ptr() + b.numel() * b.element_size(), name) for name, b in buffers]

    def resolve(v):
        if isinstance(v, _Ptr):
            if v == 0:
                return 0
            hits = ["%s+%d" % (name, v - lo) for lo, hi, name in ranges if lo <= v < hi]
            assert len(hits) == 1, (c["name"], int(v), hits)
            return hits[0]
        return [resolve(e) for e in v] if isinstance(v, list) else v

    name_of = lambda r: None if r is None else [name for name, b in buffers if b is r][0]
    returned = [name_of(r) for r in ret] if isinstance(ret, (list, tuple)) else name_of(ret)
    return [resolve(events), returned]


def read_table(path):
    return [dict(name=name, events=events, returned=returned) for name, events, returned in json.load(open(path))]


def main():
    argv = sys.argv[1:]
    out = argv.pop(0)
    tree = os.path.abspath(argv[argv.index("--tree") + 1]) if "--tree" in argv else ROOT
    sys.path.insert(0, tree)
    from caesar_mrcnn_amd import _hip, ops
    assert os.path.dirname(os.path.dirname(os.path.abspath(ops.__file__))) == tree, ops.__file__
    if "--lib" in argv:
        _hip.LIB_PATH = os.path.abspath(argv[argv.index("--lib") + 1])
    rows = []
    for c in all_cases():
        patch = Patch()
        try:
            rows.append([c["name"]] + record(c, patch, ops, _hip))
        finally:
            patch.undo()
    with open(out, "w") as f:                # one array per row: name, events, returned
        f.write("[\n" + ",\n".join(json.dumps(r, separators=(",", ":")) for r in rows) + "\n]\n")
    print(len(rows), "rows,", sum(len(r[1]) for r in rows), "events, from", ops.__file__)


if __name__ == "__main__":
    main()
