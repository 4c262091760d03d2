"""Thin host-side operator layer over the C-ABI (one function per kernel group).

Every function takes/returns torch CUDA tensors that only serve as device-memory handles; the
arithmetic happens in libmrcnn_hip.so.  Shapes follow the reference graph (NHWC float32).
"""
import ctypes as C
import functools
import math
import os

import torch

from . import _hip
from ._hip import (ACT_NONE, ACT_RELU, ACT_SIGMOID, OUT_DECONV2, OUT_NHWC, RES_NONE, RES_SAME, RES_UP2,
                   check, current_stream, ptr)

BN_EPS = 1e-3  # Keras BatchNormalization default epsilon [3P]


def _need_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise _hip.HipPathError("hot-path operators need device tensors (got a CPU tensor)")
        if t is not None and not t.is_contiguous():
            raise _hip.HipPathError("hot-path operators need contiguous tensors")


def same_padding(size, k, stride):
    """TF 'SAME': out = ceil(size/stride); pad_before = total//2 (asymmetric when total is odd)."""
    out = -(-size // stride)
    total = max((out - 1) * stride + k - size, 0)
    return out, total // 2


def conv_desc(x_shape, w_shape, stride=1, padding="same", act=ACT_NONE, res_mode=RES_NONE):
    N, H, W, Cin = x_shape
    KH, KW, wcin, Cout = w_shape
    assert wcin == Cin, (x_shape, w_shape)
    d = _hip.ConvDesc()
    d.N, d.H, d.W, d.Cin, d.Cout, d.KH, d.KW, d.stride = N, H, W, Cin, Cout, KH, KW, stride
    if padding == "same":
        d.OH, d.pad_t = same_padding(H, KH, stride)
        d.OW, d.pad_l = same_padding(W, KW, stride)
    elif padding == "valid":
        d.OH, d.OW = (H - KH) // stride + 1, (W - KW) // stride + 1
        d.pad_t = d.pad_l = 0
    else:  # explicit symmetric zero padding (ZeroPadding2D + valid conv)
        ph, pw = padding
        d.OH, d.OW = (H + 2 * ph - KH) // stride + 1, (W + 2 * pw - KW) // stride + 1
        d.pad_t, d.pad_l = ph, pw
    d.act, d.res_mode, d.out_mode, d.cmod = act, res_mode, OUT_NHWC, Cout
    d.out_w_stride = Cout
    d.out_h_stride = d.OW * Cout
    d.out_n_stride = d.OH * d.OW * Cout
    return d


def conv2d(x, w, bias=None, scale=None, shift=None, res=None, stride=1, padding="same", act=ACT_NONE,
           res_mode=RES_NONE, out=None, z_out=None, desc=None):
    """out = act(bn(conv(x, w) + bias) + res).  w is HWIO.  Returns out [N, OH, OW, Cout]."""
    _need_cuda(x, w, bias, scale, shift, res, out, z_out)
    d = desc or conv_desc(tuple(x.shape), tuple(w.shape), stride, padding, act, res_mode)
    if out is None:
        out = empty((d.N, d.OH, d.OW, d.Cout), torch.float32, x.device)
    nbytes = _hip.lib().mrcnn_conv2d_fwd_workspace(C.byref(d))
    ws = workspace(nbytes, x.device, "conv_splitk") if nbytes else None
    check(_hip.lib().mrcnn_conv2d_fwd_ws(C.byref(d), ptr(x), ptr(w), ptr(bias), ptr(scale), ptr(shift), ptr(res),
                                         ptr(out), ptr(z_out), ptr(ws), ws.numel() if ws is not None else 0,
                                         current_stream()), "mrcnn_conv2d_fwd")
    return out


def conv2d_plan(d, x=16, w=16, bias=None, scale=None, shift=None, res=None, out=16, z_out=None, workspace=None,
                workspace_bytes=None, ep=None):
    """(status, _hip.ConvPlan) of the launch conv2d (ep None) or conv2d_dgrad_ep (ep a _hip.BwdEpilogue) would issue for the
    descriptor d.  Host only: the operands are addresses (only their nullness and alignment count; tensors are taken by
    their address), nothing is launched.  workspace_bytes None: what conv2d passes, mrcnn_conv2d_fwd_workspace(d), at a
    16-byte aligned address when that is not 0."""
    adr = lambda t: t if t is None or isinstance(t, int) else ptr(t)
    if workspace_bytes is None:
        workspace_bytes = _hip.lib().mrcnn_conv2d_fwd_workspace(C.byref(d))
        workspace = 16 if workspace_bytes else None
    plan = _hip.ConvPlan()
    rc = _hip.lib().mrcnn_conv2d_fwd_plan(C.byref(d), adr(x), adr(w), adr(bias), adr(scale), adr(shift), adr(res), adr(out), adr(z_out),
                                          adr(workspace), workspace_bytes, C.byref(ep) if ep is not None else None, C.byref(plan))
    return rc, plan


ERR_UNSUPPORTED = -4


def conv2d_dgrad_ep(dz, w_t, padding, below_out, below_z, scale, mean, rstd, dgamma, dbeta, dbias, act, res=None, out=None,
                    dy_out=None):
    """Data-gradient convolution (stride 1) fused with the epilogue backward of the layer below; returns dz_below, or
    None when the layer is too small for the fused kernel (the caller then uses conv2d + epilogue_bwd)."""
    _need_cuda(dz, w_t, below_out, below_z, scale, mean, rstd, dgamma, dbeta, dbias, res, out, dy_out)
    d = conv_desc(tuple(dz.shape), tuple(w_t.shape), 1, padding, ACT_NONE, RES_SAME if res is not None else RES_NONE)
    ep = _hip.BwdEpilogue()
    ep.out, ep.z, ep.scale, ep.mean, ep.rstd = ptr(below_out), ptr(below_z), ptr(scale), ptr(mean), ptr(rstd)
    ep.dgamma, ep.dbeta, ep.dbias, ep.act = ptr(dgamma), ptr(dbeta), ptr(dbias), act
    ep.dy = ptr(dy_out)                                # optional: y * act' (gradient a residual branch below receives)
    if out is None:
        out = empty((d.N, d.OH, d.OW, d.Cout), torch.float32, dz.device)
    nbytes = _hip.lib().mrcnn_conv2d_fwd_workspace(C.byref(d))
    ws = workspace(nbytes, dz.device, "conv_splitk") if nbytes else None
    rc = _hip.lib().mrcnn_conv2d_dgrad_ep(C.byref(d), ptr(dz), ptr(w_t), ptr(res), ptr(out), C.byref(ep), ptr(ws),
                                          ws.numel() if ws is not None else 0, current_stream())
    if rc == ERR_UNSUPPORTED:
        return None
    check(rc, "mrcnn_conv2d_dgrad_ep")
    return out


def conv2d_into(x, w, bias, out_view_ptr, n_stride, h_stride, w_stride, stride=1, padding="same", act=ACT_NONE):
    """Conv whose output rows land inside a larger buffer (e.g. one pyramid level of the concatenated
    RPN outputs).  out_view_ptr is the device address of element (0,0,0,0)."""
    _need_cuda(x, w, bias)
    d = conv_desc(tuple(x.shape), tuple(w.shape), stride, padding, act)
    d.out_n_stride, d.out_h_stride, d.out_w_stride = n_stride, h_stride, w_stride
    check(_hip.lib().mrcnn_conv2d_fwd(C.byref(d), ptr(x), ptr(w), ptr(bias), None, None, None, out_view_ptr, None,
                                      current_stream()), "mrcnn_conv2d_fwd(into)")


def _conv2d_problem(pr):
    """One problem of conv2d_multi as an ordinary launch."""
    if "out_ptr" in pr:
        x, w = pr["x"], pr["w"]
        _need_cuda(x, w, pr.get("bias"))
        d = conv_desc(tuple(x.shape), tuple(w.shape), pr.get("stride", 1), pr.get("padding", "same"), pr.get("act", ACT_NONE))
        d.out_n_stride, d.out_h_stride, d.out_w_stride = pr["out_strides"]
        nbytes = _hip.lib().mrcnn_conv2d_fwd_workspace(C.byref(d))
        ws = workspace(nbytes, x.device, "conv_splitk") if nbytes else None
        check(_hip.lib().mrcnn_conv2d_fwd_ws(C.byref(d), ptr(x), ptr(w), ptr(pr.get("bias")), ptr(pr.get("scale")),
                                             ptr(pr.get("shift")), None, pr["out_ptr"], None, ptr(ws),
                                             ws.numel() if ws is not None else 0, current_stream()), "mrcnn_conv2d_fwd(into)")
        return None
    return conv2d(pr["x"], pr["w"], pr.get("bias"), pr.get("scale"), pr.get("shift"), pr.get("res"), pr.get("stride", 1),
                  pr.get("padding", "same"), pr.get("act", ACT_NONE), pr.get("res_mode", RES_NONE), out=pr.get("out"),
                  z_out=pr.get("z_out"))


def conv2d_multi(problems):
    """Up to 5 independent convolutions in one launch (mrcnn_conv2d_fwd_multi).  Each problem is a dict:
    x, w, and optionally bias, scale, shift, res, res_mode, stride, padding, act, z_out, and either `out` (a dense
    tensor, allocated when missing) or `out_ptr` + `out_strides` (n, h, w strides in floats, as conv2d_into).
    Returns the list of `out` tensors (None where out_ptr was given), or None when the problems do not share a
    launch shape (the caller then issues them one by one)."""
    # problems large enough for the 128x128 LDS-DMA kernel (>= 640 tiles) fill the chip on their own and run faster
    # there than on the 64-row tiles of the shared launch: they go out individually, the small rest travels together
    def big(pr):
        x, w = pr["x"], pr["w"]
        d = conv_desc(tuple(x.shape), tuple(w.shape), pr.get("stride", 1), pr.get("padding", "same"))
        return d.Cout % 128 == 0 and d.Cin % 32 == 0 and ((d.N * d.OH * d.OW + 127) // 128) * (d.Cout // 128) >= 640
    flags = [big(pr) for pr in problems]
    if any(flags):
        small = [pr for pr, f in zip(problems, flags) if not f]
        so = conv2d_multi(small) if len(small) > 1 else None
        if so is None:
            so = [_conv2d_problem(pr) for pr in small]
        small_outs = iter(so)
        return [_conv2d_problem(pr) if f else next(small_outs) for pr, f in zip(problems, flags)]
    n = len(problems)
    arr = (_hip.ConvProblem * n)()
    outs = []
    for q, pr in zip(arr, problems):
        x, w = pr["x"], pr["w"]
        _need_cuda(x, w, pr.get("bias"), pr.get("scale"), pr.get("shift"), pr.get("res"), pr.get("out"), pr.get("z_out"))
        d = conv_desc(tuple(x.shape), tuple(w.shape), pr.get("stride", 1), pr.get("padding", "same"), pr.get("act", ACT_NONE),
                      pr.get("res_mode", RES_NONE))
        out = pr.get("out")
        if "out_ptr" in pr:
            d.out_n_stride, d.out_h_stride, d.out_w_stride = pr["out_strides"]
            q.out = pr["out_ptr"]
            out = None
        else:
            if out is None:
                out = empty((d.N, d.OH, d.OW, d.Cout), torch.float32, x.device)
            q.out = ptr(out)
        outs.append(out)
        q.d = d
        q.x, q.w, q.bias, q.scale, q.shift = ptr(x), ptr(w), ptr(pr.get("bias")), ptr(pr.get("scale")), ptr(pr.get("shift"))
        q.res, q.z_out = ptr(pr.get("res")), ptr(pr.get("z_out"))
    nbytes = _hip.lib().mrcnn_conv2d_fwd_multi_workspace(arr, n)
    ws = workspace(nbytes, problems[0]["x"].device, "conv_splitk") if nbytes else None
    rc = _hip.lib().mrcnn_conv2d_fwd_multi(arr, n, ptr(ws), ws.numel() if ws is not None else 0, current_stream())
    if rc == ERR_UNSUPPORTED:
        return None
    check(rc, "mrcnn_conv2d_fwd_multi")
    return outs


_DECONV_GEMM = os.environ.get("MRCNN_DECONV_GEMM", "1") != "0"          # transposed convolution on the persistent GEMM (A/B switch)
_DECONV_GEMM_MIN_ROWS = int(os.environ.get("MRCNN_DECONV_GEMM_MIN_ROWS", "16384"))


def deconv2x2(x, w_gemm, bias, act=ACT_RELU, out=None):
    """Conv2DTranspose(2x2, stride 2): x [N,H,W,Cin], w_gemm [Cin, 4*Cd] with column (a*2+b)*Cd+co."""
    _need_cuda(x, w_gemm, bias, out)
    N, H, W, Cin = x.shape
    Cd = w_gemm.shape[1] // 4
    if out is None:
        out = empty((N, 2 * H, 2 * W, Cd), torch.float32, x.device)
    if (_DECONV_GEMM and Cin % 16 == 0 and Cd % 32 == 0 and (4 * Cd) % 128 == 0 and act in (ACT_NONE, ACT_RELU) and
            N * H * W * Cin * 4 < 0x7FFFFFF0 and N * H * W >= _DECONV_GEMM_MIN_ROWS):
        # one filter tap of K: the persistent GEMM with the pixel-shuffle store in its epilogue
        check(_hip.lib().mrcnn_deconv2x2_gemm(ptr(x), ptr(w_gemm), ptr(bias), ptr(out), N, H, W, Cin, Cd, act, current_stream()),
              "mrcnn_deconv2x2_gemm")
        return out
    d = _hip.ConvDesc()
    d.N, d.H, d.W, d.Cin, d.Cout, d.KH, d.KW, d.stride, d.pad_t, d.pad_l = N, H, W, Cin, 4 * Cd, 1, 1, 1, 0, 0
    d.OH, d.OW, d.act, d.res_mode, d.out_mode, d.cmod = H, W, act, RES_NONE, OUT_DECONV2, Cd
    d.out_w_stride = Cd
    d.out_h_stride = 2 * W * Cd
    d.out_n_stride = 4 * H * W * Cd
    check(_hip.lib().mrcnn_conv2d_fwd(C.byref(d), ptr(x), ptr(w_gemm), ptr(bias), None, None, None, ptr(out), None,
                                      current_stream()), "mrcnn_conv2d_fwd(deconv)")
    return out


def deconv2x2_mask(x, w_gemm, bias, w_mask, b_mask, act=ACT_RELU, want_up=True):
    """The mask head's output stage: up = deconv2x2(x, w_gemm, bias, act), m = sigmoid(up . w_mask + b_mask) with w_mask [Cd, C].
    Returns (up, m), or (None, m) for want_up=False where the single launch ran (mrcnn_deconv2x2_mask_gemm: the 1x1 convolution
    and the sigmoid in the deconvolution's epilogue, `up` not read back).  Shapes that launch does not take run deconv2x2 and the
    1x1 convolution as two launches; `up` is returned then whatever want_up says."""
    _need_cuda(x, w_gemm, bias, w_mask, b_mask)
    N, H, W, Cin = x.shape
    Cd, Cm = w_gemm.shape[1] // 4, w_mask.shape[-1]
    if (_DECONV_GEMM and Cin % 16 == 0 and Cd == 256 and 1 <= Cm <= 16 and act in (ACT_NONE, ACT_RELU) and
            N * H * W * Cin * 4 < 0x7FFFFFF0 and N * H * W >= _DECONV_GEMM_MIN_ROWS):
        up = empty((N, 2 * H, 2 * W, Cd), torch.float32, x.device) if want_up else None
        m = empty((N, 2 * H, 2 * W, Cm), torch.float32, x.device)
        rc = _hip.lib().mrcnn_deconv2x2_mask_gemm(ptr(x), ptr(w_gemm), ptr(bias), ptr(up), ptr(w_mask), ptr(b_mask), ptr(m), N, H, W, Cin,
                                                  Cd, Cm, act, current_stream())
        if rc != ERR_UNSUPPORTED:
            check(rc, "mrcnn_deconv2x2_mask_gemm")
            return up, m
    up = deconv2x2(x, w_gemm, bias, act)
    m = conv2d(up, w_mask.reshape(1, 1, Cd, Cm), b_mask, act=ACT_SIGMOID)
    return up, m


_ws_cache = {}
_ws_retired = []


def workspace(nbytes, device, tag="default"):
    """Grow-only scratch buffer per (device, tag) -- nothing is allocated inside the C-ABI calls."""
    key = (str(device), tag, current_stream())        # one scratch buffer per stream: concurrent branches never share
    buf = _ws_cache.get(key)
    if buf is None or buf.numel() < nbytes:
        if buf is not None:
            _ws_retired.append(buf)     # captured HIP graphs may still point at it: never hand it back
        buf = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)
        _ws_cache[key] = buf
    return buf


class StepArena(object):
    """Reuses the tensors one training step allocates.  A step requests its activations, gradients and
    scratch in a fixed order with fixed shapes, so the k-th request of a step gets the k-th tensor of the
    previous step (a shape change simply replaces that slot).  Nothing is handed out twice within a step,
    and every side stream is joined before a step ends, so the reuse is race free.  Saves the ~20 ms/step the
    caching allocator costs for ~2 500 requests."""

    def __init__(self):
        self.slots, self.pos, self.active = [], 0, False

    def begin(self):
        self.pos, self.active = 0, True

    def end(self):
        self.active = False

    def take(self, shape, dtype, device):
        k = self.pos
        self.pos = k + 1
        if k < len(self.slots):
            t = self.slots[k]
            if t.shape == shape and t.dtype == dtype:
                return t
            t = torch.empty(shape, dtype=dtype, device=device)
            self.slots[k] = t
            return t
        t = torch.empty(shape, dtype=dtype, device=device)
        self.slots.append(t)
        return t


_arena = None


def set_arena(arena):
    global _arena
    _arena = arena


def empty(shape, dtype, device):
    if _arena is not None and _arena.active:
        return _arena.take(tuple(shape), dtype, device)
    return torch.empty(tuple(shape), dtype=dtype, device=device)


def empty_like(t):
    return empty(t.shape, t.dtype, t.device)


def conv2d_wgrad(x, dy, w_shape, stride=1, padding="same", dw=None, accumulate=False, desc=None):
    _need_cuda(x, dy, dw)
    d = desc or conv_desc(tuple(x.shape), tuple(w_shape), stride, padding)
    if dw is None:
        dw = empty(tuple(w_shape), torch.float32, x.device)
    nbytes = _hip.lib().mrcnn_conv2d_wgrad_workspace(C.byref(d))
    ws = workspace(nbytes, x.device, "wgrad")
    check(_hip.lib().mrcnn_conv2d_wgrad(C.byref(d), ptr(x), ptr(dy), ptr(dw), ptr(ws), ws.numel(),
                                        1 if accumulate else 0, current_stream()), "mrcnn_conv2d_wgrad")
    return dw


def conv2d_wgrad_plan(d, x=16, dy=16, dw=16, workspace=256, workspace_bytes=None):
    """(status, _hip.WgradPlan) of the launch conv2d_wgrad would issue for the descriptor d.  Host only, like conv2d_plan:
    operands are addresses (or tensors, taken by their address), only their nullness and 16-byte alignment count, nothing is
    launched.  workspace_bytes None: what conv2d_wgrad needs at least, mrcnn_conv2d_wgrad_workspace(d) (its grow-only scratch
    buffer may be larger)."""
    adr = lambda t: t if t is None or isinstance(t, int) else ptr(t)
    if workspace_bytes is None:
        workspace_bytes = _hip.lib().mrcnn_conv2d_wgrad_workspace(C.byref(d))
    plan = _hip.WgradPlan()
    rc = _hip.lib().mrcnn_conv2d_wgrad_plan(C.byref(d), adr(x), adr(dy), adr(dw), adr(workspace), workspace_bytes, C.byref(plan))
    return rc, plan


def conv2d_wgrad_multi_plan(descs, workspace=256, workspace_bytes=None):
    """(status, _hip.WgradMultiPlan) of the launch conv2d_wgrad_multi would issue for the descriptors `descs`, every operand at
    an aligned address; host only.  workspace_bytes None: mrcnn_conv2d_wgrad_multi_workspace's answer."""
    n = len(descs)
    arr = (_hip.WgradProblem * max(n, 1))()
    for q, d in zip(arr, descs):
        q.d, q.x, q.dy, q.dw = d, 16, 16, 16
    if workspace_bytes is None:
        workspace_bytes = _hip.lib().mrcnn_conv2d_wgrad_multi_workspace(arr, n)
    plan = _hip.WgradMultiPlan()
    rc = _hip.lib().mrcnn_conv2d_wgrad_multi_plan(arr, n, workspace, workspace_bytes, C.byref(plan))
    return rc, plan


def conv2d_wgrad_multi(items):
    """The weight gradients of up to _hip.WGRAD_MULTI_MAX layers in one launch (mrcnn_conv2d_wgrad_multi).  items: [(x, dy,
    w_shape, stride, padding, dw, accumulate)].  Returns False (nothing launched) when a layer does not fit the shared kernel."""
    n = len(items)
    arr = (_hip.WgradProblem * n)()
    for q, (x, dy, w_shape, stride, padding, dw, accumulate) in zip(arr, items):
        _need_cuda(x, dy, dw)
        q.d = conv_desc(tuple(x.shape), tuple(w_shape), stride, padding)
        q.x, q.dy, q.dw, q.accumulate = ptr(x), ptr(dy), ptr(dw), 1 if accumulate else 0
    nbytes = _hip.lib().mrcnn_conv2d_wgrad_multi_workspace(arr, n)
    if nbytes == 0:
        return False
    ws = workspace(nbytes, items[0][0].device, "wgrad")
    rc = _hip.lib().mrcnn_conv2d_wgrad_multi(arr, n, ptr(ws), ws.numel(), current_stream())
    if rc == ERR_UNSUPPORTED:
        return False
    check(rc, "mrcnn_conv2d_wgrad_multi")
    return True


def flip_table(entries, device):
    """entries: [(offset_floats, KH, KW, Cin, Cout)] -> (device table, n_layers, total_tiles) for
    weight_flip_transpose_batched."""
    import numpy as np
    rec = np.zeros(len(entries), dtype=[("off", "<i8"), ("KH", "<i4"), ("KW", "<i4"), ("Cin", "<i4"), ("Cout", "<i4"),
                                        ("first", "<i4"), ("pad", "<i4")])
    tiles = 0
    for i, (off, kh, kw, cin, cout) in enumerate(entries):
        rec[i] = (off, kh, kw, cin, cout, tiles, 0)
        tiles += kh * kw * ((cin + 31) // 32) * ((cout + 31) // 32)
    t = torch.from_numpy(rec.view(np.uint8).copy()).to(device)
    return t, len(entries), tiles


def weight_flip_transpose_batched(params, params_t, table):
    _need_cuda(params, params_t, table[0])
    check(_hip.lib().mrcnn_weight_flip_transpose_batched(ptr(params), ptr(params_t), ptr(table[0]), table[1], table[2],
                                                         current_stream()), "mrcnn_weight_flip_transpose_batched")


def weight_flip_transpose(w, out=None):
    _need_cuda(w, out)
    KH, KW, Cin, Cout = w.shape
    if out is None:
        out = empty((KH, KW, Cout, Cin), torch.float32, w.device)
    check(_hip.lib().mrcnn_weight_flip_transpose(ptr(w), ptr(out), KH, KW, Cin, Cout, current_stream()),
          "mrcnn_weight_flip_transpose")
    return out


def bn_fold(gamma, beta, mean, var, scale, shift, rstd=None, eps=BN_EPS):
    _need_cuda(gamma, beta, mean, var, scale, shift, rstd)
    check(_hip.lib().mrcnn_bn_fold(ptr(gamma), ptr(beta), ptr(mean), ptr(var), eps, ptr(scale), ptr(shift),
                                   ptr(rstd), gamma.numel(), current_stream()), "mrcnn_bn_fold")


def epilogue_bwd(dout, out=None, z=None, scale=None, mean=None, rstd=None, dy_out=None, dz_out=None,
                 dgamma=None, dbeta=None, dbias=None, act=ACT_NONE):
    _need_cuda(dout, out, z, scale, mean, rstd, dy_out, dz_out, dgamma, dbeta, dbias)
    C_ = dout.shape[-1]
    M = dout.numel() // C_
    check(_hip.lib().mrcnn_epilogue_bwd(ptr(dout), ptr(out), ptr(z), ptr(scale), ptr(mean), ptr(rstd), ptr(dy_out),
                                        ptr(dz_out), ptr(dgamma), ptr(dbeta), ptr(dbias), M, C_, act,
                                        current_stream()), "mrcnn_epilogue_bwd")


def maxpool3x3s2(x, want_argmax=False):
    _need_cuda(x)
    N, H, W, C_ = x.shape
    OH, pt = same_padding(H, 3, 2)
    OW, pl = same_padding(W, 3, 2)
    out = empty((N, OH, OW, C_), torch.float32, x.device)
    am = empty((N, OH, OW, C_), torch.int32, x.device) if want_argmax else None
    check(_hip.lib().mrcnn_maxpool3x3s2_fwd(ptr(x), ptr(out), ptr(am), N, H, W, C_, OH, OW, pt, pl,
                                            current_stream()), "mrcnn_maxpool3x3s2_fwd")
    return (out, am) if want_argmax else out


def maxpool3x3s2_bwd(dout, argmax, in_shape):
    _need_cuda(dout, argmax)
    N, H, W, C_ = in_shape
    dx = empty(in_shape, torch.float32, dout.device)
    check(_hip.lib().mrcnn_maxpool3x3s2_bwd(ptr(dout), ptr(argmax), ptr(dx), N, H, W, C_, dout.shape[1],
                                            dout.shape[2], current_stream()), "mrcnn_maxpool3x3s2_bwd")
    return dx


def subsample2(x):
    _need_cuda(x)
    N, H, W, C_ = x.shape
    out = empty((N, (H + 1) // 2, (W + 1) // 2, C_), torch.float32, x.device)
    check(_hip.lib().mrcnn_subsample2_fwd(ptr(x), ptr(out), N, H, W, C_, current_stream()), "mrcnn_subsample2_fwd")
    return out


def subsample2_bwd_acc(dout, dx):
    _need_cuda(dout, dx)
    N, H, W, C_ = dx.shape
    check(_hip.lib().mrcnn_subsample2_bwd_acc(ptr(dout), ptr(dx), N, H, W, C_, current_stream()),
          "mrcnn_subsample2_bwd_acc")


def upsample2_bwd(dout, dsrc, accumulate):
    _need_cuda(dout, dsrc)
    N, H, W, C_ = dsrc.shape
    check(_hip.lib().mrcnn_upsample2_bwd(ptr(dout), ptr(dsrc), N, H, W, C_, 1 if accumulate else 0,
                                         current_stream()), "mrcnn_upsample2_bwd")


def add_inplace(dst, src):
    _need_cuda(dst, src)
    assert dst.numel() == src.numel()
    check(_hip.lib().mrcnn_add_inplace(ptr(dst), ptr(src), dst.numel(), current_stream()), "mrcnn_add_inplace")


def softmax_rows(logits, out=None):
    _need_cuda(logits, out)
    C_ = logits.shape[-1]
    if out is None:
        out = empty_like(logits)
    check(_hip.lib().mrcnn_softmax_rows(ptr(logits), ptr(out), logits.numel() // C_, C_, current_stream()),
          "mrcnn_softmax_rows")
    return out


def _roi_desc(boxes, fms, pool, image_area):
    d = _hip.RoiAlignDesc()
    d.B, d.R, d.P, d.C = boxes.shape[0], boxes.shape[1], pool, fms[0].shape[3]
    for i, f in enumerate(fms):
        d.H[i], d.W[i] = f.shape[1], f.shape[2]
    d.image_area = float(image_area)
    return d


def roialign(boxes, fms, pool, image_area, want_levels=False):
    """PyramidROIAlign: boxes [B,R,4], fms = [P2,P3,P4,P5] -> [B,R,pool,pool,C]."""
    _need_cuda(boxes, *fms)
    d = _roi_desc(boxes, fms, pool, image_area)
    out = empty((d.B, d.R, pool, pool, d.C), torch.float32, boxes.device)
    lv = empty((d.B, d.R), torch.int32, boxes.device) if want_levels else None
    check(_hip.lib().mrcnn_roialign_fwd(C.byref(d), ptr(boxes), ptr(fms[0]), ptr(fms[1]), ptr(fms[2]), ptr(fms[3]),
                                        ptr(out), ptr(lv), current_stream()), "mrcnn_roialign_fwd")
    return (out, lv) if want_levels else out


def roialign_bwd(boxes, dout, dfms, pool, image_area, dense=False):
    """Scatter-add dout [B,R,pool,pool,C] into the (already initialised) gradient maps dfms.  dense=True: every ROI
    carries gradient -- use the gather form (one wave per pyramid pixel) when the shape allows."""
    _need_cuda(boxes, dout, *dfms)
    d = _roi_desc(boxes, dfms, pool, image_area)
    if dense:
        rc = _hip.lib().mrcnn_roialign_bwd_gather(C.byref(d), ptr(boxes), ptr(dout), ptr(dfms[0]), ptr(dfms[1]), ptr(dfms[2]),
                                                  ptr(dfms[3]), current_stream())
        if rc != ERR_UNSUPPORTED:
            check(rc, "mrcnn_roialign_bwd_gather")
            return
    check(_hip.lib().mrcnn_roialign_bwd(C.byref(d), ptr(boxes), ptr(dout), ptr(dfms[0]), ptr(dfms[1]), ptr(dfms[2]),
                                        ptr(dfms[3]), current_stream()), "mrcnn_roialign_bwd")


def roialign_h16(boxes, fms16, pool, image_area):
    """PyramidROIAlign on 16-bit pyramid levels -> 16-bit [B,R,pool,pool,C] (interpolation in float32, one rounding)."""
    _need_cuda(boxes, *fms16)
    dt = fms16[0].dtype
    assert dt in _H16 and all(f.dtype == dt and f.is_contiguous() for f in fms16)
    d = _roi_desc(boxes, fms16, pool, image_area)
    out = empty((d.B, d.R, pool, pool, d.C), dt, boxes.device)
    check(_hip.lib().mrcnn_roialign_fwd_h16(C.byref(d), _H16[dt], ptr(boxes), ptr(fms16[0]), ptr(fms16[1]), ptr(fms16[2]), ptr(fms16[3]),
                                            ptr(out), current_stream()), "mrcnn_roialign_fwd_h16")
    return out


def roialign_bwd_h16(boxes, dout16, dfms, pool, image_area, multiplier=1.0):
    """Scatter-add the 16-bit gradient dout16 [B,R,pool,pool,C] * multiplier into the float32 gradient maps dfms."""
    _need_cuda(boxes, dout16, *dfms)
    assert dout16.dtype in _H16 and dout16.is_contiguous()
    d = _roi_desc(boxes, dfms, pool, image_area)
    check(_hip.lib().mrcnn_roialign_bwd_h16(C.byref(d), _H16[dout16.dtype], ptr(boxes), ptr(dout16), float(multiplier), ptr(dfms[0]),
                                            ptr(dfms[1]), ptr(dfms[2]), ptr(dfms[3]), current_stream()), "mrcnn_roialign_bwd_h16")


def proposals(rpn_probs, rpn_bbox, anchors, pre_nms_limit, proposal_count, nms_threshold, std_dev, debug=False):
    """ProposalLayer. rpn_probs [B,A,2], rpn_bbox [B,A,4], anchors [A,4] (normalised) -> rois [B,count,4]."""
    _need_cuda(rpn_probs, rpn_bbox, anchors)
    B, A = rpn_probs.shape[0], rpn_probs.shape[1]
    d = _hip.ProposalDesc()
    d.B, d.A, d.pre_nms_limit, d.proposal_count, d.nms_threshold = B, A, pre_nms_limit, proposal_count, nms_threshold
    for i in range(4):
        d.std_dev[i] = float(std_dev[i])
    K = min(pre_nms_limit, A)
    rois = empty((B, proposal_count, 4), torch.float32, rpn_probs.device)
    top_idx = keep_idx = num_keep = None
    if debug:
        top_idx = empty((B, K), torch.int32, rois.device)
        keep_idx = empty((B, proposal_count), torch.int32, rois.device)
        num_keep = empty((B,), torch.int32, rois.device)
    nbytes = _hip.lib().mrcnn_proposal_workspace(C.byref(d))
    ws = workspace(nbytes, rois.device, "proposal")
    check(_hip.lib().mrcnn_proposal_fwd(C.byref(d), ptr(rpn_probs), ptr(rpn_bbox), ptr(anchors), ptr(rois),
                                        ptr(top_idx), ptr(keep_idx), ptr(num_keep), ptr(ws), ws.numel(),
                                        current_stream()), "mrcnn_proposal_fwd")
    if debug:
        # sorted, decoded, clipped boxes live at the head of the workspace: [B, K, 4]
        base = (ws.data_ptr() + 255) // 256 * 256 - ws.data_ptr()
        boxes = ws[base: base + B * K * 16].view(torch.float32).view(B, K, 4).clone()
        return rois, top_idx, keep_idx, num_keep, boxes
    return rois


def proposal_status(rpn_probs, pre_nms_limit, proposal_count):
    """Health words of the last proposals() call of this shape on the current stream (synchronises):
    int32 [B, 3] = keys collected, keys announced, stores refused by the bounds guard of the multi-workgroup
    selection (mrcnn_proposal_status_offset)."""
    B, A = rpn_probs.shape[0], rpn_probs.shape[1]
    d = _hip.ProposalDesc()
    d.B, d.A, d.pre_nms_limit, d.proposal_count = B, A, pre_nms_limit, proposal_count
    ws = workspace(_hip.lib().mrcnn_proposal_workspace(C.byref(d)), rpn_probs.device, "proposal")
    stride = C.c_size_t(0)
    off = _hip.lib().mrcnn_proposal_status_offset(C.byref(d), ptr(ws), C.byref(stride))
    torch.cuda.synchronize()
    words = ws.cpu().numpy()
    import numpy as np
    return np.stack([np.frombuffer(words[off + b * stride.value: off + b * stride.value + 12].tobytes(), np.uint32)
                     for b in range(B)]).astype(np.int64)


def detection_targets(proposals_, gt_class_ids, gt_boxes, gt_masks, rand_keys, train_rois, positive_ratio,
                      bbox_std_dev, mask_shape, use_mini_mask=False):
    _need_cuda(proposals_, gt_class_ids, gt_boxes, gt_masks, rand_keys)
    B, R = proposals_.shape[0], proposals_.shape[1]
    G = gt_boxes.shape[1]
    d = _hip.DetTargetDesc()
    d.B, d.R, d.G, d.T = B, R, G, train_rois
    d.MH, d.MW = gt_masks.shape[1], gt_masks.shape[2]
    d.mask_h, d.mask_w = mask_shape
    d.positive_count = int(train_rois * positive_ratio)
    import numpy as np
    d.negative_ratio_r = float(np.float32(1.0 / positive_ratio))
    for i in range(4):
        d.bbox_std_dev[i] = float(np.float32(bbox_std_dev[i]))
    d.use_mini_mask = 1 if use_mini_mask else 0
    dev = proposals_.device
    rois = empty((B, train_rois, 4), torch.float32, dev)
    tcls = empty((B, train_rois), torch.int32, dev)
    tbbox = empty((B, train_rois, 4), torch.float32, dev)
    tmask = empty((B, train_rois, mask_shape[0], mask_shape[1]), torch.float32, dev)
    assign = empty((B, train_rois), torch.int32, dev)
    counts = empty((B, 2), torch.int32, dev)
    check(_hip.lib().mrcnn_detection_targets(C.byref(d), ptr(proposals_), ptr(gt_class_ids), ptr(gt_boxes),
                                             ptr(gt_masks), ptr(rand_keys), ptr(rois), ptr(tcls), ptr(tbbox),
                                             ptr(tmask), ptr(assign), ptr(counts), current_stream()),
          "mrcnn_detection_targets")
    return rois, tcls, tbbox, tmask, assign, counts


def rpn_targets(anchors_px, gt_class_ids, gt_boxes_px, rand_keys, n_train, bbox_std_dev):
    """build_rpn_targets (mrcnn/model.py:1536-1644) for a batch: anchors_px [A,4] float64 pixels,
    gt_class_ids [B,G] int32, gt_boxes_px [B,G,4] int32, rand_keys [B,A] float32 ->
    rpn_match [B,A,1] int32, rpn_bbox [B,n_train,4] float32."""
    _need_cuda(anchors_px, gt_class_ids, gt_boxes_px, rand_keys)
    assert anchors_px.dtype == torch.float64 and gt_boxes_px.dtype == torch.int32 and gt_class_ids.dtype == torch.int32
    assert rand_keys.dtype == torch.float32
    B, G = gt_class_ids.shape
    A = anchors_px.shape[0]
    assert rand_keys.shape == (B, A) and gt_boxes_px.shape == (B, G, 4)
    d = _hip.RpnTargetDesc()
    d.B, d.A, d.G, d.n_train = B, A, G, int(n_train)
    for i in range(4):
        d.bbox_std_dev[i] = float(bbox_std_dev[i])
    dev = anchors_px.device
    match = empty((B, A, 1), torch.int32, dev)
    bbox = empty((B, int(n_train), 4), torch.float32, dev)
    nbytes = _hip.lib().mrcnn_rpn_targets_workspace(C.byref(d))
    ws = workspace(nbytes, dev, "rpn_targets")
    check(_hip.lib().mrcnn_rpn_targets(C.byref(d), ptr(anchors_px), ptr(gt_class_ids), ptr(gt_boxes_px), ptr(rand_keys),
                                       ptr(match), ptr(bbox), ptr(ws), nbytes, current_stream()), "mrcnn_rpn_targets")
    return match, bbox


def detections(rois, probs, deltas, windows, max_instances, min_confidence, nms_threshold, bbox_std_dev):
    _need_cuda(rois, probs, deltas, windows)
    B, R, C_ = probs.shape
    d = _hip.DetectionDesc()
    d.B, d.R, d.C, d.max_instances = B, R, C_, max_instances
    d.min_confidence, d.nms_threshold = float(min_confidence), float(nms_threshold)
    for i in range(4):
        d.bbox_std_dev[i] = float(bbox_std_dev[i])
    out = empty((B, max_instances, 6), torch.float32, rois.device)
    nbytes = _hip.lib().mrcnn_detection_workspace(C.byref(d))
    ws = workspace(nbytes, rois.device, "detection")
    check(_hip.lib().mrcnn_detection_fwd(C.byref(d), ptr(rois), ptr(probs), ptr(deltas), ptr(windows), ptr(out),
                                         ptr(ws), ws.numel(), current_stream()), "mrcnn_detection_fwd")
    return out


def losses_fwd_bwd(rpn_match, rpn_bbox_t, rpn_logits, rpn_bbox, tcls, tbbox, tmask, active_class_ids, cls_logits,
                   mbbox, mmask, weights, dice=False, class_weights=None):
    """Returns (losses[5], d_rpn_logits, d_rpn_bbox, d_cls_logits, d_mbbox, d_mmask).

    class_weights: None, or a float32 device tensor [C] of positive finite class weights (index 0 the background) that every ROI
    row of the three head losses carries by its target class.  None takes the unweighted entry."""
    if class_weights is not None:
        if not torch.is_tensor(class_weights) or class_weights.dtype != torch.float32:
            raise ValueError("class_weights must be a float32 tensor (got %s)" % getattr(class_weights, "dtype", type(class_weights)))
        if tuple(class_weights.shape) != (cls_logits.shape[2],):
            raise ValueError("class_weights must have shape [%d], one weight per model class (got %s)"
                             % (cls_logits.shape[2], tuple(class_weights.shape)))
        if class_weights.device != cls_logits.device or not class_weights.is_contiguous():
            raise ValueError("class_weights must be a contiguous tensor on %s (got %s)" % (cls_logits.device, class_weights.device))
    _need_cuda(rpn_match, rpn_bbox_t, rpn_logits, rpn_bbox, tcls, tbbox, tmask, active_class_ids, cls_logits, mbbox,
               mmask)
    d = _hip.LossDesc()
    d.B, d.A = rpn_logits.shape[0], rpn_logits.shape[1]
    d.T, d.C = cls_logits.shape[1], cls_logits.shape[2]
    d.mask_h, d.mask_w = tmask.shape[2], tmask.shape[3]
    d.max_rpn_pos = rpn_bbox_t.shape[1]
    d.mask_loss_dice = 1 if dice else 0
    for i in range(5):
        d.w[i] = float(weights[i])
    dev = rpn_logits.device
    losses = torch.empty((5,), dtype=torch.float32, device=dev)
    g = [empty_like(t) for t in (rpn_logits, rpn_bbox, cls_logits, mbbox, mmask)]
    nbytes = _hip.lib().mrcnn_losses_workspace(C.byref(d))
    ws = workspace(nbytes, dev, "losses")
    if class_weights is not None:
        check(_hip.lib().mrcnn_losses_fwd_bwd_weighted(C.byref(d), ptr(rpn_match), ptr(rpn_bbox_t), ptr(rpn_logits), ptr(rpn_bbox),
                                                       ptr(tcls), ptr(tbbox), ptr(tmask), ptr(active_class_ids), ptr(cls_logits),
                                                       ptr(mbbox), ptr(mmask), ptr(class_weights), ptr(losses), ptr(g[0]),
                                                       ptr(g[1]), ptr(g[2]), ptr(g[3]), ptr(g[4]), ptr(ws), ws.numel(),
                                                       current_stream()),
              "mrcnn_losses_fwd_bwd_weighted")
        return (losses,) + tuple(g)
    check(_hip.lib().mrcnn_losses_fwd_bwd(C.byref(d), ptr(rpn_match), ptr(rpn_bbox_t), ptr(rpn_logits), ptr(rpn_bbox),
                                          ptr(tcls), ptr(tbbox), ptr(tmask), ptr(active_class_ids), ptr(cls_logits),
                                          ptr(mbbox), ptr(mmask), ptr(losses), ptr(g[0]), ptr(g[1]), ptr(g[2]),
                                          ptr(g[3]), ptr(g[4]), ptr(ws), ws.numel(), current_stream()),
          "mrcnn_losses_fwd_bwd")
    return (losses,) + tuple(g)


def grad_prepare(grads, params, grad_scale, gran_coef, sumsq_out):
    _need_cuda(grads, params, gran_coef, sumsq_out)
    check(_hip.lib().mrcnn_grad_prepare(ptr(grads), ptr(params), float(grad_scale), ptr(gran_coef), grads.numel(),
                                        ptr(sumsq_out), current_stream()), "mrcnn_grad_prepare")


def sumsq(g, out):
    _need_cuda(g, out)
    check(_hip.lib().mrcnn_sumsq(ptr(g), g.numel(), ptr(out), current_stream()), "mrcnn_sumsq")


def sgd_momentum(params, mom, grads, sumsq_t, clipnorm, lr, momentum, gran_coef, skipped=None):
    """skipped (int32 device tensor, 1 element): the guarded mixed-precision form -- a non-finite gradient norm skips the
    update on the device and counts the step there."""
    _need_cuda(params, mom, grads, sumsq_t, gran_coef, skipped)
    if skipped is not None:
        check(_hip.lib().mrcnn_sgd_momentum_guarded(ptr(params), ptr(mom), ptr(grads), ptr(sumsq_t), float(clipnorm), float(lr),
                                                    float(momentum), ptr(gran_coef), params.numel(), ptr(skipped),
                                                    current_stream()), "mrcnn_sgd_momentum_guarded")
        return
    check(_hip.lib().mrcnn_sgd_momentum(ptr(params), ptr(mom), ptr(grads), ptr(sumsq_t), float(clipnorm), float(lr),
                                        float(momentum), ptr(gran_coef), params.numel(), current_stream()),
          "mrcnn_sgd_momentum")


def pixel_unshuffle2(src, out=None):
    """[N,2H,2W,C] -> [N,H,W,4C] with column (a*2+b)*C + c."""
    _need_cuda(src, out)
    N, H2, W2, C_ = src.shape
    if out is None:
        out = empty((N, H2 // 2, W2 // 2, 4 * C_), torch.float32, src.device)
    check(_hip.lib().mrcnn_pixel_unshuffle2(ptr(src), ptr(out), N, H2 // 2, W2 // 2, C_, current_stream()),
          "mrcnn_pixel_unshuffle2")
    return out


def tuning_set(key, value):
    check(_hip.lib().mrcnn_tuning_set(key.encode(), int(value)), "mrcnn_tuning_set(%s)" % key)


def copy2d(dst_ptr, dst_pitch, src_ptr, src_pitch, row_bytes, rows):
    check(_hip.lib().mrcnn_copy2d(dst_ptr, dst_pitch, src_ptr, src_pitch, row_bytes, rows, current_stream()),
          "mrcnn_copy2d")


def unpack_mask_bits(packed, n_used, G):
    """packed [..., ceil(n_used / 8)] uint8 (numpy.packbits along the instance axis, bitorder="little") -> [..., G] uint8 planes,
    zeros from n_used on."""
    _need_cuda(packed)
    lead = tuple(packed.shape[:-1])
    out = torch.empty(lead + (G,), dtype=torch.uint8, device=packed.device)
    npix = 1
    for v in lead:
        npix *= v
    check(_hip.lib().mrcnn_unpack_mask_bits(ptr(packed), ptr(out), npix, packed.shape[-1], n_used, G, current_stream()),
          "mrcnn_unpack_mask_bits")
    return out


def unmold_masks(mrcnn_mask, dets, image_hw, packed=False, out=None):
    """utils.unmold_mask for all detections of one image on the device (mrcnn/model.py:2607-2619, mrcnn/utils.py:629-645).
    mrcnn_mask [R, MH, MW, C] float32 device; dets [n, 6] int32 device = (y1, x1, y2, x2, class_id, row of mrcnn_mask), boxes in
    pixels of the original image.  Returns uint8 [H, W, n] (0 / 1; .view(bool) is the reference's array) or, packed, [H, W,
    ceil(n / 8)] with detection d in bit d & 7 of byte d >> 3."""
    _need_cuda(mrcnn_mask, dets, out)
    assert mrcnn_mask.dtype == torch.float32 and mrcnn_mask.dim() == 4 and mrcnn_mask.is_contiguous()
    assert dets.dtype == torch.int32 and dets.dim() == 2 and dets.shape[1] == 6 and dets.is_contiguous()
    R, MH, MW, C_ = mrcnn_mask.shape
    n = dets.shape[0]
    H, W = int(image_hw[0]), int(image_hw[1])
    shape = (H, W, (n + 7) // 8 if packed else n)
    if out is None:
        out = torch.empty(shape, dtype=torch.uint8, device=mrcnn_mask.device)
    assert tuple(out.shape) == shape and out.dtype == torch.uint8 and out.is_contiguous()
    if n == 0 or H == 0 or W == 0:
        return out
    L = _hip.lib()
    nbytes = L.mrcnn_unmold_masks_workspace(n, MH, MW)
    ws = workspace(nbytes, mrcnn_mask.device, "unmold")
    check(L.mrcnn_unmold_masks(ptr(mrcnn_mask), R, MH, MW, C_, ptr(dets), n, H, W, 1 if packed else 0, ptr(out), ptr(ws),
                               ws.numel(), current_stream()), "mrcnn_unmold_masks")
    return out


FITS_TILE_DTYPE = [("x0", "<i4"), ("y0", "<i4"), ("w", "<i4"), ("h", "<i4"), ("pixel_offset", "<i8"), ("chunk_offset", "<i8")]
FITS_TILE_CHUNK = 1024                   # pixels per statistics chunk (csrc/fits.hip)


class FitsTileUnsupported(_hip.HipPathError):
    """A tile above the kernel's size limit (2048 x 2048 pixels): the caller takes the single-tile or the host path."""


def fits_tile_table(tiles):
    """mrcnn_fits_tile records (include/mrcnn_hip.h) of rectangles [(x0, y0, w, h), ...]: the pools laid out back to back in
    table order.  Host array; nothing is checked here -- mrcnn_fits_tiles_to_image does that before it launches."""
    import numpy as np
    r = np.asarray(tiles, dtype=np.int64).reshape(-1, 4)
    table = np.zeros(r.shape[0], dtype=FITS_TILE_DTYPE)
    for k, name in enumerate(("x0", "y0", "w", "h")):
        if r.shape[0] and (r[:, k].min() < -2 ** 31 or r[:, k].max() >= 2 ** 31):
            raise ValueError("tile rectangle outside the 32-bit range")
        table[name] = r[:, k]
    n = np.maximum(r[:, 2], 0) * np.maximum(r[:, 3], 0)
    table["pixel_offset"][1:] = np.cumsum(n)[:-1]
    table["chunk_offset"][1:] = np.cumsum((n + FITS_TILE_CHUNK - 1) // FITS_TILE_CHUNK)[:-1]
    return table


# ---- read_fits on the device, every flag combination (csrc/fits.hip: mrcnn_fits_to_image / mrcnn_fits_tiles_to_image) -------------
FITS_OUT_UINT8_RGB, FITS_OUT_FLOAT_RGB, FITS_OUT_GRAY = 0, 1, 2


class FitsChainUnsupported(_hip.HipPathError):
    """A flag combination the device chain refuses: uint8 output with neither stretch (nothing clips the channel to [0, 1] and
    the host's cast of out-of-range floats to uint8 is platform-defined).  Nothing was launched: the caller takes the host path."""


def _fits_rgb_chain(zscale_contrasts):
    """The run.py flags (zscale, / max, uint8 RGB; no bias / contrast stretch) with these three contrasts."""
    from .fits import DeviceChain
    return DeviceChain(True, False, True, FITS_OUT_UINT8_RGB, tuple(zscale_contrasts), 0.5, 1.0)


def _fits_chain(chain, H=1, W=1):
    """(mrcnn_fits_chain, dtype, trailing shape) of a chain description: an object with the fields of fits.DeviceChain, checked
    for an H x W tile (mrcnn_fits_image_check: the refusals of fits_to_image, before anything is allocated)."""
    zc = [float(v) for v in chain.zscale_contrasts]
    assert len(zc) == 3, "zscale_contrasts must hold three values"
    c = _hip.FitsChain(1 if chain.zscale else 0, 1 if chain.biascontrast else 0, 1 if chain.normalize else 0, int(chain.out_kind),
                       (C.c_double * 3)(*zc), float(chain.bias), float(chain.contrast))
    if c.out_kind not in (FITS_OUT_UINT8_RGB, FITS_OUT_FLOAT_RGB, FITS_OUT_GRAY):
        raise ValueError("out_kind must be 0 (uint8 RGB), 1 (float32 RGB) or 2 (float32 gray), got %r" % (chain.out_kind,))
    rc = _hip.lib().mrcnn_fits_image_check(C.byref(c), H, W)
    if rc == ERR_UNSUPPORTED:
        if (H, W) == (1, 1) or _hip.lib().mrcnn_fits_image_check(C.byref(c), 1, 1) == ERR_UNSUPPORTED:
            raise FitsChainUnsupported("the device chain does not take uint8 output with neither zscale nor the bias / contrast stretch")
        raise FitsTileUnsupported("mrcnn_fits_to_image: a %d x %d tile is above the kernel's size limit (2048 x 2048 pixels)" % (H, W))
    check(rc, "mrcnn_fits_image_check")
    dtype = torch.uint8 if c.out_kind == FITS_OUT_UINT8_RGB else torch.float32
    return c, dtype, (() if c.out_kind == FITS_OUT_GRAY else (3,))


def fits_to_image(raw, H, W, chain, big_endian=False, out=None):
    """utils.read_fits's numeric part on the device (mrcnn/utils.py:1088-1157; mrcnn_fits_to_image) for any flag combination of
    fits.read_fits: raw = the tile's H * W float32 values as a device tensor (any dtype of 4 * H * W bytes: float32, or the
    file's big-endian bytes as uint8 with big_endian=True); chain: what fits.device_chain returns.  -> uint8 [H, W, 3], float32
    [H, W, 3] or float32 [H, W] device tensor by chain.out_kind, equal bit for bit to the host branch of fits.read_fits on the
    same tile.  FitsChainUnsupported for the one combination the chain refuses, FitsTileUnsupported for a tile above 2048 x 2048
    pixels; neither launches or allocates anything."""
    _need_cuda(raw, out)
    assert raw.is_contiguous() and raw.numel() * raw.element_size() == 4 * H * W, "raw must hold H * W float32 values"
    c, dtype, tail = _fits_chain(chain, H, W)
    L = _hip.lib()
    shape = (H, W) + tail
    if out is None:
        out = torch.empty(shape, dtype=dtype, device=raw.device)
    assert tuple(out.shape) == shape and out.dtype == dtype and out.is_contiguous()
    nbytes = L.mrcnn_fits_workspace(H, W)
    ws = workspace(nbytes, raw.device, "fits")
    check(L.mrcnn_fits_to_image(ptr(raw), 1 if big_endian else 0, H, W, C.byref(c), ptr(out), out.numel() * out.element_size(), ptr(ws),
                                ws.numel(), current_stream()), "mrcnn_fits_to_image")
    return out


def fits_to_rgb(raw, H, W, zscale_contrasts=(0.25, 0.25, 0.25), big_endian=False, out=None):
    """fits_to_image with the run.py flags: -> uint8 [H, W, 3] (NaN -> min, per-channel zscale, / max, round(255 x))."""
    return fits_to_image(raw, H, W, _fits_rgb_chain(zscale_contrasts), big_endian=big_endian, out=out)


def fits_tiles_to_image(plane, tiles, chain, big_endian=False):
    """fits_to_image for T tiles of one plane that is already on the device, every stage one launch over all tiles
    (mrcnn_fits_tiles_to_image).  plane: [NY, NX] float32 device tensor, or with big_endian=True the file's bytes as uint8
    [NY, NX, 4]; tiles: T rectangles (x0, y0, w, h) in plane pixels -- sizes may differ, rectangles may overlap; chain as for
    fits_to_image.  Returns a list of T device tensors, views into one pool, each equal to fits_to_image of that cut (so to
    fits.read_fits of it).  Runs on the current stream.  ValueError for a malformed table (no tile, w or h <= 0, a rectangle
    that leaves the plane), FitsTileUnsupported for a tile above 2048 x 2048 pixels, FitsChainUnsupported; none launches or
    writes anything."""
    import numpy as np
    _need_cuda(plane)
    if plane.dim() < 2 or plane.numel() * plane.element_size() != 4 * plane.shape[0] * plane.shape[1]:
        raise ValueError("plane must hold NY x NX float32 values (got shape %r, dtype %s)" % (tuple(plane.shape), plane.dtype))
    NY, NX = int(plane.shape[0]), int(plane.shape[1])
    c, dtype, tail = _fits_chain(chain)
    table = fits_tile_table(tiles)
    T = int(table.shape[0])
    L = _hip.lib()
    host = table.ctypes.data_as(C.c_void_p)
    stream = current_stream()
    rc = L.mrcnn_fits_tiles_check(host, T, NY, NX)          # the call's own host-side check: nothing is allocated for a refused table
    if rc == ERR_UNSUPPORTED:
        raise FitsTileUnsupported("mrcnn_fits_tiles_to_image: a tile above the kernel's size limit (2048 x 2048 pixels)")
    if rc:
        raise ValueError("mrcnn_fits_tiles_to_image refuses the tiles (status %d): no tile, an empty rectangle or one outside the "
                         "%d x %d plane" % (rc, NY, NX))
    nbytes = L.mrcnn_fits_tiles_workspace(host, T, NY, NX)
    ws = workspace(nbytes, plane.device, "fits_tiles")
    total = int(table["pixel_offset"][-1]) + int(table["w"][-1]) * int(table["h"][-1])
    per = 3 if tail else 1
    pool = torch.empty(per * total, dtype=dtype, device=plane.device)
    table_dev = torch.from_numpy(table.view(np.uint8)).to(plane.device)
    check(L.mrcnn_fits_tiles_to_image(ptr(plane), 1 if big_endian else 0, NY, NX, host, ptr(table_dev), T, C.byref(c), ptr(pool),
                                      pool.numel() * pool.element_size(), ptr(ws), ws.numel(), stream), "mrcnn_fits_tiles_to_image")
    out = []
    for r in table:
        o, h, w = per * int(r["pixel_offset"]), int(r["h"]), int(r["w"])
        out.append(pool[o:o + per * h * w].view((h, w) + tail))
    return out


def fits_tiles_to_rgb(plane, tiles, zscale_contrasts=(0.25, 0.25, 0.25), big_endian=False):
    """fits_tiles_to_image with the run.py flags: a list of T uint8 [h, w, 3] device tensors."""
    return fits_tiles_to_image(plane, tiles, _fits_rgb_chain(zscale_contrasts), big_endian=big_endian)


# ---- the overview picture of a mosaic (csrc/fits.hip: mrcnn_mosaic_overview; csrc/maskgraph.hip: mrcnn_sources_to_planes) --------
class MosaicUnsupported(_hip.HipPathError):
    """A mosaic past a cap of mrcnn_mosaic_overview (more than 2^31 - 1 pixels) or of mrcnn_sources_to_planes (planes of more
    than 2^31 - 1 words, shrink * h or shrink * w beyond 2^31 - 1): nothing was launched, the caller takes the host statement."""


def _mosaic_refusal(rc, what):
    if rc == ERR_UNSUPPORTED:
        raise MosaicUnsupported("%s: past a cap of the kernel (status %d)" % (what, rc))
    if rc:
        raise ValueError("%s refuses the call (status %d): an empty plane or frame, a shrink below 1 or a contrast that is not "
                         "finite" % (what, rc))


def mosaic_overview(plane, shrink, contrast=0.25, big_endian=False, timing=None):
    """The overview frame of a whole mosaic (fits.mosaic_overview_host is the statement): plane [ny, nx] float32 on the device,
    or with big_endian=True the file's bytes as uint8 [ny, nx, 4] (what SFinder._plane_device holds) -> uint8 [ceil(ny / shrink),
    ceil(nx / shrink), 3] device tensor: read_fits's chain on the whole plane with that zscale contrast, then the maximum of every
    shrink x shrink block.  The plane is read where it lies, twice; the workspace holds 24 bytes per 1024 pixels.  ValueError for
    a malformed call, MosaicUnsupported past 2^31 - 1 pixels; neither launches anything.  timing: a dict that receives the device
    time of the four launches (overview_kernels_ms, from events; costs a synchronisation)."""
    _need_cuda(plane)
    if plane.dim() < 2 or not plane.is_contiguous() or plane.numel() * plane.element_size() != 4 * plane.shape[0] * plane.shape[1]:
        raise ValueError("plane must hold ny x nx float32 values, contiguous (got shape %r, dtype %s)" % (tuple(plane.shape), plane.dtype))
    if big_endian and plane.dtype != torch.uint8:
        raise ValueError("big-endian input: the file's bytes as uint8 [ny, nx, 4]")
    if not big_endian and plane.dtype != torch.float32:
        raise ValueError("native input: float32 [ny, nx]")
    if int(shrink) != shrink:
        raise ValueError("shrink must be an integer (got %r)" % (shrink,))
    ny, nx, k = int(plane.shape[0]), int(plane.shape[1]), int(shrink)
    if ny >= 2 ** 31 or nx >= 2 ** 31 or not -2 ** 31 <= k < 2 ** 31:
        raise ValueError("plane side or shrink outside the 32-bit range")
    L = _hip.lib()
    _mosaic_refusal(L.mrcnn_mosaic_overview_check(ny, nx, k, float(contrast)), "mrcnn_mosaic_overview")
    h, w = -(-ny // k), -(-nx // k)
    ws = workspace(L.mrcnn_mosaic_overview_workspace(ny, nx), plane.device, "mosaic")
    out = torch.empty((h, w, 3), dtype=torch.uint8, device=plane.device)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)] if timing is not None else None
    if ev:
        ev[0].record()
    check(L.mrcnn_mosaic_overview(ptr(plane), 1 if big_endian else 0, ny, nx, k, float(contrast), ptr(out), out.numel(), ptr(ws),
                                  ws.numel(), current_stream()), "mrcnn_mosaic_overview")
    if ev:
        ev[1].record()
        ev[1].synchronize()
        timing["overview_kernels_ms"] = round(ev[0].elapsed_time(ev[1]), 4)
        timing["plane_bytes"] = 4 * ny * nx
    return out


def sources_to_planes(pool, desc, shrink, h, w, timing=None):
    """The sources of a mosaic as the MaskPlanes of its overview frame (sfinder.source_planes_host is the statement): pool, desc
    from tile_upload (x0 / y0 in mosaic pixels); bit (Y, X) of plane i is set iff source i has a pixel (y, x) with y // shrink == Y
    and x // shrink == X, pixels outside [0, shrink h) x [0, shrink w) are dropped; count and box as mask_planes_pack fills them.
    ValueError for a malformed call, MosaicUnsupported past a cap; neither launches anything."""
    _need_cuda(pool, desc)
    assert pool.dtype == torch.int32 and desc.dtype == torch.int32 and desc.dim() == 2 and desc.shape[1] == 6 and desc.is_contiguous()
    for name, v in (("shrink", shrink), ("h", h), ("w", w)):
        if int(v) != v or not -2 ** 31 <= int(v) < 2 ** 31:
            raise ValueError("sources_to_planes: %s must be a 32-bit integer (got %r)" % (name, v))
    n, k, h, w = int(desc.shape[0]), int(shrink), int(h), int(w)
    L = _hip.lib()
    _mosaic_refusal(L.mrcnn_sources_to_planes_check(n, k, h, w), "mrcnn_sources_to_planes")
    dev = pool.device
    words = torch.empty((n, h, (w + 31) // 32), dtype=torch.int32, device=dev)
    count = torch.empty((n,), dtype=torch.int32, device=dev)
    box = torch.empty((n, 4), dtype=torch.int32, device=dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)] if timing is not None else None
    if ev:
        ev[0].record()
    check(L.mrcnn_sources_to_planes(ptr(pool), pool.numel(), ptr(desc), n, k, h, w, ptr(words), ptr(count), ptr(box), current_stream()),
          "mrcnn_sources_to_planes")
    if ev:
        ev[1].record()
        ev[1].synchronize()
        timing["planes_kernels_ms"] = round(ev[0].elapsed_time(ev[1]), 4)
    return MaskPlanes(words, count, box, w)


# ---- source catalogue (csrc/catalog.hip) ------------------------------------------------------------------------------------
CATALOG_MAX_SOURCES = 1 << 18            # MRCNN_CATALOG_MAX_SOURCES (include/mrcnn_hip.h)
CATALOG_FILL_WALK, CATALOG_FILL_LAUNCHES = 0, 1


class CatalogUnsupported(_hip.HipPathError):
    """A catalogue mrcnn_catalog_count / _fill do not take: more sources than the cap (2^18), member lists of more than 2^31 - 1
    entries, or a window coordinate outside the supported range (not finite, or of magnitude 2^31 or more).  Nothing was launched:
    the caller takes the host statement."""


def catalog_members(table, dx, dy, device):
    """Windows and member lists of a whole catalogue (mrcnn_catalog_count, a scan, mrcnn_catalog_fill).  table: host float64
    [S, 6], columns x0, y0, xmin, xmax, ymin, ymax; dx, dy: the cut-out size.  Returns host arrays: windows int32 [S, 4] (xmin,
    xmax, ymin, ymax = int(x0 -/+ dx / 2), int(y0 -/+ dy / 2)), offsets int64 [S + 1], members int32 and cut uint8 [offsets[S]]:
    row i = the sources j != i, ascending, whose centre lies strictly inside window i, and whether j's box touches or crosses it.
    CatalogUnsupported -- before any launch -- for a catalogue past the caps above."""
    import numpy as np
    t = np.ascontiguousarray(np.asarray(table, dtype=np.float64).reshape(-1, 6).T)        # six columns, each contiguous
    S = int(t.shape[1])
    dx, dy = float(dx), float(dy)
    if S == 0 or not (0 < dx < 2 ** 31 and 0 < dy < 2 ** 31):
        raise ValueError("catalog_members needs at least one source and a positive cut-out size")
    L = _hip.lib()
    rc = L.mrcnn_catalog_check(S)
    if rc == ERR_UNSUPPORTED:
        raise CatalogUnsupported("mrcnn_catalog_count: %d sources are above the kernel's cap" % S)
    check(rc, "mrcnn_catalog_check")
    with np.errstate(all="ignore"):
        edges = np.stack([t[0] - dx / 2, t[0] + dx / 2, t[1] - dy / 2, t[1] + dy / 2])
        if not (np.isfinite(edges).all() and (np.abs(edges) < 2.0 ** 31).all()):
            raise CatalogUnsupported("mrcnn_catalog_count: a window coordinate is not finite or outside the 32-bit range")
    device = torch.device(device)
    if device.type != "cuda":
        raise _hip.HipPathError("catalog_members needs a GPU device")
    cols = torch.from_numpy(t).to(device)
    windows = torch.empty((S, 4), dtype=torch.int32, device=device)
    counts = torch.empty(S, dtype=torch.int32, device=device)
    stream = current_stream()
    check(L.mrcnn_catalog_count(ptr(cols[0]), ptr(cols[1]), S, dx, dy, ptr(windows), ptr(counts), stream), "mrcnn_catalog_count")
    offsets = torch.zeros(S + 1, dtype=torch.int64, device=device)
    offsets[1:] = torch.cumsum(counts, 0, dtype=torch.int64)
    total = int(offsets[-1].item())
    if total > 2 ** 31 - 1:
        raise CatalogUnsupported("mrcnn_catalog_fill: %d member entries are above 2^31 - 1" % total)
    members = torch.empty(total, dtype=torch.int32, device=device)
    cut = torch.empty(total, dtype=torch.uint8, device=device)
    check(L.mrcnn_catalog_fill(ptr(cols[0]), ptr(cols[1]), ptr(cols[2]), ptr(cols[3]), ptr(cols[4]), ptr(cols[5]), S, dx, dy,
                               ptr(offsets), total, ptr(members) if total else None, ptr(cut) if total else None, stream),
          "mrcnn_catalog_fill")
    return windows.cpu().numpy(), offsets.cpu().numpy(), members.cpu().numpy(), cut.cpu().numpy()


def _catalog_plane(plane):
    _need_cuda(plane)
    if plane.dim() != 2 or plane.dtype != torch.float32:
        raise ValueError("plane must be a [NY, NX] float32 device tensor (got shape %r, dtype %s)" % (tuple(plane.shape), plane.dtype))
    return int(plane.shape[0]), int(plane.shape[1])


def _catalog_windows(windows, device):
    import numpy as np
    w = np.ascontiguousarray(np.asarray(windows, dtype=np.int64).reshape(-1, 4))
    if w.size and (w.min() < -2 ** 31 or w.max() >= 2 ** 31):
        raise ValueError("window outside the 32-bit range")
    return torch.from_numpy(w.astype(np.int32)).to(device)


def catalog_window_flags(plane, windows):
    """Finite and NaN pixel counts of T windows (xmin, xmax, ymin, ymax) of a resident float32 plane, clipped to the plane at the
    far edges as NumPy slicing clips (mrcnn_catalog_window_flags, one launch).  Returns a host int32 [T, 2]; a window with a
    negative corner or without a pixel gets (0, 0)."""
    import numpy as np
    NY, NX = _catalog_plane(plane)
    w = _catalog_windows(windows, plane.device)
    T = int(w.shape[0])
    if T == 0:
        return np.zeros((0, 2), np.int32)
    flags = torch.empty((T, 2), dtype=torch.int32, device=plane.device)
    check(_hip.lib().mrcnn_catalog_window_flags(ptr(plane), NY, NX, ptr(w), T, ptr(flags), current_stream()), "mrcnn_catalog_window_flags")
    return flags.cpu().numpy()


def catalog_nan_fill(plane, windows, form=CATALOG_FILL_WALK):
    """crop_img's in-place NaN fill for K windows of the resident plane, in the order given (mrcnn_catalog_nan_fill): window k's
    NaN pixels get the non-NaN minimum of window k of the plane as it is after the turns before it; a window without a finite
    pixel at its turn is left alone.  Writes `plane`.  Returns a host bool [K]: the window had a finite pixel at its turn.
    form: CATALOG_FILL_WALK (one workgroup walks the table) or CATALOG_FILL_LAUNCHES (one launch per window); same plane."""
    import numpy as np
    NY, NX = _catalog_plane(plane)
    w = _catalog_windows(windows, plane.device)
    K = int(w.shape[0])
    if K == 0:
        return np.zeros(0, bool)
    alive = torch.zeros(K, dtype=torch.int32, device=plane.device)
    check(_hip.lib().mrcnn_catalog_nan_fill(ptr(plane), NY, NX, ptr(w), K, int(form), ptr(alive), current_stream()), "mrcnn_catalog_nan_fill")
    return alive.cpu().numpy().astype(bool)


def mold_image_u8(src, out_hw, pad_tl, canvas_hw, mean_pixel, out=None):
    """utils.resize_image's pixel work + mold_image on the device (mrcnn/model.py:2519-2556): src [h, w, C] uint8 device ->
    float32 [OH, OW, C]: the image scaled to out_hw (bilinear, float64, clipped to the image's range, truncated to uint8; a copy
    when out_hw == (h, w)) at pad_tl inside a zero canvas, minus mean_pixel."""
    import numpy as np
    _need_cuda(src, out)
    assert src.dtype == torch.uint8 and src.dim() == 3 and src.is_contiguous()
    h, w, C_ = src.shape
    (oh, ow), (top, left), (OH, OW) = out_hw, pad_tl, canvas_hw
    if out is None:
        out = torch.empty((OH, OW, C_), dtype=torch.float32, device=src.device)
    assert tuple(out.shape) == (OH, OW, C_) and out.dtype == torch.float32 and out.is_contiguous()
    ws = workspace(64, src.device, "mold")
    mean = (C.c_double * C_)(*[float(v) for v in np.broadcast_to(np.asarray(mean_pixel, np.float64), (C_,))])
    check(_hip.lib().mrcnn_mold_image_u8(ptr(src), h, w, C_, int(oh), int(ow), int(top), int(left), int(OH), int(OW), mean, ptr(out),
                                         ptr(ws), ws.numel(), current_stream()), "mrcnn_mold_image_u8")
    return out


def mold_image_f32(src, out_hw, pad_tl, canvas_hw, mean_pixel, out=None):
    """mold_image_u8's float32 twin (mrcnn_mold_image_f32): src [h, w, C] float32 device (C <= 4) -> float32 [OH, OW, C]: the image
    scaled to out_hw (bilinear in float64, np.clip to the image's minimum / maximum, rounded to float32 as resize_image's
    astype(dtype) does; a copy when out_hw == (h, w)) at pad_tl inside a zero canvas, minus mean_pixel (float64), rounded to
    float32 -- MaskRCNN.mold_inputs followed by the graph's float32 cast, bit for bit apart from the payload of a NaN.  A NaN in
    an image that is scaled makes the scaled image NaN throughout, as np.clip with NaN bounds does.  ValueError for malformed
    input; it allocates, launches and writes nothing then."""
    import numpy as np
    if not torch.is_tensor(src) or src.dtype != torch.float32 or src.dim() != 3 or not src.is_contiguous():
        raise ValueError("mold_image_f32: src must be a contiguous float32 [h, w, C] tensor")
    h, w, C_ = (int(v) for v in src.shape)
    if h < 1 or w < 1 or not 1 <= C_ <= 4:
        raise ValueError("mold_image_f32: src %r must be non-empty with 1 to 4 channels" % ((h, w, C_),))
    try:
        (oh, ow), (top, left), (OH, OW) = (int(v) for v in out_hw), (int(v) for v in pad_tl), (int(v) for v in canvas_hw)
    except (TypeError, ValueError):
        raise ValueError("mold_image_f32: out_hw, pad_tl and canvas_hw must be pairs of integers")
    if oh < 1 or ow < 1 or top < 0 or left < 0 or top + oh > OH or left + ow > OW or max(OH, OW, h, w) >= 2 ** 31:
        raise ValueError("mold_image_f32: a %d x %d image at %r does not fit the %d x %d canvas" % (oh, ow, (top, left), OH, OW))
    if out is not None and (not torch.is_tensor(out) or out.dtype != torch.float32 or tuple(out.shape) != (OH, OW, C_)
                            or not out.is_contiguous() or out.device != src.device or out.data_ptr() == src.data_ptr()):
        raise ValueError("mold_image_f32: out must be a contiguous float32 [%d, %d, %d] tensor on src's device, not src itself"
                         % (OH, OW, C_))
    m = np.asarray(mean_pixel, np.float64).reshape(-1)
    if m.size not in (1, C_):
        raise ValueError("mold_image_f32: mean_pixel %r does not fit %d channel(s)" % (mean_pixel, C_))
    _need_cuda(src)
    if out is None:
        out = torch.empty((OH, OW, C_), dtype=torch.float32, device=src.device)
    ws = workspace(int(_hip.lib().mrcnn_mold_image_f32_workspace_bytes()), src.device, "mold_f32")
    mean = (C.c_double * C_)(*[float(v) for v in np.broadcast_to(m, (C_,))])
    check(_hip.lib().mrcnn_mold_image_f32(ptr(src), h, w, C_, oh, ow, top, left, OH, OW, mean, ptr(out), ptr(ws), ws.numel(),
                                          current_stream()), "mrcnn_mold_image_f32")
    return out


def _augment_matrix(m):
    import numpy as np
    m = np.asarray(m, dtype=np.float64).reshape(-1)
    assert m.shape == (6,) and np.all(np.isfinite(m)), "m must be a finite 2 x 3 inverse map"
    return (C.c_double * 6)(*[float(v) for v in m])


def augment_warp_u8(src, m, out=None):
    """One stage of the reference's training augmentation (scripts/run.py:1091-1100) on the device: src [H, W, C] uint8 (C <= 4)
    -> uint8 [H, W, C] sampled bilinearly (float64, zero outside, rint) at the inverse map m (2 x 3 doubles: (sx, sy) =
    m @ (x, y, 1)); byte-identical to augment.warp_host(..., "image")."""
    _need_cuda(src, out)
    assert src.dtype == torch.uint8 and src.dim() == 3 and 1 <= src.shape[2] <= 4
    H, W, C_ = src.shape
    if out is None:
        out = torch.empty_like(src)
    assert out.shape == src.shape and out.dtype == torch.uint8 and out.data_ptr() != src.data_ptr()
    check(_hip.lib().mrcnn_augment_warp_u8(ptr(src), H, W, C_, _augment_matrix(m), ptr(out), current_stream()),
          "mrcnn_augment_warp_u8")
    return out


def augment_warp_mask_bits(packed, m, out=None):
    """The same stage on bit-packed instance masks: packed [H, W, nbytes] uint8 (numpy.packbits(mask, axis=-1,
    bitorder="little")) -> [H, W, nbytes], warped without unpacking; a bit is set where the bilinear value of its 0 / 1 plane
    is > 0.5 (augment.warp_host(..., "mask"))."""
    _need_cuda(packed, out)
    assert packed.dtype == torch.uint8 and packed.dim() == 3 and packed.shape[2] >= 1
    H, W, nb = packed.shape
    if out is None:
        out = torch.empty_like(packed)
    assert out.shape == packed.shape and out.dtype == torch.uint8 and out.data_ptr() != packed.data_ptr()
    check(_hip.lib().mrcnn_augment_warp_mask_bits(ptr(packed), H, W, nb, _augment_matrix(m), ptr(out), current_stream()),
          "mrcnn_augment_warp_mask_bits")
    return out


class GtPrepUnsupported(_hip.HipPathError):
    """Masks past a cap of mrcnn_mask_bits_stats / mrcnn_mask_bits_gather (include/mrcnn_hip.h: a frame side above 8192, more than
    4096 instances, bits per pixel or output planes): the caller takes the host statement (datagen.mask_bits_stats_host /
    mask_bits_gather_host)."""


GTPREP_MAX_SIDE, GTPREP_MAX_INSTANCES = 8192, 4096          # MRCNN_GTPREP_MAX_* (include/mrcnn_hip.h)


def _gtprep_packed(packed, what):
    if not torch.is_tensor(packed) or packed.dtype != torch.uint8 or packed.dim() != 3:
        raise ValueError("%s: packed must be a uint8 [H, W, nb] tensor" % what)
    H, W, nb = (int(v) for v in packed.shape)
    if H < 1 or W < 1 or nb < 1 or nb % 4:
        raise ValueError("%s: packed %r must be non-empty with whole 32-bit words per pixel (nb %% 4 == 0)" % (what, (H, W, nb)))
    return H, W, nb


def _gtprep_refusal(rc, what):
    if rc == ERR_UNSUPPORTED:
        raise GtPrepUnsupported("%s: past a cap of the kernel (status %d)" % (what, rc))
    if rc:
        raise ValueError("%s refuses the request (status %d)" % (what, rc))


def gtprep_check(H, W, nb, n, G):
    """Raises what mask_bits_stats (n instances) and mask_bits_gather (G planes) would raise for masks of these sizes; launches
    nothing (the device sample path asks before it draws an augmentation plan)."""
    L = _hip.lib()
    _gtprep_refusal(L.mrcnn_mask_bits_stats_check(int(H), int(W), int(nb), int(n)), "mrcnn_mask_bits_stats")
    _gtprep_refusal(L.mrcnn_mask_bits_gather_check(int(H), int(W), int(nb), 0, int(G)), "mrcnn_mask_bits_gather")


def gtprep_zoom_check(h, w, nb, oh, ow, top, left, OH, OW):
    """Raises what mask_bits_zoom would raise for these sizes; launches nothing."""
    _gtprep_refusal(_hip.lib().mrcnn_mask_bits_zoom_check(int(h), int(w), int(nb), int(oh), int(ow), int(top), int(left), int(OH),
                                                          int(OW)), "mrcnn_mask_bits_zoom")


def mask_bits_stats(packed, n):
    """Pixel count and box of every instance of bit-packed masks, on the device: packed [H, W, nb] uint8 =
    np.packbits(mask != 0, axis=-1, bitorder="little") with nb % 4 == 0 (the layout of augment_warp_mask_bits), n instances ->
    (count [n] int32, box [n, 4] int32), equal to np.sum(mask, axis=(0, 1)) and utils.extract_bboxes(mask)
    (datagen.mask_bits_stats_host).  Bits >= n are ignored.  The two results are views of ONE int32 buffer of 5 n values (count,
    then box: ``count._base``), so a caller brings both to the host in one copy.  ValueError for malformed input,
    GtPrepUnsupported past a cap; neither allocates or launches anything."""
    H, W, nb = _gtprep_packed(packed, "mask_bits_stats")
    n = int(n)
    if n < 1 or n > 8 * nb:
        raise ValueError("mask_bits_stats: n = %d instances do not fit %d bytes per pixel" % (n, nb))
    L = _hip.lib()
    _gtprep_refusal(L.mrcnn_mask_bits_stats_check(H, W, nb, n), "mrcnn_mask_bits_stats")
    _need_cuda(packed)
    table = torch.empty((5 * n,), dtype=torch.int32, device=packed.device)
    count, box = table[:n], table[n:].view(n, 4)
    ws = workspace(L.mrcnn_mask_bits_stats_workspace(nb), packed.device, "gtprep")
    check(L.mrcnn_mask_bits_stats(ptr(packed), H, W, nb, n, ptr(count), ptr(box), ptr(ws), ws.numel(), current_stream()),
          "mrcnn_mask_bits_stats")
    return count, box


def mask_bits_gather(packed, sel, G, out=None):
    """Selected instances of bit-packed masks as uint8 planes, on the device: out[y, x, j] = bit sel[j] of pixel (y, x) for
    j < len(sel), 0 up to G -- mask[:, :, sel] padded to G planes (datagen.mask_bits_gather_host).  packed as for
    mask_bits_stats; sel: int32 indices (NumPy / list: checked against 0 <= sel < 8 nb here, then uploaded); out: a contiguous
    uint8 [H, W, G] device tensor, e.g. one image of the [B, H, W, G] batch.  ValueError for malformed input, GtPrepUnsupported
    past a cap; neither allocates, launches or writes anything."""
    import numpy as np
    H, W, nb = _gtprep_packed(packed, "mask_bits_gather")
    G = int(G)
    sel_h = np.asarray(sel)
    if sel_h.ndim != 1 or (sel_h.size and not np.issubdtype(sel_h.dtype, np.integer)):
        raise ValueError("mask_bits_gather: sel must be a 1-D integer table")
    k = int(sel_h.size)
    if G < 1 or k > G:
        raise ValueError("mask_bits_gather: %d selected instances for G = %d planes" % (k, G))
    if k and (int(sel_h.min()) < 0 or int(sel_h.max()) >= 8 * nb):
        raise ValueError("mask_bits_gather: sel must lie in [0, %d)" % (8 * nb))
    if out is not None and (not torch.is_tensor(out) or out.dtype != torch.uint8 or tuple(out.shape) != (H, W, G)
                            or not out.is_contiguous() or out.device != packed.device):
        raise ValueError("mask_bits_gather: out must be a contiguous uint8 [%d, %d, %d] tensor on packed's device" % (H, W, G))
    L = _hip.lib()
    _gtprep_refusal(L.mrcnn_mask_bits_gather_check(H, W, nb, k, G), "mrcnn_mask_bits_gather")
    _need_cuda(packed)
    if out is None:
        out = torch.empty((H, W, G), dtype=torch.uint8, device=packed.device)
    # (through pinned memory: the caller need not synchronise before the host table goes away)
    sel_d = torch.from_numpy(np.ascontiguousarray(sel_h, dtype=np.int32)).pin_memory().to(packed.device, non_blocking=True) if k else None
    check(L.mrcnn_mask_bits_gather(ptr(packed), H, W, nb, ptr(sel_d), k, G, ptr(out), current_stream()), "mrcnn_mask_bits_gather")
    return out                               # (sel_d goes back to the allocator of this stream: reused in stream order only)


def _zoom_table(t, n_in, device, what):
    """An index table of mask_bits_zoom on `device`: a NumPy / list table is checked against -1 <= t < n_in here and uploaded; a
    device tensor is taken as it is (the kernel reads any entry outside [0, n_in) as the constant)."""
    import numpy as np
    if torch.is_tensor(t):
        if t.dtype != torch.int32 or t.dim() != 1 or t.numel() < 1 or not t.is_contiguous() or t.device != device:
            raise ValueError("mask_bits_zoom: %s must be a contiguous 1-D int32 table on packed's device" % what)
        return t, int(t.numel())
    t_h = np.asarray(t)
    if t_h.ndim != 1 or t_h.size < 1 or not np.issubdtype(t_h.dtype, np.integer):
        raise ValueError("mask_bits_zoom: %s must be a non-empty 1-D integer table" % what)
    if int(t_h.min()) < -1 or int(t_h.max()) >= n_in:
        raise ValueError("mask_bits_zoom: %s must lie in [-1, %d)" % (what, n_in))
    return np.ascontiguousarray(t_h, dtype=np.int32), int(t_h.size)


def mask_bits_zoom(packed, iy, ix, pad_tl, canvas_hw, out=None):
    """utils.resize_mask on bit-packed masks, on the device: packed [h, w, nb] uint8 (as for mask_bits_stats) -> uint8
    [OH, OW, nb], canvas_hw = (OH, OW): pixel (top + y, left + x) = packed pixel (iy[y], ix[x]), pad_tl = (top, left), zeros where
    a table entry is -1 and everywhere outside the len(iy) x len(ix) window -- scipy.ndimage.zoom(order=0) with the tables of
    gtprep.zoom_index_tables, then np.pad (gtprep.mask_bits_zoom_host).  iy, ix: int32 tables, NumPy / list (checked against
    [-1, h) / [-1, w) here, then uploaded) or device tensors.  ValueError for malformed input, GtPrepUnsupported past a cap;
    neither allocates, launches or writes anything."""
    h, w, nb = _gtprep_packed(packed, "mask_bits_zoom")
    iy, oh = _zoom_table(iy, h, packed.device, "iy")
    ix, ow = _zoom_table(ix, w, packed.device, "ix")
    try:
        (top, left), (OH, OW) = (int(v) for v in pad_tl), (int(v) for v in canvas_hw)
    except (TypeError, ValueError):
        raise ValueError("mask_bits_zoom: pad_tl and canvas_hw must be pairs of integers")
    if not packed.is_contiguous() or packed.data_ptr() % 4:
        raise ValueError("mask_bits_zoom: packed must be contiguous and 4-byte aligned")
    if top < 0 or left < 0 or OH < 1 or OW < 1 or top + oh > OH or left + ow > OW:
        raise ValueError("mask_bits_zoom: a %d x %d window at %r does not fit the %d x %d canvas" % (oh, ow, (top, left), OH, OW))
    if out is not None and (not torch.is_tensor(out) or out.dtype != torch.uint8 or tuple(out.shape) != (OH, OW, nb)
                            or not out.is_contiguous() or out.device != packed.device or out.data_ptr() % 4):
        raise ValueError("mask_bits_zoom: out must be a contiguous, 4-byte aligned uint8 [%d, %d, %d] tensor on packed's device"
                         % (OH, OW, nb))
    L = _hip.lib()
    _gtprep_refusal(L.mrcnn_mask_bits_zoom_check(h, w, nb, oh, ow, top, left, OH, OW), "mrcnn_mask_bits_zoom")
    _need_cuda(packed)
    if out is None:
        out = torch.empty((OH, OW, nb), dtype=torch.uint8, device=packed.device)
    if not torch.is_tensor(iy):                  # (through pinned memory, as mask_bits_gather's table)
        iy = torch.from_numpy(iy).pin_memory().to(packed.device, non_blocking=True)
    if not torch.is_tensor(ix):
        ix = torch.from_numpy(ix).pin_memory().to(packed.device, non_blocking=True)
    check(L.mrcnn_mask_bits_zoom(ptr(packed), h, w, nb, ptr(iy), oh, ptr(ix), ow, top, left, OH, OW, ptr(out), current_stream()),
          "mrcnn_mask_bits_zoom")
    return out


def resize_image_u8(src, out_hw, pad_tl, canvas_hw, out=None):
    """utils.resize_image's pixel work on the device, for the training loader: src [h, w, C] uint8 device (C <= 4) -> uint8
    [OH, OW, C]: the image scaled to out_hw (bilinear, float64, clipped to the image's range, truncated to uint8 -- the value
    mold_image_u8 computes before it subtracts the mean; a copy when out_hw == (h, w)) at pad_tl inside a zero canvas.  ValueError
    for malformed input; it allocates, launches and writes nothing."""
    if not torch.is_tensor(src) or src.dtype != torch.uint8 or src.dim() != 3 or not src.is_contiguous():
        raise ValueError("resize_image_u8: src must be a contiguous uint8 [h, w, C] tensor")
    h, w, C_ = (int(v) for v in src.shape)
    if h < 1 or w < 1 or not 1 <= C_ <= 4:
        raise ValueError("resize_image_u8: src %r must be non-empty with 1 to 4 channels" % ((h, w, C_),))
    try:
        (oh, ow), (top, left), (OH, OW) = (int(v) for v in out_hw), (int(v) for v in pad_tl), (int(v) for v in canvas_hw)
    except (TypeError, ValueError):
        raise ValueError("resize_image_u8: out_hw, pad_tl and canvas_hw must be pairs of integers")
    if oh < 1 or ow < 1 or top < 0 or left < 0 or top + oh > OH or left + ow > OW or max(OH, OW) >= 2 ** 31:
        raise ValueError("resize_image_u8: a %d x %d image at %r does not fit the %d x %d canvas" % (oh, ow, (top, left), OH, OW))
    if out is not None and (not torch.is_tensor(out) or out.dtype != torch.uint8 or tuple(out.shape) != (OH, OW, C_)
                            or not out.is_contiguous() or out.device != src.device or out.data_ptr() == src.data_ptr()):
        raise ValueError("resize_image_u8: out must be a contiguous uint8 [%d, %d, %d] tensor on src's device, not src itself"
                         % (OH, OW, C_))
    _need_cuda(src)
    if out is None:
        out = torch.empty((OH, OW, C_), dtype=torch.uint8, device=src.device)
    ws = workspace(64, src.device, "mold")
    check(_hip.lib().mrcnn_resize_image_u8(ptr(src), h, w, C_, oh, ow, top, left, OH, OW, ptr(out), ptr(ws), ws.numel(),
                                           current_stream()), "mrcnn_resize_image_u8")
    return out


def tile_upload(pool, desc, device):
    """Sources of a mosaic for tile_adjacency / tile_union (include/mrcnn_hip.h: mrcnn_tile_source): pool = uint32 words (NumPy),
    desc [n, 6] int32 = (x0, y0, w, h, word_offset, words_per_row).  Checks every descriptor against the pool and uploads both
    once; returns (pool, desc) device tensors (int32 views)."""
    import numpy as np
    pool = np.ascontiguousarray(pool, dtype=np.uint32).reshape(-1)
    desc = np.ascontiguousarray(desc, dtype=np.int32).reshape(-1, 6)
    if desc.shape[0]:
        w, h, off, wpr = (desc[:, k].astype(np.int64) for k in (2, 3, 4, 5))
        ok = (w > 0) & (h > 0) & (off >= 0) & (wpr >= (w + 31) // 32) & (off + h * wpr <= pool.size)
        if not ok.all():
            raise _hip.HipPathError("tile source %d does not fit the pool of %d words" % (int(np.flatnonzero(~ok)[0]), pool.size))
    pool_t = torch.from_numpy(pool.view(np.int32) if pool.size else np.zeros(1, np.int32)).to(device)
    desc_t = torch.from_numpy(desc if desc.shape[0] else np.zeros((1, 6), np.int32)).to(device)
    return pool_t, desc_t


def tile_adjacency(pool, desc, pairs):
    """SFinder.merge_edge_sources' pixel-pair loops (mrcnn/sfinder.py:787-810) for all candidate pairs in one launch: pool, desc from
    tile_upload; pairs [P, 2] int32 (NumPy or device) source indices -> int32 [P] device, 1 where some pixel of the first and some
    pixel of the second source have |dx| <= 1 and |dy| <= 1."""
    import numpy as np
    _need_cuda(pool, desc)
    n = desc.shape[0]
    if not torch.is_tensor(pairs):
        pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
        if pairs.size and (pairs.min() < 0 or pairs.max() >= n):
            raise _hip.HipPathError("tile_adjacency: pair index outside [0, %d)" % n)
        pairs = torch.from_numpy(pairs).to(pool.device)
    _need_cuda(pairs)
    assert pairs.dtype == torch.int32 and pairs.dim() == 2 and pairs.shape[1] == 2
    P = pairs.shape[0]
    out = torch.empty((P,), dtype=torch.int32, device=pool.device)
    if P:
        check(_hip.lib().mrcnn_tile_adjacency(ptr(pool), pool.numel(), ptr(desc), n, ptr(pairs), P, ptr(out), current_stream()),
              "mrcnn_tile_adjacency")
    return out


def tile_union_plan(desc_host, comp_offsets, member_ids):
    """Output layout of tile_union, from the boxes alone: (out_offsets [C], out_words, fresh_offsets [M], fresh_words), int64."""
    import numpy as np
    d = np.asarray(desc_host, dtype=np.int64).reshape(-1, 6)
    co = np.asarray(comp_offsets, dtype=np.int64)
    ids = np.asarray(member_ids, dtype=np.int64)
    C_, M = co.size - 1, ids.size
    if C_ < 0 or co[0] != 0 or co[-1] != M or np.any(np.diff(co) < 0) or (M and (ids.min() < 0 or ids.max() >= d.shape[0])):
        raise _hip.HipPathError("tile_union: malformed component list")
    m = d[ids]
    fresh_sizes = m[:, 3] * m[:, 5]
    fresh_offsets = np.concatenate([[0], np.cumsum(fresh_sizes)])
    out_sizes = np.zeros(C_, np.int64)
    nonempty = np.flatnonzero(np.diff(co) > 0)
    if nonempty.size:
        starts = co[:-1][nonempty]
        x0 = np.minimum.reduceat(m[:, 0], starts)
        y0 = np.minimum.reduceat(m[:, 1], starts)
        x1 = np.maximum.reduceat(m[:, 0] + m[:, 2], starts)
        y1 = np.maximum.reduceat(m[:, 1] + m[:, 3], starts)
        out_sizes[nonempty] = (y1 - y0) * ((x1 - x0 + 31) // 32)
    out_offsets = np.concatenate([[0], np.cumsum(out_sizes)])
    return out_offsets[:-1].copy(), int(out_offsets[-1]), fresh_offsets[:-1].copy(), int(fresh_offsets[-1])


def tile_union(pool, desc, desc_host, comp_offsets, member_ids):
    """The pixel union of SFinder.merge_edge_sources (mrcnn/sfinder.py:848-884) for all components in one launch.  Components in
    CSR form (comp_offsets [C + 1], member_ids [M], NumPy, members in the reference's visiting order); desc_host = the NumPy
    descriptors behind `desc`.  Returns a dict of device tensors: out_desc [C, 6] (box of the set bits, word_offset into
    out_pool), out_count [C], out_pool, fresh_pool (int32 views of the words) and the NumPy offsets out_offsets [C],
    fresh_offsets [M] (member position q's fresh bitmap: h * words_per_row words of member q's own box)."""
    import numpy as np
    _need_cuda(pool, desc)
    out_offsets, out_words, fresh_offsets, fresh_words = tile_union_plan(desc_host, comp_offsets, member_ids)
    C_, M = len(comp_offsets) - 1, len(member_ids)
    dev = pool.device
    res = {"out_offsets": out_offsets, "fresh_offsets": fresh_offsets,
           "out_desc": torch.zeros((C_, 6), dtype=torch.int32, device=dev), "out_count": torch.zeros((C_,), dtype=torch.int32, device=dev),
           "out_pool": torch.zeros((max(out_words, 1),), dtype=torch.int32, device=dev),
           "fresh_pool": torch.zeros((max(fresh_words, 1),), dtype=torch.int32, device=dev)}
    if C_ == 0:
        return res
    meta = np.concatenate([out_offsets, fresh_offsets]).astype(np.int64)
    meta_t = torch.from_numpy(meta).to(dev)
    csr_t = torch.from_numpy(np.concatenate([np.asarray(comp_offsets, np.int32), np.asarray(member_ids, np.int32)])).to(dev)
    check(_hip.lib().mrcnn_tile_union(ptr(pool), pool.numel(), ptr(desc), desc.shape[0], csr_t.data_ptr(), csr_t.data_ptr() + 4 * (C_ + 1),
                                      C_, M, meta_t.data_ptr(), meta_t.data_ptr() + 8 * C_, ptr(res["out_desc"]), ptr(res["out_count"]),
                                      ptr(res["out_pool"]), out_words, ptr(res["fresh_pool"]), fresh_words, current_stream()),
          "mrcnn_tile_union")
    res["_keep"] = (meta_t, csr_t)          # alive until the caller has synchronised on the results
    return res


def source_record_dtype():
    """NumPy view of mrcnn_source_record (include/mrcnn_hip.h)."""
    import numpy as np
    return np.dtype([("s64", "<f8"), ("w00", "<f8"), ("w10", "<f8"), ("w01", "<f8"), ("clip_mean", "<f8"), ("clip_median", "<f8"),
                     ("clip_std", "<f8"), ("m00", "<i8"), ("m10", "<i8"), ("m01", "<i8"), ("fill", "<f4"), ("smin", "<f4"),
                     ("smax", "<f4"), ("n_mask", "<i4"), ("npix", "<i4"), ("clip_kept", "<i4"), ("clip_iters", "<i4"),
                     ("n_gathered", "<i4")])


def source_params(img, pool, desc, cutouts, sigma=3.0, maxiters=5, big_endian=False, desc_host=None):
    """SFinder.compute_source_params' masked reductions (mrcnn/sfinder.py:1046-1075) for all sources of a mosaic in one launch
    (include/mrcnn_hip.h: mrcnn_source_params).  img: the image plane [H, W] on the device, float32, or the file's big-endian
    bytes as uint8 [H, W, 4] with big_endian=True; pool, desc from tile_upload; cutouts [n, 4] int32 (cx0, cy0, cx1, cy1), NumPy or
    device; desc_host = the NumPy descriptors behind `desc` (read back when not given).  Returns the records as a device uint8
    tensor [n, sizeof(mrcnn_source_record)]: `.cpu().numpy().view(source_record_dtype())` after which every field is an [n, 1]
    column."""
    import numpy as np
    _need_cuda(img, pool, desc)
    if big_endian:
        assert img.dtype == torch.uint8 and img.dim() == 3 and img.shape[2] == 4, "big-endian input: uint8 [H, W, 4]"
    else:
        assert img.dtype == torch.float32 and img.dim() == 2, "native input: float32 [H, W]"
    H, W = int(img.shape[0]), int(img.shape[1])
    n = int(desc.shape[0])
    if not torch.is_tensor(cutouts):
        cutouts = torch.from_numpy(np.ascontiguousarray(cutouts, dtype=np.int32).reshape(-1, 4)).to(pool.device)
    _need_cuda(cutouts)
    assert cutouts.dtype == torch.int32 and tuple(cutouts.shape) == (n, 4), "one cut-out rectangle per source"
    if H <= 0 or W <= 0:
        raise _hip.HipPathError("source_params: empty image")
    d = np.asarray(desc.cpu().numpy() if desc_host is None else desc_host, dtype=np.int64).reshape(-1, 6)
    assert d.shape[0] == n
    # a slice per source for its gathered pixel values: the bits its mask rows hold always suffice
    offs = np.concatenate([[0], np.cumsum(np.maximum(d[:, 3], 0) * np.maximum(d[:, 5], 0) * 32)]).astype(np.int64)
    rec = source_record_dtype()
    out = torch.zeros((n, rec.itemsize), dtype=torch.uint8, device=pool.device)
    if n == 0:
        return out
    values = workspace(4 * max(int(offs[-1]), 1), pool.device, "srcparams")
    offs_t = torch.from_numpy(offs).to(pool.device)
    check(_hip.lib().mrcnn_source_params(ptr(img), 1 if big_endian else 0, H, W, ptr(pool), pool.numel(), ptr(desc), n, ptr(cutouts),
                                         ptr(offs_t), ptr(values), values.numel() // 4, float(sigma), int(maxiters), ptr(out),
                                         current_stream()), "mrcnn_source_params")
    out._keep = (offs_t, cutouts)           # alive until the caller has synchronised on the result
    return out


class MaskPlanes(object):
    """The masks of one frame as bit planes on the device (include/mrcnn_hip.h, "mask graph"): words [n, H, ceil(W / 32)] int32
    (views of the 32-bit words), count [n] int32 = set pixels, box [n, 4] int32 = (y1, x1, y2, x2) as utils.extract_bboxes."""

    def __init__(self, words, count, box, W):
        self.words, self.count, self.box, self.W = words, count, box, int(W)
        self.n, self.H, self.wpr = (int(v) for v in words.shape)


def mask_planes_pack(masks):
    """masks [H, W, n] uint8 / bool device tensor (nonzero = set; what unmold_masks returns) -> MaskPlanes."""
    _need_cuda(masks)
    if masks.dtype == torch.bool:
        masks = masks.view(torch.uint8)
    assert masks.dtype == torch.uint8 and masks.dim() == 3
    H, W, n = (int(v) for v in masks.shape)
    if n <= 0 or H <= 0 or W <= 0:
        raise _hip.HipPathError("mask_planes_pack: empty request %r" % ((H, W, n),))
    dev = masks.device
    words = torch.empty((n, H, (W + 31) // 32), dtype=torch.int32, device=dev)
    count = torch.empty((n,), dtype=torch.int32, device=dev)
    box = torch.empty((n, 4), dtype=torch.int32, device=dev)
    check(_hip.lib().mrcnn_mask_planes_pack(ptr(masks), H, W, n, ptr(words), ptr(count), ptr(box), current_stream()),
          "mrcnn_mask_planes_pack")
    return MaskPlanes(words, count, box, W)


def mask_pair_stats(planes, pairs):
    """For pairs [P, 2] int32 (NumPy or device) of plane indices: (inter [P], touch [P]) int32 device tensors -- the pixels two
    planes share and analyze.masks_touch4 (== Analyzer.are_mask_connected) of the two.  An index outside [0, n) gives 0, 0."""
    import numpy as np
    _need_cuda(planes.words, planes.box)
    dev = planes.words.device
    if not torch.is_tensor(pairs):
        pairs = torch.from_numpy(np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)).to(dev)
    _need_cuda(pairs)
    assert pairs.dtype == torch.int32 and pairs.dim() == 2 and pairs.shape[1] == 2
    P = pairs.shape[0]
    inter = torch.empty((P,), dtype=torch.int32, device=dev)
    touch = torch.empty((P,), dtype=torch.int32, device=dev)
    if P:
        check(_hip.lib().mrcnn_mask_pair_stats(ptr(planes.words), ptr(planes.box), planes.n, planes.H, planes.W, ptr(pairs), P,
                                               ptr(inter), ptr(touch), current_stream()), "mrcnn_mask_pair_stats")
    return inter, touch


def mask_union(planes, comp_offsets, member_ids):
    """OR of the member planes of every component (CSR: comp_offsets [C + 1], member_ids [M], NumPy) -> MaskPlanes of the C unions,
    an empty component giving a zero plane."""
    import numpy as np
    _need_cuda(planes.words)
    co = np.ascontiguousarray(comp_offsets, dtype=np.int32).reshape(-1)
    ids = np.ascontiguousarray(member_ids, dtype=np.int32).reshape(-1)
    C_, M = co.size - 1, ids.size
    if C_ < 0 or co[0] != 0 or co[-1] != M or np.any(np.diff(co) < 0):
        raise _hip.HipPathError("mask_union: malformed component list")
    dev = planes.words.device
    words = torch.empty((C_, planes.H, planes.wpr), dtype=torch.int32, device=dev)
    count = torch.empty((C_,), dtype=torch.int32, device=dev)
    box = torch.empty((C_, 4), dtype=torch.int32, device=dev)
    if C_:
        csr_t = torch.from_numpy(np.concatenate([co, ids, np.zeros(1, np.int32)])).to(dev)
        check(_hip.lib().mrcnn_mask_union(ptr(planes.words), planes.n, planes.H, planes.W, csr_t.data_ptr(),
                                          csr_t.data_ptr() + 4 * (C_ + 1), C_, M, ptr(words), ptr(count), ptr(box), current_stream()),
              "mrcnn_mask_union")
    return MaskPlanes(words, count, box, planes.W)


def mask_cross_stats(planes_a, planes_b):
    """inter [na, nb] int32 device tensor: the pixels plane i of `planes_a` shares with plane j of `planes_b` (two MaskPlanes of one
    frame; the same object may be given twice), in one launch (include/mrcnn_hip.h: mrcnn_mask_cross_stats).  An empty set gives
    an empty tensor, without a launch."""
    _need_cuda(planes_a.words, planes_a.box, planes_b.words, planes_b.box)
    if (planes_a.H, planes_a.W) != (planes_b.H, planes_b.W):
        raise _hip.HipPathError("mask_cross_stats: plane sets of different frames %r, %r" % ((planes_a.H, planes_a.W), (planes_b.H, planes_b.W)))
    inter = torch.empty((planes_a.n, planes_b.n), dtype=torch.int32, device=planes_a.words.device)
    if planes_a.n > 0 and planes_b.n > 0 and planes_a.H > 0 and planes_a.W > 0:
        check(_hip.lib().mrcnn_mask_cross_stats(ptr(planes_a.words), ptr(planes_a.box), planes_a.n, ptr(planes_b.words), ptr(planes_b.box),
                                                planes_b.n, planes_a.H, planes_a.W, ptr(inter), current_stream()), "mrcnn_mask_cross_stats")
    return inter


def mask_plane_sums(img, planes, big_endian=False):
    """sum [n] float64 device tensor: np.nansum of the image values under every plane (include/mrcnn_hip.h: mrcnn_mask_plane_sums).
    img: the image plane [H, W] on the device, float32, or the file's big-endian bytes as uint8 [H, W, 4] with big_endian=True
    (as for source_params)."""
    _need_cuda(img, planes.words, planes.box)
    if big_endian:
        assert img.dtype == torch.uint8 and img.dim() == 3 and img.shape[2] == 4, "big-endian input: uint8 [H, W, 4]"
    else:
        assert img.dtype == torch.float32 and img.dim() == 2, "native input: float32 [H, W]"
    if (int(img.shape[0]), int(img.shape[1])) != (planes.H, planes.W):
        raise _hip.HipPathError("mask_plane_sums: image %r, planes %r" % (tuple(img.shape[:2]), (planes.H, planes.W)))
    out = torch.empty((planes.n,), dtype=torch.float64, device=planes.words.device)
    if planes.n > 0 and planes.H > 0 and planes.W > 0:
        check(_hip.lib().mrcnn_mask_plane_sums(ptr(img.contiguous()), 1 if big_endian else 0, ptr(planes.words), ptr(planes.box), planes.n,
                                               planes.H, planes.W, ptr(out), current_stream()), "mrcnn_mask_plane_sums")
    return out


class ComponentsUnsupported(_hip.HipPathError):
    """A frame or box table past a cap of mrcnn_mask_components_* (include/mrcnn_hip.h: a frame side above 8192, more than 4096
    planes, a box whose run capacity rows * ceil(columns / 2) is above 2^22, a workspace past 2^31 - 1 words, more than 2^24
    pieces): the caller takes the host statement."""


COMPONENTS_ALL, COMPONENTS_FIRST = 0, 1


class MaskComponents(object):
    """What mask_components leaves on the device for mask_components_split: ncomp [n] int32 (components per plane) and the
    workspace with the run table and its labels, for the planes and the host copy of their boxes they were made from."""

    def __init__(self, planes, connectivity, boxes_host, ncomp, ws):
        self.planes, self.connectivity, self.boxes_host, self.ncomp, self.ws = planes, int(connectivity), boxes_host, ncomp, ws
        self.ncomp_host = None               # set by mask_components_split, the one reader


def _components_refusal(rc, what):
    if rc == ERR_UNSUPPORTED:
        raise ComponentsUnsupported("%s: the frame or its box table is past a cap of the kernels (status %d): a side above 8192, more "
                                    "than 4096 planes, a box of more than 2^22 possible runs, or a workspace past int32 words" % (what, rc))
    if rc:
        raise ValueError("%s refuses the request (status %d): no plane, an empty frame or a connectivity other than 4 or 8" % (what, rc))


def _plane_boxes_host(planes, boxes_host):
    """The host copy of planes.box as contiguous int32 [n, 4]: the caller's, or one download (a synchronisation)."""
    import numpy as np
    b = planes.box.cpu().numpy() if boxes_host is None else boxes_host
    b = np.ascontiguousarray(b, dtype=np.int32).reshape(-1, 4)
    if b.shape[0] != planes.n:
        raise ValueError("boxes_host must be the host copy of the planes' boxes")
    return b


def mask_components(planes, connectivity=4, boxes_host=None):
    """Labels the 4- or 8-connected components of every plane of a MaskPlanes inside its box (include/mrcnn_hip.h:
    mrcnn_mask_components_count), numbered as analyze.label_components numbers them.  Returns a MaskComponents: ncomp stays on the
    device, nothing is read back here when `boxes_host` -- the NumPy copy of planes.box, which sizes the workspace -- is given;
    without it the boxes are downloaded first.  ValueError for a malformed request, ComponentsUnsupported past a cap; neither
    launches anything."""
    _need_cuda(planes.words, planes.box)
    if planes.n <= 0:
        raise ValueError("mask_components: no plane")
    bh = _plane_boxes_host(planes, boxes_host)
    L = _hip.lib()
    host = bh.ctypes.data_as(C.c_void_p)
    nbytes = int(L.mrcnn_mask_components_workspace(planes.n, planes.H, planes.W, host))
    _components_refusal(L.mrcnn_mask_components_check(planes.n, planes.H, planes.W, int(connectivity), host, nbytes), "mrcnn_mask_components_count")
    dev = planes.words.device
    ws = torch.empty((max(nbytes // 4, 1),), dtype=torch.int32, device=dev)
    ncomp = torch.empty((planes.n,), dtype=torch.int32, device=dev)
    check(L.mrcnn_mask_components_count(ptr(planes.words.contiguous()), host, ptr(planes.box.contiguous()), planes.n, planes.H, planes.W,
                                        int(connectivity), ptr(ws), nbytes, ptr(ncomp), current_stream()), "mrcnn_mask_components_count")
    return MaskComponents(planes, connectivity, bh, ncomp, ws)


def mask_components_split(handle, first_only=False):
    """The components of a MaskComponents as planes: (MaskPlanes of the P pieces, piece_offsets [n + 1] NumPy) -- plane p's pieces are
    piece_offsets[p] .. piece_offsets[p + 1], in component order; with `first_only` component 1 of every plane that has one.  The
    pieces have the layout of mask_union's result.  Reads ncomp back (kept as handle.ncomp_host): the one synchronisation."""
    import numpy as np
    planes = handle.planes
    nc = handle.ncomp.cpu().numpy().astype(np.int64)
    handle.ncomp_host = nc
    per = np.minimum(nc, 1) if first_only else nc
    if int(per.sum()) > 2 ** 24:
        raise ComponentsUnsupported("mask_components_split: %d pieces are past the 2^24 of mrcnn_mask_components_emit" % int(per.sum()))
    offs = np.concatenate([[0], np.cumsum(per)]).astype(np.int32)
    P, dev = int(offs[-1]), planes.words.device
    words = torch.empty((P, planes.H, planes.wpr), dtype=torch.int32, device=dev)
    count = torch.empty((P,), dtype=torch.int32, device=dev)
    box = torch.empty((P, 4), dtype=torch.int32, device=dev)
    if P:
        offs_t = torch.from_numpy(offs).to(dev)
        rc = _hip.lib().mrcnn_mask_components_emit(
            handle.boxes_host.ctypes.data_as(C.c_void_p), ptr(planes.box.contiguous()), planes.n, planes.H, planes.W, ptr(handle.ws),
            4 * handle.ws.numel(), ptr(handle.ncomp), offs.ctypes.data_as(C.c_void_p), ptr(offs_t),
            COMPONENTS_FIRST if first_only else COMPONENTS_ALL, ptr(words), ptr(count), ptr(box), current_stream())
        _components_refusal(rc if rc == ERR_UNSUPPORTED else 0, "mrcnn_mask_components_emit")
        check(rc, "mrcnn_mask_components_emit")
        words._keep = offs_t                 # alive until the caller has synchronised on the result
    return MaskPlanes(words, count, box, planes.W), offs


def mask_row_extents(planes, boxes_host=None):
    """(extents [R, 2] int32 device tensor, row_offsets [n + 1] NumPy): for every row of every plane's box the x of its leftmost and
    rightmost set pixel, (-1, -1) for a row without one; plane p's rows are extents[row_offsets[p] : row_offsets[p + 1]], top to
    bottom from its box's y1 (include/mrcnn_hip.h: mrcnn_mask_row_extents).  boxes_host as for mask_components."""
    import numpy as np
    _need_cuda(planes.words, planes.box)
    if planes.n <= 0:
        raise ValueError("mask_row_extents: no plane")
    bh = _plane_boxes_host(planes, boxes_host)
    b = bh.astype(np.int64)
    hgt = np.minimum(b[:, 2], planes.H) - np.maximum(b[:, 0], 0)
    wid = np.minimum(b[:, 3], planes.W) - np.maximum(b[:, 1], 0)
    hgt = np.where((hgt > 0) & (wid > 0), hgt, 0)
    if int(hgt.sum()) > 2 ** 31 - 1:
        raise ComponentsUnsupported("mask_row_extents: %d rows are past int32" % int(hgt.sum()))
    offs = np.concatenate([[0], np.cumsum(hgt)]).astype(np.int32)
    R, dev = int(offs[-1]), planes.words.device
    extents = torch.empty((R, 2), dtype=torch.int32, device=dev)
    if R:
        offs_t = torch.from_numpy(offs).to(dev)
        rc = _hip.lib().mrcnn_mask_row_extents(ptr(planes.words.contiguous()), bh.ctypes.data_as(C.c_void_p), ptr(planes.box.contiguous()),
                                               planes.n, planes.H, planes.W, ptr(offs_t), R, ptr(extents), current_stream())
        _components_refusal(rc if rc == ERR_UNSUPPORTED else 0, "mrcnn_mask_row_extents")
        check(rc, "mrcnn_mask_row_extents")
        extents._keep = offs_t
    return extents, offs


def voc_match(det_box, det_cls, det_score, det_off, gt_box, gt_cls, gt_off, thr):
    """The matching step of the Pascal-VOC box metrics for a whole test set in one launch (include/mrcnn_hip.h: mrcnn_voc_match).
    Device tensors: det_box [D, 4] / gt_box [G, 4] float64 corner boxes, det_cls [D] / gt_cls [G] int32, det_score [D] float64, thr [T]
    float64 (all > 0: the caller's contract).  det_off / gt_off: the CSR offsets of the I images, NumPy (checked here) --
    image i owns rows off[i] .. off[i + 1].  Returns (best_gt [D] int32, best_iou [D] float64, tp [T, D] uint8) on the device.
    D == 0 or I == 0 gives empty tensors, without a launch."""
    import numpy as np
    _need_cuda(det_box, det_cls, det_score, gt_box, gt_cls, thr)
    D, G, T = int(det_box.shape[0]), int(gt_box.shape[0]), int(thr.shape[0])
    assert det_box.dtype == gt_box.dtype == det_score.dtype == thr.dtype == torch.float64 and det_cls.dtype == gt_cls.dtype == torch.int32
    assert tuple(det_box.shape) == (D, 4) and tuple(gt_box.shape) == (G, 4) and tuple(det_cls.shape) == (D,) and tuple(gt_cls.shape) == (G,)
    assert tuple(det_score.shape) == (D,) and thr.dim() == 1
    do = np.ascontiguousarray(det_off, dtype=np.int64).reshape(-1)
    go = np.ascontiguousarray(gt_off, dtype=np.int64).reshape(-1)
    I = do.size - 1
    if I < 0 or go.size != I + 1 or do[0] != 0 or go[0] != 0 or do[-1] != D or go[-1] != G or np.any(np.diff(do) < 0) or np.any(np.diff(go) < 0):
        raise _hip.HipPathError("voc_match: malformed image offsets")
    if T <= 0 or max(D, G, I) > 0x7FFFFFFF:
        raise _hip.HipPathError("voc_match: no threshold, or tables past int32 rows")
    dev = det_box.device
    best_gt = torch.empty((D,), dtype=torch.int32, device=dev)
    best_iou = torch.empty((D,), dtype=torch.float64, device=dev)
    tp = torch.empty((T, D), dtype=torch.uint8, device=dev)
    if D > 0 and I > 0:
        off_t = torch.from_numpy(np.concatenate([do, go]).astype(np.int32)).to(dev)
        tensors = [t.contiguous() for t in (det_box, det_cls, det_score, gt_box, gt_cls, thr)]
        check(_hip.lib().mrcnn_voc_match(ptr(tensors[0]), ptr(tensors[1]), ptr(tensors[2]), off_t.data_ptr(), D,
                                         ptr(tensors[3]) if G else None, ptr(tensors[4]) if G else None, off_t.data_ptr() + 4 * (I + 1), G, I,
                                         ptr(tensors[5]), T, ptr(best_gt), ptr(best_iou), ptr(tp), current_stream()), "mrcnn_voc_match")
        best_gt._keep = (off_t, tensors)      # alive until the caller has synchronised on the result
    return best_gt, best_iou, tp


class ApSweepUnsupported(_hip.HipPathError):
    """A request past a cap of mrcnn_ap_sweep (include/mrcnn_hip.h: more than AP_SWEEP_CAPS["det"] detections or
    AP_SWEEP_CAPS["gt"] ground truths in one problem, more than AP_SWEEP_CAPS["thr"] thresholds): the caller keeps such problems
    for the host statement, or splits the thresholds."""


AP_SWEEP_OK, AP_SWEEP_OVER_CANDIDATES, AP_SWEEP_OVER_ROWS = 0, 1, 2
_ap_sweep_caps = None


def ap_sweep_caps():
    """{"det", "gt", "thr", "cand"}: the compile-time caps of csrc/apsweep.hip, read from the library once."""
    global _ap_sweep_caps
    if _ap_sweep_caps is None:
        caps = (C.c_int32 * 4)()
        check(_hip.lib().mrcnn_ap_sweep_caps(C.cast(caps, C.c_void_p)), "mrcnn_ap_sweep_caps")
        _ap_sweep_caps = dict(zip(("det", "gt", "thr", "cand"), (int(v) for v in caps)))
    return dict(_ap_sweep_caps)


def ap_sweep(det_box, det_off, gt_box, gt_off, thr):
    """The suffix tables of the sweep mAP for the N problems of a test set in one launch (include/mrcnn_hip.h: mrcnn_ap_sweep).
    Device tensors: det_box [D, 4] / gt_box [G, 4] float64 corner boxes, each problem's detections in ascending-score order, thr [T]
    float64 (all > 0, boxes well formed: the caller's contract).  det_off / gt_off: the CSR offsets of the N problems, NumPy
    (checked here) -- problem p owns rows off[p] .. off[p + 1].  Returns (tp [T * (D + N)] int32, status [N] int32) on the device:
    problem p's T x (P + 1) table starts at tp[T * (det_off[p] + p)]; a problem whose status is AP_SWEEP_OVER_CANDIDATES is the
    caller's to compute (its rows are zeros).  A problem past the row caps, or T past the threshold cap: ApSweepUnsupported, nothing
    launched.  No problem: a HipPathError."""
    import numpy as np
    _need_cuda(det_box, gt_box, thr)
    D, G, T = int(det_box.shape[0]), int(gt_box.shape[0]), int(thr.shape[0])
    assert det_box.dtype == gt_box.dtype == thr.dtype == torch.float64
    assert tuple(det_box.shape) == (D, 4) and tuple(gt_box.shape) == (G, 4) and thr.dim() == 1
    do = np.ascontiguousarray(det_off, dtype=np.int64).reshape(-1)
    go = np.ascontiguousarray(gt_off, dtype=np.int64).reshape(-1)
    N = do.size - 1
    if N < 1 or go.size != N + 1:
        raise _hip.HipPathError("ap_sweep: empty problem table")
    if do[0] != 0 or go[0] != 0 or do[-1] != D or go[-1] != G or np.any(np.diff(do) < 0) or np.any(np.diff(go) < 0):
        raise _hip.HipPathError("ap_sweep: malformed problem offsets")
    if T <= 0 or max(G, N) > 0x7FFFFFFF or T * (D + N) > 0x7FFFFFFF:
        raise _hip.HipPathError("ap_sweep: no threshold, or tables past int32 entries")
    caps = ap_sweep_caps()
    if T > caps["thr"]:
        raise ApSweepUnsupported("ap_sweep: %d thresholds are past the %d of mrcnn_ap_sweep" % (T, caps["thr"]))
    if int(np.diff(do).max()) > caps["det"] or int(np.diff(go).max()) > caps["gt"]:
        raise ApSweepUnsupported("ap_sweep: a problem of %d detections x %d ground truths is past the %d x %d of mrcnn_ap_sweep" % (
            int(np.diff(do).max()), int(np.diff(go).max()), caps["det"], caps["gt"]))
    dev = thr.device
    tp = torch.empty((T * (D + N),), dtype=torch.int32, device=dev)
    status = torch.empty((N,), dtype=torch.int32, device=dev)
    off_t = torch.from_numpy(np.concatenate([do, go]).astype(np.int32)).to(dev)
    tensors = [t.contiguous() for t in (det_box, gt_box, thr)]
    check(_hip.lib().mrcnn_ap_sweep(ptr(tensors[0]) if D else None, off_t.data_ptr(), D, ptr(tensors[1]) if G else None,
                                    off_t.data_ptr() + 4 * (N + 1), G, N, ptr(tensors[2]), T, ptr(tp), ptr(status), current_stream()),
          "mrcnn_ap_sweep")
    tp._keep = (off_t, tensors)               # alive until the caller has synchronised on the result
    return tp, status


class OutlineUnsupported(_hip.HipPathError):
    """A table past a cap of mrcnn_outline_* (include/mrcnn_hip.h: a source wider or higher than 8192 pixels, more than 65535
    sources, more than 2^22 contour segments in one source, int32 totals): the caller takes the host path."""


class Outlines(object):
    """Contours and pixel lists of n bit masks on the device (include/mrcnn_hip.h: mrcnn_outline_emit), coordinates in each
    source's own frame:
      points [P, 2] float32 (x, y); contour_offsets [C + 1] int32; source_contours [n + 1] int32 (the contours of source i);
      pixels [K, 2] int32 (y, x) in raster order; pixel_offsets [n + 1] int32.
    P and C are known on the device only: `points` and `contour_offsets` read C once (a synchronisation) to cut their buffers
    to size; `host()` downloads everything in one copy instead."""

    def __init__(self, points_buf, contour_offsets_buf, source_contours, pixels, pixel_offsets, segments):
        self._points_buf, self._contour_offsets_buf, self._segments, self._C = points_buf, contour_offsets_buf, int(segments), None
        self.source_contours, self.pixels, self.pixel_offsets = source_contours, pixels, pixel_offsets
        self.n = int(source_contours.shape[0]) - 1

    def _contours(self):
        if self._C is None:
            self._C = int(self.source_contours[-1])
        return self._C

    @property
    def points(self):
        return self._points_buf[:self._segments + self._contours()]

    @property
    def contour_offsets(self):
        return self._contour_offsets_buf[:self._contours() + 1]

    def host(self):
        """One download: dict of NumPy arrays under the five names above."""
        n, K, cc = self.n, int(self.pixels.shape[0]), int(self._contour_offsets_buf.shape[0])
        flat = torch.cat([self.source_contours, self.pixel_offsets, self._contour_offsets_buf, self.pixels.reshape(-1),
                          self._points_buf.view(torch.int32).reshape(-1)]).cpu().numpy()
        sc, po, co = flat[:n + 1], flat[n + 1:2 * n + 2], flat[2 * n + 2:2 * n + 2 + cc]
        rest = flat[2 * n + 2 + cc:]
        self._C = C_ = int(sc[-1])
        return {"source_contours": sc, "pixel_offsets": po, "contour_offsets": co[:C_ + 1], "pixels": rest[:2 * K].reshape(K, 2),
                "points": rest[2 * K:].view("<f4").reshape(-1, 2)[:self._segments + C_]}


def _outline_refusal(rc, what):
    if rc == ERR_UNSUPPORTED:
        raise OutlineUnsupported("%s: the table is past a cap of the kernels (status %d): a source above 8192 x 8192 pixels, more than "
                                 "65535 sources, more than 2^22 segments in a source, or totals past int32" % (what, rc))
    if rc:
        raise ValueError("%s refuses the table (status %d): no source, a negative size or a descriptor that leaves the pool" % (what, rc))


def bitmap_outlines(pool, desc, desc_host=None, timing=None):
    """Contours (find_contours at 0.5 of the zero-padded mask, as (x, y)) and pixel lists (np.argwhere) of n bit masks in one
    call: pool, desc as for tile_adjacency (pool of 32-bit words, desc [n, 6] int32 = (x0, y0, w, h, word_offset, words_per_row),
    both on the device; tile_union's out_pool / out_desc as they stand); desc_host = the NumPy descriptors behind `desc` (read
    back when not given).  Returns an Outlines.  Synchronises once, to read the per-source totals that size the outputs.
    ValueError for a malformed table, OutlineUnsupported past a cap; neither launches anything.  timing: a dict that receives
    the device time of the two launch groups (count_kernels_ms, emit_kernels_ms, from events; costs one more synchronisation)."""
    import numpy as np
    _need_cuda(pool, desc)
    assert desc.dtype == torch.int32 and desc.dim() == 2 and desc.shape[1] == 6 and desc.is_contiguous()
    assert pool.dim() == 1 and pool.element_size() == 4 and pool.is_contiguous()
    dh = np.ascontiguousarray(desc.cpu().numpy() if desc_host is None else desc_host, dtype=np.int32).reshape(-1, 6)
    n, dev, words = int(desc.shape[0]), pool.device, int(pool.numel())
    assert dh.shape[0] == n, "desc_host must be the host copy of desc"
    L = _hip.lib()
    host = dh.ctypes.data_as(C.c_void_p)
    _outline_refusal(L.mrcnn_outline_check(host, n, words, None), "mrcnn_outline_count")
    stream = current_stream()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)] if timing is not None else None
    cws = workspace(L.mrcnn_outline_workspace(host, n, words, None), dev, "outline_count")
    totals = torch.empty((n, 2), dtype=torch.int32, device=dev)
    pixel_offsets = torch.empty((n + 1,), dtype=torch.int32, device=dev)
    if ev:
        ev[0].record()
    check(L.mrcnn_outline_count(ptr(pool), words, host, ptr(desc), n, ptr(cws), cws.numel(), ptr(totals), ptr(pixel_offsets), stream),
          "mrcnn_outline_count")
    if ev:
        ev[1].record()
    th = np.ascontiguousarray(totals.cpu().numpy())                # the one synchronisation: sizes of everything below
    thost = th.ctypes.data_as(C.c_void_p)
    _outline_refusal(L.mrcnn_outline_check(host, n, words, thost), "mrcnn_outline_emit")
    S, K = int(th[:, 0].sum()), int(th[:, 1].sum())
    ews = workspace(L.mrcnn_outline_workspace(host, n, words, thost), dev, "outline_emit")
    points = torch.empty((S + S // 4 + 1, 2), dtype=torch.float32, device=dev)        # one spare row each: never an empty buffer
    contour_offsets = torch.zeros((S // 4 + 1,), dtype=torch.int32, device=dev)
    source_contours = torch.empty((n + 1,), dtype=torch.int32, device=dev)
    pixels = torch.empty((K + 1, 2), dtype=torch.int32, device=dev)
    if ev:
        ev[2].record()
    check(L.mrcnn_outline_emit(ptr(pool), words, host, ptr(desc), n, thost, ptr(cws), cws.numel(), ptr(ews), ews.numel(), ptr(pixel_offsets),
                               ptr(points), points.shape[0], ptr(contour_offsets), S // 4, ptr(source_contours), ptr(pixels), K, stream),
          "mrcnn_outline_emit")
    if ev:
        ev[3].record()
        ev[3].synchronize()
        timing["count_kernels_ms"] = round(ev[0].elapsed_time(ev[1]), 4)
        timing["emit_kernels_ms"] = round(ev[2].elapsed_time(ev[3]), 4)
        timing["segments"], timing["pixels"] = S, K
    return Outlines(points, contour_offsets, source_contours, pixels[:K], pixel_offsets, S)


def mask_plane_table(n, H, wpr, W):
    """mrcnn_tile_source records [n, 6] int32 of the bit planes of one frame (MaskPlanes.words as one pool)."""
    import numpy as np
    table = np.zeros((n, 6), np.int64)
    table[:, 2], table[:, 3], table[:, 5] = W, H, wpr
    table[:, 4] = np.arange(n, dtype=np.int64) * H * wpr
    if n and table[-1, 4] + H * wpr > 2 ** 31 - 1:
        raise OutlineUnsupported("mask_plane_outlines: %d planes of %d x %d words are past a pool of 2^31 - 1 words" % (n, H, wpr))
    return table.astype(np.int32)


def mask_plane_outlines(planes, timing=None):
    """bitmap_outlines of every plane of a MaskPlanes (the masks of one frame), full frame each."""
    _need_cuda(planes.words)
    table = mask_plane_table(planes.n, planes.H, planes.wpr, planes.W)
    if planes.n <= 0:
        raise ValueError("mask_plane_outlines: no plane")
    desc = torch.from_numpy(table).to(planes.words.device)
    return bitmap_outlines(planes.words.contiguous().view(-1), desc, table, timing)


class DrawUnsupported(_hip.HipPathError):
    """A scene past a cap of mrcnn_draw_overlay (include/mrcnn_hip.h: a frame side above 16384, a scale above 64, a canvas side
    above 65536 or a canvas above 2^31 - 1 bytes, more than 4096 items or texts, a text above 256 characters, more than 256
    colours, coordinates beyond +-2^20): the caller takes the host statement."""


def _draw_desc(H, W, n_planes, tables, scale):
    import numpy as np
    from . import draw
    items = np.ascontiguousarray(tables["items"], dtype=draw.ITEM_DTYPE).reshape(-1)
    texts = np.ascontiguousarray(tables["texts"], dtype=draw.TEXT_DTYPE).reshape(-1)
    glyphs = np.ascontiguousarray(tables["glyphs"], dtype=np.uint64).reshape(-1)
    palette = np.ascontiguousarray(tables["palette"], dtype=np.uint8)
    shade = tables.get("shade")
    if palette.ndim != 2 or palette.shape[1] != 4:
        raise ValueError("draw_overlay: palette must be [K, 4] uint8")
    if shade is not None:
        shade = np.ascontiguousarray(shade, dtype=np.uint8)
        if tuple(shade.shape) != (palette.shape[0], 3, 256):
            raise ValueError("draw_overlay: shade must be [K, 3, 256] uint8 for the K colours of the palette")
    d = _hip.DrawDesc(int(H), int(W), int(scale), int(n_planes), items.size, texts.size, glyphs.size, int(palette.shape[0]),
                      0 if shade is None else 1, 0)
    return d, items, texts, glyphs, palette, shade


def _draw_refusal(rc):
    if rc == ERR_UNSUPPORTED:
        raise DrawUnsupported("mrcnn_draw_overlay: the scene is past a cap of the kernel (status %d)" % rc)
    if rc:
        raise ValueError("mrcnn_draw_overlay refuses the tables (status %d): an unknown kind, a colour, plane or glyph index outside "
                         "its table, a glyph beyond 35 bits, or an empty frame" % rc)


def draw_check(H, W, n_planes, tables, scale):
    """The status mrcnn_draw_overlay would return for these tables (draw.device_tables); launches nothing."""
    d, items, texts, glyphs, _, _ = _draw_desc(H, W, n_planes, tables, scale)
    host = [a.ctypes.data_as(C.c_void_p) if a.size else None for a in (items, texts, glyphs)]
    return _hip.lib().mrcnn_draw_check(C.byref(d), *host)


def draw_overlay(image_u8, planes, tables, scale, timing=None):
    """The detection overlay (include/mrcnn_hip.h: mrcnn_draw_overlay) -> uint8 [scale (H + 4), scale (W + 4), 3]
    device tensor, equal to draw.render_host of the same scene byte for byte.  image_u8 [H, W, 3] uint8 on the device; planes: the
    MaskPlanes of the frame's masks (None when no item names a plane); tables: draw.device_tables(scene) -- NumPy tables, uploaded
    here in one copy.  ValueError for malformed tables, DrawUnsupported past a cap; neither launches anything.  timing: a dict
    that receives the kernel's device time (render_kernel_ms, from events; costs a synchronisation)."""
    import numpy as np
    _need_cuda(image_u8)
    assert image_u8.dtype == torch.uint8 and image_u8.dim() == 3 and image_u8.shape[2] == 3 and image_u8.is_contiguous()
    H, W = int(image_u8.shape[0]), int(image_u8.shape[1])
    n_planes = 0
    if planes is not None:
        _need_cuda(planes.words, planes.box)
        if (planes.H, planes.W) != (H, W):
            raise _hip.HipPathError("draw_overlay: image %r, planes %r" % ((H, W), (planes.H, planes.W)))
        assert planes.words.is_contiguous() and planes.box.is_contiguous() and planes.box.dtype == torch.int32
        n_planes = planes.n
    d, items, texts, glyphs, palette, shade = _draw_desc(H, W, n_planes, tables, scale)
    L = _hip.lib()
    host = [a.ctypes.data_as(C.c_void_p) if a.size else None for a in (items, texts, glyphs)]
    _draw_refusal(L.mrcnn_draw_check(C.byref(d), *host))
    # one upload: every table at an offset that is a multiple of 8
    parts, offs, at = [], [], 0
    for a in (glyphs, items, texts, palette, shade):
        raw = np.zeros(0, np.uint8) if a is None else a.view(np.uint8).reshape(-1)
        raw = np.concatenate([raw, np.zeros(-raw.size % 8, np.uint8)])
        offs.append(at)
        parts.append(raw)
        at += raw.size
    blob = torch.from_numpy(np.concatenate(parts + [np.zeros(8, np.uint8)])).to(image_u8.device)
    base = blob.data_ptr()
    dev = [base + o if a is not None and a.size else None for o, a in zip(offs, (glyphs, items, texts, palette, shade))]
    Hc, Wc = int(scale) * (H + 4), int(scale) * (W + 4)
    canvas = torch.empty((Hc, Wc, 3), dtype=torch.uint8, device=image_u8.device)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)] if timing is not None else None
    if ev:
        ev[0].record()
    check(L.mrcnn_draw_overlay(C.byref(d), host[0], host[1], host[2], ptr(image_u8), ptr(planes.words) if n_planes else None,
                               ptr(planes.box) if n_planes else None, dev[1], dev[2], dev[0], dev[3], dev[4], ptr(canvas),
                               current_stream()), "mrcnn_draw_overlay")
    if ev:
        ev[1].record()
        ev[1].synchronize()
        timing["render_kernel_ms"] = round(ev[0].elapsed_time(ev[1]), 4)
        timing["canvas_bytes"] = 3 * Hc * Wc
    canvas._keep = blob                      # alive until the caller has synchronised on the result
    return canvas


def fill_zero(t):
    _need_cuda(t)
    check(_hip.lib().mrcnn_fill_zero(ptr(t), t.numel() * t.element_size(), current_stream()), "mrcnn_fill_zero")


def mask_out_bwd(d_mask, mask, up, w_mask, dw_mask, db_mask, db_deconv):
    """Fused backward of sigmoid(conv1x1(relu(deconv))) -> dzg [M, H/2, W/2, 4*Cd]; the three small
    gradients accumulate in place."""
    _need_cuda(d_mask, mask, up, w_mask, dw_mask, db_mask, db_deconv)
    M, H, W, Cd = up.shape
    C_ = mask.shape[-1]
    dzg = empty((M, H // 2, W // 2, 4 * Cd), torch.float32, up.device)
    check(_hip.lib().mrcnn_mask_out_bwd(ptr(d_mask), ptr(mask), ptr(up), ptr(w_mask), ptr(dzg), ptr(dw_mask),
                                        ptr(db_mask), ptr(db_deconv), M, H, W, Cd, C_, current_stream()),
          "mrcnn_mask_out_bwd")
    return dzg


# ---- 16-bit matrix-core path (configs[4], stage 1: ROI-head convolutions) ---------------------------------------
_H16 = {torch.float16: 0, torch.bfloat16: 1}


def weights_to_h16(w, dtype=torch.float16, want_dgrad=True, out=None):
    """float32 HWIO kernel -> (W^T [Cout, KH*KW*Cin], data-gradient image [Cin, KH*KW*Cout]) in `dtype`.
    `out` = a pair returned by an earlier call: refreshed in place (addresses captured in HIP graphs stay valid)."""
    _need_cuda(w)
    KH, KW, Cin, Cout = w.shape
    if out is not None:
        wf, wd = out
        assert wf.dtype == dtype and tuple(wf.shape) == (Cout, KH * KW * Cin)
    else:
        wf = torch.empty((Cout, KH * KW * Cin), dtype=dtype, device=w.device)
        wd = torch.empty((Cin, KH * KW * Cout), dtype=dtype, device=w.device) if want_dgrad else None
    check(_hip.lib().mrcnn_weights_to_h16(ptr(w), ptr(wf), ptr(wd), KH, KW, Cin, Cout, _H16[dtype], current_stream()),
          "mrcnn_weights_to_h16")
    return wf, wd


# ---- Winograd F(2x2, 3x3) / F(4x4, 3x3), float32 (mask-head 3x3 convolutions) ---------------------------------------------
_WINO_MIN_ROWS = int(os.environ.get("MRCNN_WINOGRAD_MIN_ROWS", "16384"))   # 84 ROIs of 14 x 14: detect's 100 detections take the path (3.48 -> 3.18 ms/image)
# 4: F(4x4, 3x3) for layers of at least _WINO_TILE4_MIN_ROWS pixels (512 ROIs of 14 x 14: the training step's layers and their
# halves; detect's 100 ROIs per image stay on F(2x2, 3x3)); headline step 44.5 -> 40.9 ms.  2: F(2x2, 3x3) everywhere
_WINO_TILE = int(os.environ.get("MRCNN_WINOGRAD_TILE", "4"))
_WINO_TILE4_MIN_ROWS = int(os.environ.get("MRCNN_WINOGRAD_TILE4_MIN_ROWS", "100352"))


_WINO_MIXED = os.environ.get("MRCNN_WINOGRAD_MIXED", "1") != "0"          # tile 4 on maps with extent % 4 == 2: four groups, no overhang
TILE_MIXED = 6                                                              # "4 + 2": 4 x 4 tiles and a last row / column of 2


def winograd_tile(xshape):
    """Tiling of a TRAINING layer of this input shape: 2 (F(2x2,3x3) everywhere), 4 (F(4x4,3x3): 36 GEMMs over a quarter of the
    tiles, about one decimal digit less accurate: 1.3e-5 of the result's range against 1.6e-6) for layers of at least
    MRCNN_WINOGRAD_TILE4_MIN_ROWS pixels, or TILE_MIXED when H and W are 2 mod 4 (the mask head's 14 x 14): 4 x 4 tiles plus a
    last row / column of 4 x 2, 2 x 4 and 2 x 2 tiles -- 484 multiplications per map and channel pair where the uniform 4 x 4
    tiling with its overhang needs 576.  MRCNN_WINOGRAD_TILE=2 keeps 2 everywhere, MRCNN_WINOGRAD_MIXED=0 the uniform tiling.
    A pure function of the shape, so the forward pass, the data gradient and the weight gradient of a layer agree on it."""
    N, H, W, _ = xshape
    if not (_WINO_TILE == 4 and N * H * W >= _WINO_TILE4_MIN_ROWS):
        return 2
    return TILE_MIXED if (_WINO_MIXED and H % 4 == 2 and W % 4 == 2 and H > 4 and W > 4) else 4


def winograd_groups(H, W, tile):
    """The tile groups (mrcnn_wino_group) of an H x W map under a tiling."""
    G = _hip.WinoGroup
    if tile == 2:
        assert H % 2 == 0 and W % 2 == 0
        return [G(2, 2, H // 2, W // 2, 0, 0)]
    if tile == 4:
        return [G(4, 4, (H + 3) // 4, (W + 3) // 4, 0, 0)]
    assert tile == TILE_MIXED and H % 4 == 2 and W % 4 == 2
    return [G(4, 4, H // 4, W // 4, 0, 0), G(4, 2, H // 4, 1, 0, W - 2), G(2, 4, 1, W // 4, H - 2, 0), G(2, 2, 1, 1, H - 2, W - 2)]


class _WinoLayout(object):
    """The tile layout of N maps of H x W under a tiling, made once per (N, H, W, tile) by _wino_layout and only read afterwards:
    the groups, the transform-domain matrices nb of each, and per channel count -- asked of the library once -- the floats of each
    group's transform (V, Mt and dM alike: nb matrices of whole row tiles) and the rows of channel-sum partials each group's
    backward output transform writes, both with their prefix sums: a buffer of all groups end to end has group gi at offs[gi] and
    offs[-1] elements."""

    def __init__(self, N, H, W, tile):
        self.N, self.H, self.W, self.tile = N, H, W, tile
        self.groups = tuple(winograd_groups(H, W, tile))
        self.nbs = tuple((g.oth + 2) * (g.otw + 2) for g in self.groups)
        self.all = range(len(self.groups))
        self._floats, self._rows = {}, {}

    def _per_group(self, memo, entry, C_):
        if C_ not in memo:
            query = getattr(_hip.lib(), entry)
            ns = tuple(query(C.byref(g), self.N, C_) for g in self.groups)
            memo[C_] = (ns, tuple(sum(ns[:i]) for i in range(len(ns) + 1)))
        return memo[C_]

    def floats(self, C_):
        """(floats of each group's transform of C_ channels, their prefix sums)"""
        return self._per_group(self._floats, "mrcnn_winograd_group_floats", C_)

    def sum_rows(self, C_):
        """(rows of partials [3][C_] of each group, their prefix sums)"""
        return self._per_group(self._rows, "mrcnn_winograd_output_bwd_rows", C_)


_wino_layout = functools.lru_cache(maxsize=256)(_WinoLayout)


def _wino_weights_of(U):
    """U as winograd_weights made it, a tensor or -- the mixed tiling -- a list of four -> (tile, [U of each group], Cout)."""
    if isinstance(U, (list, tuple)):
        assert [u.shape[0] for u in U] == [36, 24, 24, 16], "U is not a mixed Winograd weight transform"
        return TILE_MIXED, U, U[0].shape[2]
    assert U.shape[0] in (16, 36), "U is not a Winograd weight transform"
    return (2 if U.shape[0] == 16 else 4), [U], U.shape[2]


def _wino_arg(t, ready):
    """The public 'a tensor, or -- where the caller holds its transform (v_ready / dm_ready / mt_ready) -- its SHAPE' argument ->
    (the tensor, None where it is not to be read; its shape)."""
    if isinstance(t, (tuple, list)):
        assert ready, "a shape stands for a tensor only where its transform is ready"
        return None, tuple(t)
    return (None if ready else t), tuple(t.shape)


def winograd_ok(xshape, wshape, stride=1, padding="same", min_rows=None):
    """Shapes the Winograd path takes: 3 x 3, stride 1, 'same' (or explicit 1, 1), even H and W, channels that fit the batched
    GEMM (Cin % 16, Cout % 128) and the transforms (multiples of 4), enough rows to fill the chip."""
    N, H, W, Cin = xshape
    kh, kw, cin, cout = wshape
    if min_rows is None:
        min_rows = _WINO_MIN_ROWS
    return (kh == 3 and kw == 3 and stride == 1 and padding in ("same", (1, 1)) and H % 2 == 0 and W % 2 == 0 and cin == Cin and
            Cin % 16 == 0 and cout % 128 == 0 and N * H * W >= min_rows and N * (H // 2) * (W // 2) * 16 * max(Cin, cout) < 2 ** 31)


def winograd_weights(w, out=None, tile=2):
    """HWIO 3 x 3 kernel -> U = G g G^T: [(tile + 2)^2, Cin, Cout] for the uniform tilings, a list of four (36, 24, 24, 16
    matrices) for TILE_MIXED."""
    kh, kw, cin, cout = w.shape
    assert kh == 3 and kw == 3 and w.is_contiguous()
    if tile != TILE_MIXED:
        _need_cuda(w, out)
        nb = (tile + 2) ** 2
        if out is None:
            out = torch.empty((nb, cin, cout), dtype=torch.float32, device=w.device)
        assert out.shape[0] == nb
        check(_hip.lib().mrcnn_winograd_weights(ptr(w), ptr(out), cin, cout, tile, current_stream()), "mrcnn_winograd_weights")
        return out
    shapes = ((4, 4), (4, 2), (2, 4), (2, 2))
    if out is None:
        out = [torch.empty(((a + 2) * (b + 2), cin, cout), dtype=torch.float32, device=w.device) for a, b in shapes]
    _need_cuda(w, *out)
    for (a, b), u in zip(shapes, out):
        assert u.shape[0] == (a + 2) * (b + 2)
        check(_hip.lib().mrcnn_winograd_weights_g(ptr(w), ptr(u), cin, cout, a, b, current_stream()), "mrcnn_winograd_weights_g")
    return out


# The stages, each one loop over the groups `gis` of a layout (default: all).  A transform of all groups lies end to end in one flat
# buffer (V, next_v, next_dm, a stacked Mt): group gi at the layout's prefix sum.  Where the public functions run the stages group
# by group (input transform, GEMM, output transform, then the next group), Mt and dM are per-stream scratch buffers of the largest
# group's size, reused group after group in stream order (stacked=False: every group at the buffer's start).
def _wino_input(lay, x, C_, V, gis=None):
    """B^T x B of x [N, H, W, C_] into the flat V."""
    lib, offs = _hip.lib(), lay.floats(C_)[1]
    for gi in lay.all if gis is None else gis:
        check(lib.mrcnn_winograd_input_g(ptr(x), ptr(V) + offs[gi] * 4, lay.N, lay.H, lay.W, C_, C.byref(lay.groups[gi]), current_stream()),
              "mrcnn_winograd_input_g")


def _wino_dy(lay, dz, C_, dM, stacked, gis=None):
    """A dz A^T of dz [N, H, W, C_] into dM."""
    lib, offs = _hip.lib(), lay.floats(C_)[1]
    for gi in lay.all if gis is None else gis:
        check(lib.mrcnn_winograd_dy_g(ptr(dz), ptr(dM) + (offs[gi] * 4 if stacked else 0), lay.N, lay.H, lay.W, C_, C.byref(lay.groups[gi]),
                                      current_stream()), "mrcnn_winograd_dy_g")


def _wino_product(lay, x, Us, Cin, V, Mt, stacked, gis=None):
    """Per group the input transform of x into V (x None: V holds it already), then the group's transform-domain GEMMs
    V [nb, rows, Cin] x U [nb, Cin, Cout] -> Mt [nb, rows, Cout]."""
    lib, cout = _hip.lib(), Us[0].shape[2]
    (nvs, voffs), moffs = lay.floats(Cin), lay.floats(cout)[1]
    for gi in lay.all if gis is None else gis:
        if x is not None:
            _wino_input(lay, x, Cin, V, (gi,))
        nb = lay.nbs[gi]
        check(lib.mrcnn_winograd_gemm(ptr(V) + voffs[gi] * 4, ptr(Us[gi]), ptr(Mt) + (moffs[gi] * 4 if stacked else 0), nb, nvs[gi] // (nb * Cin),
                                      Cin, cout, current_stream()), "mrcnn_winograd_gemm")


def _wino_output(lay, Mt, stacked, out, z_out, bias, scale, shift, act, gis=None):
    """Output transforms A^T Mt A with the forward epilogue into out (and z_out)."""
    lib, cout = _hip.lib(), out.shape[3]
    moffs = lay.floats(cout)[1]
    for gi in lay.all if gis is None else gis:
        check(lib.mrcnn_winograd_output_g(ptr(Mt) + (moffs[gi] * 4 if stacked else 0), ptr(out), ptr(z_out), ptr(bias), ptr(scale), ptr(shift),
                                          lay.N, lay.H, lay.W, cout, act, C.byref(lay.groups[gi]), current_stream()), "mrcnn_winograd_output_g")


def _wino_output_bwd(lay, Mt, stacked, out, below_out, below_z, scale, mean, rstd, zmask_shift, act, part, gis=None):
    """Output transforms with the epilogue backward of the layer below into out; zmask_shift (the forward's shift, or None): the ReLU
    mask is recomputed from z.  part (an address, or None): every group's workgroups write one row of channel-sum partials
    [3][cout] each, group gi from row sum_rows' prefix sum on."""
    lib, cout = _hip.lib(), out.shape[3]
    moffs, roffs = lay.floats(cout)[1], lay.sum_rows(cout)[1]
    for gi in lay.all if gis is None else gis:
        m = ptr(Mt) + (moffs[gi] * 4 if stacked else 0)
        p = None if part is None else part + roffs[gi] * 3 * cout * 4
        dims = (lay.N, lay.H, lay.W, cout)
        if zmask_shift is not None:
            check(lib.mrcnn_winograd_output_bwd_zmask_g(m, ptr(out), ptr(below_z), ptr(scale), ptr(zmask_shift), ptr(mean), ptr(rstd), p, *dims,
                                                        C.byref(lay.groups[gi]), current_stream()), "mrcnn_winograd_output_bwd_zmask_g")
        else:
            check(lib.mrcnn_winograd_output_bwd_g(m, ptr(out), ptr(below_out), ptr(below_z), ptr(scale), ptr(mean), ptr(rstd), p, *dims, act,
                                                  C.byref(lay.groups[gi]), current_stream()), "mrcnn_winograd_output_bwd_g")


def _wino_scratch(lay, Us, Cin, keep_v, stacked):
    """(V, Mt) of a layer: V of all groups in one flat buffer (keep_v: the caller's, kept for the weight gradient or written by the
    layer before), Mt for all groups end to end (stacked) or for the largest."""
    nv, nms, dev = lay.floats(Cin)[1][-1], lay.floats(Us[0].shape[2])[0], Us[0].device
    V = keep_v if keep_v is not None else workspace(nv * 4, dev, "winograd_v")[:nv * 4].view(torch.float32)
    assert keep_v is None or (keep_v.numel() == nv and keep_v.dtype == torch.float32)
    return V, workspace((sum(nms) if stacked else max(nms)) * 4, dev, "winograd_m")


def winograd_v_floats(xshape, tile=None):
    N, H, W, Cin = xshape
    return _wino_layout(N, H, W, winograd_tile(xshape) if tile is None else tile).floats(Cin)[1][-1]


def winograd_v_empty(xshape, device, tile=None):
    """A tensor for the input transform V of a layer of this input shape (or for A dz A^T of a dz of this shape)."""
    return empty((winograd_v_floats(xshape, tile),), torch.float32, device)


def conv2d_winograd(x, U, bias=None, scale=None, shift=None, act=ACT_NONE, out=None, z_out=None, keep_v=None, v_ready=False):
    """3 x 3 'same' stride-1 convolution with its epilogue through the Winograd domain (U = winograd_weights(w, tile=...)): per tile
    group the input transform, the group's transform-domain GEMMs and the output transform.  keep_v: V is written there (kept for
    the weight gradient).
    v_ready: keep_v already holds the input transform (conv2d_winograd_chain of the layer below wrote it) and x is the input's
    SHAPE: no input transform runs."""
    assert not v_ready or keep_v is not None
    x, (N, H, W, Cin) = _wino_arg(x, v_ready)
    _need_cuda(x, bias, scale, shift, out, z_out, keep_v)
    tile, Us, cout = _wino_weights_of(U)
    if out is None:
        out = empty((N, H, W, cout), torch.float32, Us[0].device)
    lay = _wino_layout(N, H, W, tile)
    V, Mt = _wino_scratch(lay, Us, Cin, keep_v, False)
    for gi in lay.all:
        _wino_product(lay, x, Us, Cin, V, Mt, False, (gi,))
        _wino_output(lay, Mt, False, out, z_out, bias, scale, shift, act, (gi,))
    return out


def winograd_chain_ok(xshape, cout, tile):
    """Layers conv2d_winograd_chain runs as one launch behind their GEMMs (mrcnn_winograd_chain's conditions): the mixed tiling,
    channels in whole 128s, a map of at most 2048 pixels."""
    _, H, W, _ = xshape
    return tile == TILE_MIXED and H % 4 == 2 and W % 4 == 2 and H > 4 and W > 4 and cout % 128 == 0 and H * W <= 2048


def conv2d_winograd_chain(x, U, next_v, bias=None, scale=None, shift=None, act=ACT_NONE, z_out=None, keep_v=None, v_ready=False):
    """conv2d_winograd(x, U, ...) of a layer whose activated output has ONE reader, the input transform of the next 3 x 3 layer
    (same tiling): the groups' GEMMs run first, into an Mt that holds all groups, then one launch applies the output transform and
    the epilogue (z_out) and writes the next layer's input transform into next_v (winograd_v_floats of this layer's output shape) --
    same bits as the separate launches; the activated output is not written.  The next layer runs as
    conv2d_winograd(shape, U2, ..., keep_v=next_v, v_ready=True).  Returns None, or -- where the one-launch kernel refuses the shape
    -- the activated output after the separate launches (output transforms, then the input transforms into next_v)."""
    assert not v_ready or keep_v is not None
    x, (N, H, W, Cin) = _wino_arg(x, v_ready)
    _need_cuda(x, bias, scale, shift, z_out, keep_v, next_v)
    tile, Us, cout = _wino_weights_of(U)
    lay = _wino_layout(N, H, W, tile)
    assert next_v.numel() == lay.floats(cout)[1][-1] and next_v.dtype == torch.float32
    V, Mt = _wino_scratch(lay, Us, Cin, keep_v, True)
    _wino_product(lay, x, Us, Cin, V, Mt, True)
    rc = _hip.lib().mrcnn_winograd_chain(ptr(Mt), ptr(z_out), ptr(bias), ptr(scale), ptr(shift), ptr(next_v), N, H, W, cout, act, tile,
                                         current_stream())
    if rc != ERR_UNSUPPORTED:
        check(rc, "mrcnn_winograd_chain")
        return None
    out = empty((N, H, W, cout), torch.float32, next_v.device)
    _wino_output(lay, Mt, True, out, z_out, bias, scale, shift, act)
    _wino_input(lay, out, cout, next_v)
    return out


def conv2d_dgrad_ep_winograd(dz, Ut, below_out, below_z, scale, mean, rstd, dgamma, dbeta, dbias, act, fwd_shift=None,
                             next_v=None, next_dm=None, dz_out=None, keep_v=None, v_ready=False, mt_ready=None):
    """Data gradient of a 3 x 3 'same' convolution (Ut = winograd_weights of the flipped / transposed kernel) fused with the
    epilogue backward of the layer below: returns dz_below, channel sums are added to dgamma / dbeta / dbias.
    fwd_shift: the shift of the layer below's forward epilogue out = max(scale * z + shift, 0) -- with it (and z, scale) the ReLU
    mask is recomputed from z, bit for bit the forward's decision, and below_out is not read (18 % of the pass's bytes).
    The chain form (next_v given: winograd_v_floats of dz_below's shape): dz_below has two readers, both transforms of it -- the
    input transform of the NEXT data gradient and A dz A^T of the layer below's weight gradient.  The groups' GEMMs run first into
    an Mt that holds all groups, then one launch (mrcnn_winograd_bwd_chain) applies the output transforms and the epilogue backward
    and writes both transforms, into next_v and next_dm (same size; None: not wanted) -- same bits as the separate launches;
    dz_below itself is stored only into dz_out (None: not at all).  The next data gradient then runs with its dz a SHAPE,
    keep_v=next_v, v_ready=True, the weight gradient as conv2d_wgrad_winograd(..., dm_ready=next_dm).  Returns dz_out, or --
    where the one-launch kernel refuses the shape or the epilogue -- dz_below after the separate launches (output transforms,
    then the input and dy transforms into next_v / next_dm).
    keep_v / v_ready: this data gradient's own input transform, written by the chain form of the layer above.
    mt_ready (chain form only): the transform-domain product Mt of all groups end to end, made by the caller -- no input transform
    and no GEMM runs, dz is a SHAPE and Ut only says the tiling and the channel count (the transforms take any channel count in
    whole 4s; the GEMM of this module wants whole 128s)."""
    chain = next_v is not None
    assert (mt_ready is None or chain) and (not v_ready or keep_v is not None)
    dz, (N, H, W, Cin) = _wino_arg(dz, v_ready or mt_ready is not None)
    _need_cuda(mt_ready, dz, below_out, below_z, scale, mean, rstd, dgamma, dbeta, dbias, fwd_shift, next_v, next_dm, dz_out, keep_v)
    tile, Us, cout = _wino_weights_of(Ut)
    dev = Us[0].device
    lay = _wino_layout(N, H, W, tile)
    lib = _hip.lib()
    zmask = act == ACT_RELU and fwd_shift is not None and below_z is not None and scale is not None
    if dgamma is None:
        mean = rstd = None
    # channel sums: every group's workgroups write one row of partials [3][cout] each into one per-stream buffer, group after
    # group (the one-launch kernel: one row per map); one launch after the last group adds the rows up (fixed order) onto dgamma /
    # dbeta / dbias
    want_sums = dgamma is not None or dbeta is not None or dbias is not None
    rows, roffs = lay.sum_rows(cout)
    assert min(rows) > 0, "channel count does not fit the Winograd data-gradient transform"
    part = ptr(workspace(max(roffs[-1], N if chain else 0) * 3 * cout * 4, dev, "winograd_bwd_sums")) if want_sums else None
    epilogue = (below_out, below_z, scale, mean, rstd, fwd_shift if zmask else None, act, part)
    n_rows = roffs[-1]
    if not chain:
        assert dz_out is None or tuple(dz_out.shape) == (N, H, W, cout)
        out = dz_out if dz_out is not None else empty((N, H, W, cout), torch.float32, dev)
        V, Mt = _wino_scratch(lay, Us, Cin, keep_v, False)
        for gi in lay.all:
            _wino_product(lay, dz, Us, Cin, V, Mt, False, (gi,))
            _wino_output_bwd(lay, Mt, False, out, *epilogue, (gi,))
    else:
        nm = lay.floats(cout)[1][-1]
        assert next_v.numel() == nm and next_v.dtype == torch.float32
        assert next_dm is None or (next_dm.numel() == nm and next_dm.dtype == torch.float32)
        Mt = mt_ready
        if Mt is None:
            V, Mt = _wino_scratch(lay, Us, Cin, keep_v, True)
            _wino_product(lay, dz, Us, Cin, V, Mt, True)
        rc = ERR_UNSUPPORTED
        if zmask:
            rc = lib.mrcnn_winograd_bwd_chain(ptr(Mt), ptr(below_z), ptr(scale), ptr(fwd_shift), ptr(mean), ptr(rstd), part, ptr(next_v),
                                              ptr(next_dm), ptr(dz_out), N, H, W, cout, tile, current_stream())
        if rc != ERR_UNSUPPORTED:
            check(rc, "mrcnn_winograd_bwd_chain")
            out, n_rows = dz_out, N
        else:
            out = dz_out if dz_out is not None else empty((N, H, W, cout), torch.float32, dev)
            _wino_output_bwd(lay, Mt, True, out, *epilogue)
            for gi in lay.all:
                _wino_input(lay, out, cout, next_v, (gi,))
                if next_dm is not None:
                    _wino_dy(lay, out, cout, next_dm, True, (gi,))
    if want_sums:
        check(lib.mrcnn_winograd_output_bwd_sums(part, n_rows, cout, ptr(dgamma), ptr(dbeta), ptr(dbias), current_stream()),
              "mrcnn_winograd_output_bwd_sums")
    return out


def conv2d_wgrad_winograd(V, xshape, dz, dw, accumulate=False, tile=None, dm_ready=None):
    """Weight gradient of a 3 x 3 'same' convolution through the Winograd domain: V = the forward's input transform of x
    (conv2d_winograd(..., keep_v=V)), dz [N, H, W, Cout] -> dw [3, 3, Cin, Cout] float32.  tile: the forward's (default:
    winograd_tile(xshape), what the forward chose for this shape).
    dm_ready: A dz A^T of all groups end to end, as the chain form of conv2d_dgrad_ep_winograd wrote it (next_dm): no transform of
    dz runs, and dz may be its SHAPE."""
    stacked = dm_ready is not None
    dz, dzshape = _wino_arg(dz, stacked)
    _need_cuda(V, dz, dw, dm_ready)
    N, H, W, Cin = xshape
    cout = dzshape[3]
    lay = _wino_layout(N, H, W, winograd_tile(xshape) if tile is None else tile)
    (nvs, voffs), (nms, moffs) = lay.floats(Cin), lay.floats(cout)
    assert V.numel() == voffs[-1], "V was made with another tiling"
    assert not stacked or (dm_ready.numel() == moffs[-1] and dm_ready.dtype == torch.float32), "dM was made with another tiling"
    dM_all = dm_ready if stacked else workspace(max(nms) * 4, V.device, "winograd_dm")[:max(nms) * 4].view(torch.float32)
    dU_all = workspace(36 * Cin * cout * 4, V.device, "winograd_du")
    for gi, g in enumerate(lay.groups):
        nb = lay.nbs[gi]
        rows = nms[gi] // (nb * cout)
        T = N * g.th_n * g.tw_n
        dU = dU_all[:nb * Cin * cout * 4].view(torch.float32).view(nb, Cin, cout)
        if not stacked:
            _wino_dy(lay, dz, cout, dM_all, False, (gi,))
        moff = moffs[gi] if stacked else 0
        dM = dM_all[moff:moff + nms[gi]].view(nb, rows, cout)
        Vv = V[voffs[gi]:voffs[gi] + nvs[gi]].view(nb, rows, Cin)
        items = [(Vv[k, :T].view(T, 1, 1, Cin), dM[k, :T].view(T, 1, 1, cout), (1, 1, Cin, cout), 1, "valid", dU[k].view(1, 1, Cin, cout), False)
                 for k in range(nb)]
        per = 16 if nb == 16 else 12                           # GEMMs per launch (+ one launch for their slab reductions): the argument block holds 16
        for i in range(0, nb, per):
            if not conv2d_wgrad_multi(items[i:i + per]):
                for x_, dy_, wshape, stride, padding, dw_, acc in items[i:i + per]:
                    conv2d_wgrad(x_, dy_, wshape, stride, padding, dw=dw_, accumulate=acc)
        check(_hip.lib().mrcnn_winograd_dw_g(ptr(dU), ptr(dw), Cin, cout, 1 if (accumulate or gi > 0) else 0, g.oth, g.otw, current_stream()),
              "mrcnn_winograd_dw_g")
    return dw


def h16_image_table(params, entries, device):
    """entries: [(w (a view into the flat float32 `params`), wf, wd or None)] -> (device table, n_layers, total_tiles) for
    weights_to_h16_batched.  The images' addresses are baked in: build it once the images exist and never move."""
    import numpy as np
    rec = np.zeros(len(entries), dtype=[("off", "<i8"), ("wf", "<u8"), ("wd", "<u8"), ("KH", "<i4"), ("KW", "<i4"), ("Cin", "<i4"),
                                        ("Cout", "<i4"), ("first", "<i4"), ("pad", "<i4")])
    tiles = 0
    for i, (w, wf, wd) in enumerate(entries):
        kh, kw, cin, cout = w.shape
        off = (w.data_ptr() - params.data_ptr()) // 4
        assert 0 <= off and off + w.numel() <= params.numel() and w.is_contiguous()
        rec[i] = (off, wf.data_ptr() if wf is not None else 0, wd.data_ptr() if wd is not None else 0, kh, kw, cin, cout, tiles, 0)
        tiles += kh * kw * ((cin + 31) // 32) * ((cout + 31) // 32)
    t = torch.from_numpy(rec.view(np.uint8).copy()).to(device)
    return t, len(entries), tiles


def weights_to_h16_batched(params, table, dtype):
    _need_cuda(params, table[0])
    check(_hip.lib().mrcnn_weights_to_h16_batched(ptr(params), ptr(table[0]), table[1], table[2], _H16[dtype], current_stream()),
          "mrcnn_weights_to_h16_batched")


def conv2d_h16(x, w_t, kshape, bias=None, scale=None, shift=None, stride=1, padding="same", act=ACT_NONE, z_out=None,
               out=None, res=None, out_strides=None):
    """16-bit convolution: x [N,H,W,Cin] half/bfloat16, w_t = W^T [Cout, KH*KW*Cin]; kshape = (KH, KW, Cin, Cout).
    res: 16-bit tensor of out's shape added before the activation; out_strides (n, h, w element strides): strided store
    into `out` (small-tile kernel)."""
    _need_cuda(x, w_t, bias, scale, shift, z_out, out, res)
    assert x.dtype in _H16 and w_t.dtype == x.dtype and (res is None or res.dtype == x.dtype)
    d = conv_desc(tuple(x.shape), tuple(kshape), stride, padding, act, RES_SAME if res is not None else RES_NONE)
    if out_strides is not None:
        assert out is not None
        d.out_n_stride, d.out_h_stride, d.out_w_stride = out_strides
    if out is None:
        out = empty((d.N, d.OH, d.OW, d.Cout), x.dtype, x.device)
    check(_hip.lib().mrcnn_conv2d_fwd_h16_res(C.byref(d), _H16[x.dtype], ptr(x), ptr(w_t), ptr(bias), ptr(scale), ptr(shift),
                                              ptr(res), ptr(out), ptr(z_out), current_stream()), "mrcnn_conv2d_fwd_h16")
    return out


def conv2d_dgrad_ep_h16(dz, w_t, kshape, padding, below_out, below_z, scale, mean, rstd, dgamma, dbeta, dbias, act,
                        grad_multiplier=1.0, res=None, want_dy=False):
    """16-bit data gradient fused with the epilogue backward of the layer below (mrcnn_conv2d_dgrad_ep_h16).  Returns
    dz_below (or (dz_below, dy)), or None when the shape has no fused kernel."""
    _need_cuda(dz, w_t, below_out, below_z, scale, mean, rstd, dgamma, dbeta, dbias, res)
    d = conv_desc(tuple(dz.shape), tuple(kshape), 1, padding, ACT_NONE, RES_SAME if res is not None else RES_NONE)
    ep = _hip.BwdEpilogueH16()
    ep.out, ep.z, ep.scale, ep.mean, ep.rstd = ptr(below_out), ptr(below_z), ptr(scale), ptr(mean), ptr(rstd)
    ep.dgamma, ep.dbeta, ep.dbias, ep.act = ptr(dgamma), ptr(dbeta), ptr(dbias), act
    out = empty((d.N, d.OH, d.OW, d.Cout), dz.dtype, dz.device)
    dy = empty((d.N, d.OH, d.OW, d.Cout), dz.dtype, dz.device) if want_dy else None
    ep.dy, ep.grad_multiplier = ptr(dy), float(grad_multiplier)
    rc = _hip.lib().mrcnn_conv2d_dgrad_ep_h16(C.byref(d), _H16[dz.dtype], ptr(dz), ptr(w_t), ptr(res), ptr(out), C.byref(ep),
                                              current_stream())
    if rc == ERR_UNSUPPORTED:
        return None
    check(rc, "mrcnn_conv2d_dgrad_ep_h16")
    return (out, dy) if want_dy else out


def conv2d_h16_supported(x_shape, kshape, stride=1, padding="same", res=False):
    d = conv_desc(tuple(x_shape), tuple(kshape), stride, padding)
    return bool(_hip.lib().mrcnn_conv2d_fwd_h16_supported(C.byref(d), 1 if res else 0))


def conv2d_h16_plan(d, dtype=torch.float16, x=16, w_t=16, bias=None, scale=None, shift=None, res=None, out=16, z_out=None, ep=None):
    """(status, _hip.H16Plan) of the launch conv2d_h16 (ep None) or conv2d_dgrad_ep_h16 (ep a _hip.BwdEpilogueH16; x = dz) would
    issue for the descriptor d.  Host only, like conv2d_plan: operands are addresses (or tensors, taken by their address), only
    their nullness and 16-byte alignment count, nothing is launched."""
    adr = lambda t: t if t is None or isinstance(t, int) else ptr(t)
    plan = _hip.H16Plan()
    rc = _hip.lib().mrcnn_conv2d_fwd_h16_plan(C.byref(d), _H16[dtype], adr(x), adr(w_t), adr(bias), adr(scale), adr(shift), adr(res),
                                              adr(out), adr(z_out), C.byref(ep) if ep is not None else None, C.byref(plan))
    return rc, plan


def conv2d_wgrad_h16_plan(d, dtype=torch.float16, x=16, dy=16, dw=16, workspace=256, workspace_bytes=None):
    """(status, _hip.H16WgradPlan) of the launch conv2d_wgrad_h16 would issue; host only.  workspace_bytes None: what
    conv2d_wgrad_h16 passes, mrcnn_conv2d_wgrad_h16_workspace(d)."""
    adr = lambda t: t if t is None or isinstance(t, int) else ptr(t)
    if workspace_bytes is None:
        workspace_bytes = _hip.lib().mrcnn_conv2d_wgrad_h16_workspace(C.byref(d))
    plan = _hip.H16WgradPlan()
    rc = _hip.lib().mrcnn_conv2d_wgrad_h16_plan(C.byref(d), _H16[dtype], adr(x), adr(dy), adr(dw), adr(workspace), workspace_bytes,
                                                C.byref(plan))
    return rc, plan


def deconv2x2_h16(x, w_t, bias, Cd, act=ACT_RELU):
    """Conv2DTranspose(2x2, stride 2) on 16-bit x [N,H,W,Cin]: w_t = W^T [4*Cd, Cin] of the GEMM matrix."""
    _need_cuda(x, w_t, bias)
    N, H, W, Cin = x.shape
    d = _hip.ConvDesc()
    d.N, d.H, d.W, d.Cin, d.Cout, d.KH, d.KW, d.stride, d.pad_t, d.pad_l = N, H, W, Cin, 4 * Cd, 1, 1, 1, 0, 0
    d.OH, d.OW, d.act, d.res_mode, d.out_mode, d.cmod = H, W, act, RES_NONE, OUT_DECONV2, Cd
    d.out_w_stride, d.out_h_stride, d.out_n_stride = Cd, 2 * W * Cd, 4 * H * W * Cd
    out = empty((N, 2 * H, 2 * W, Cd), x.dtype, x.device)
    check(_hip.lib().mrcnn_conv2d_fwd_h16(C.byref(d), _H16[x.dtype], ptr(x), ptr(w_t), ptr(bias), None, None, ptr(out), None,
                                          current_stream()), "mrcnn_conv2d_fwd_h16(deconv)")
    return out


def mask_out_fwd_h16(up, w_mask, b_mask):
    """sigmoid(1x1 conv) of the 16-bit deconvolution output -> float32 [M,H,W,C]."""
    _need_cuda(up, w_mask, b_mask)
    M, H, W, Cd = up.shape
    C_ = w_mask.shape[-1]
    out = empty((M, H, W, C_), torch.float32, up.device)
    check(_hip.lib().mrcnn_mask_out_fwd_h16(_H16[up.dtype], ptr(up), ptr(w_mask), ptr(b_mask), ptr(out), M * H * W, Cd, C_,
                                            current_stream()), "mrcnn_mask_out_fwd_h16")
    return out


def mask_out_bwd_h16(d_mask_out, mask_out, up, w_mask, dw_mask, db_mask, db_deconv, loss_scale):
    """One-pass backward of the mask-head output stage on a 16-bit `up`; returns dzg [M,H/2,W/2,4*Cd] (16 bit, scaled)."""
    _need_cuda(d_mask_out, mask_out, up, w_mask, dw_mask, db_mask, db_deconv)
    M, H, W, Cd = up.shape
    C_ = mask_out.shape[-1]
    dzg = empty((M, H // 2, W // 2, 4 * Cd), up.dtype, up.device)
    check(_hip.lib().mrcnn_mask_out_bwd_h16(_H16[up.dtype], ptr(d_mask_out), ptr(mask_out), ptr(up), ptr(w_mask), ptr(dzg),
                                            ptr(dw_mask), ptr(db_mask), ptr(db_deconv), M, H, W, Cd, C_, float(loss_scale),
                                            current_stream()), "mrcnn_mask_out_bwd_h16")
    return dzg


def conv2d_wgrad_h16(x, dy, w_shape, stride=1, padding="same", dw=None, accumulate=False, multiplier=1.0):
    """dw (float32 HWIO) from 16-bit x / dy; multiplier undoes a loss scale."""
    _need_cuda(x, dy, dw)
    assert x.dtype in _H16 and dy.dtype == x.dtype
    d = conv_desc(tuple(x.shape), tuple(w_shape), stride, padding)
    if dw is None:
        dw = empty(tuple(w_shape), torch.float32, x.device)
    nbytes = _hip.lib().mrcnn_conv2d_wgrad_h16_workspace(C.byref(d))
    ws = workspace(nbytes, x.device, "wgrad_h16")
    check(_hip.lib().mrcnn_conv2d_wgrad_h16(C.byref(d), _H16[x.dtype], ptr(x), ptr(dy), ptr(dw), ptr(ws), ws.numel(),
                                            1 if accumulate else 0, float(multiplier), current_stream()),
          "mrcnn_conv2d_wgrad_h16")
    return dw


def epilogue_bwd_h16(dout, out=None, z=None, scale=None, mean=None, rstd=None, dgamma=None, dbeta=None, dbias=None,
                     act=ACT_NONE, grad_multiplier=1.0, want_dy=False):
    """16-bit twin of epilogue_bwd: returns dz (same dtype as dout), or (dz, dy) with want_dy (dy = dout * act': the
    gradient a shortcut receives); channel sums go to the float32 gradients."""
    _need_cuda(dout, out, z, scale, mean, rstd, dgamma, dbeta, dbias)
    C_ = dout.shape[-1]
    M = dout.numel() // C_
    dz = empty(dout.shape, dout.dtype, dout.device)
    dy = empty(dout.shape, dout.dtype, dout.device) if want_dy else None
    check(_hip.lib().mrcnn_epilogue_bwd_h16_dy(_H16[dout.dtype], ptr(dout), ptr(out), ptr(z), ptr(scale), ptr(mean), ptr(rstd),
                                               ptr(dz), ptr(dy), ptr(dgamma), ptr(dbeta), ptr(dbias), M, C_, act,
                                               float(grad_multiplier), current_stream()), "mrcnn_epilogue_bwd_h16")
    return (dz, dy) if want_dy else dz


def cast_to_h16(src, dtype=torch.float16, out=None, multiplier=1.0):
    _need_cuda(src, out)
    if out is None:
        out = empty(src.shape, dtype, src.device)
    check(_hip.lib().mrcnn_cast_to_h16(ptr(src), ptr(out), src.numel(), _H16[dtype], float(multiplier), current_stream()),
          "mrcnn_cast_to_h16")
    return out


def cast_from_h16(src, multiplier=1.0, out=None):
    _need_cuda(src, out)
    if out is None:
        out = empty(src.shape, torch.float32, src.device)
    check(_hip.lib().mrcnn_cast_from_h16(ptr(src), ptr(out), src.numel(), _H16[src.dtype], float(multiplier),
                                         current_stream()), "mrcnn_cast_from_h16")
    return out


def axpy_from_h16(src, dst, multiplier=1.0):
    """dst (float32) += multiplier * src (16 bit), elementwise."""
    _need_cuda(src, dst)
    assert dst.dtype == torch.float32 and dst.numel() == src.numel()
    check(_hip.lib().mrcnn_axpy_from_h16(ptr(src), ptr(dst), src.numel(), _H16[src.dtype], float(multiplier), current_stream()),
          "mrcnn_axpy_from_h16")
    return dst
