"""Device-side execution of the Mask R-CNN graph wired by MaskRCNN.build (mrcnn/model.py:1935-2166):
forward (inference and training), the hand-derived backward pass, and the optimiser step
(MaskRCNN.compile, mrcnn/model.py:2255-2291).  Every arithmetic step is a launch into
libmrcnn_hip.so; torch only owns the buffers.

Gradient plumbing conventions
  * all parameter gradients live in one flat buffer (params.ParamLayout) that is zeroed per step;
    bias / BatchNorm gamma,beta gradients are accumulated by the epilogue-backward kernel;
  * a tensor consumed by several ops gets its gradient summed by chaining: every data-gradient
    convolution can add an existing buffer in its epilogue (res_mode SAME, in place);
  * the ROIAlign adjoints scatter-add into zero-initialised pyramid gradients first.
"""
import collections
import contextlib
import gc
import operator
from functools import partial
import os
import numpy as np
import torch

from . import ops
from . import _hip as _hip_mod
from ._hip import ACT_NONE, ACT_RELU, ACT_SIGMOID, RES_NONE, RES_SAME, RES_UP2
from .params import ParamLayout, deconv_gemm_to_keras, deconv_keras_to_gemm, granule_coefficients, init_weights

# configs[4], stage 3: besides the mask head, these layers run on the 16-bit matrix cores when head_dtype is set (and
# their shapes fit the 16-bit kernels): the FPN smoothing convolutions, the shared RPN convolution over all five levels,
# and the two FC layers of the class head (K = 12 544: weight-bandwidth halves) -- 82 of the 161 GFLOP per image of the
# 512 x 512 trunk.  float32 at their boundaries (casts), float32 master weights, accumulation and gradients.
H16_WIDE_LAYERS = ("fpn_p2", "fpn_p3", "fpn_p4", "fpn_p5", "rpn_conv_shared", "mrcnn_class_conv1", "mrcnn_class_conv2")

LOSS_NAMES = ("rpn_class_loss", "rpn_bbox_loss", "mrcnn_class_loss", "mrcnn_bbox_loss", "mrcnn_mask_loss")


# What a layer's forward pass leaves for its backward pass.  The forward pass is the only writer; the backward pass decides from
# these fields alone, never from the engine's switches.  path: the kernels the forward ran -- the direct float32 ones, the
# Winograd domain, or the 16-bit matrix cores (x, z, out are 16-bit tensors then).  V: the Winograd input transform kept for
# the weight gradient (winograd_wgrad), else None.
DIRECT, WINO, H16 = "direct", "winograd", "h16"
Ctx = collections.namedtuple("Ctx", "x z out act path V", defaults=(DIRECT, None))
# a bottleneck block: the contexts of its 2a, 2b, 2c and shortcut (None: identity) convolutions, and whether it ran in 16 bits
BlockCtx = collections.namedtuple("BlockCtx", "a b c shortcut h16")


_on = lambda s: s != "0"        # an environment switch is on unless it is "0"

# The engine's switches: (attribute, environment variable or None, default, parser, paths that read it: "t" the training step,
# "i" inference, "" construction only).  __init__ reads them once; they stay plain attributes that tests and bench.py flip
# between calls, so a recorded step is keyed by the "t" switches (_mode_key) and a captured inference graph by the "i" ones.
SWITCHES = (
    # BASELINE configs[4], stage 1: torch.float16 / torch.bfloat16 runs the four 3x3 convolutions of the mask head (forward, data
    # and weight gradient) on the 16-bit matrix cores; master weights, accumulation and every gradient buffer stay float32.
    # None = float32 everywhere.  loss_scale guards float16 gradients.
    ("head_dtype", None, None, None, "ti"),
    ("sparse_mask_bwd", None, True, None, "t"),                 # skip the exactly-zero rows of the mask-head backward
    ("h16_wide", "MRCNN_H16_WIDE", True, _on, "ti"),            # False: only the mask head in 16 bits (round-1 stages 1-2)
    ("h16_blocks", "MRCNN_H16_BLOCKS", True, _on, "ti"),        # bottleneck blocks in 16 bits (stage 4)
    ("h16_all_blocks", "MRCNN_H16_ALL_BLOCKS", True, _on, "ti"),    # False: only the identity blocks of res4 / res5
    ("h16_fused_bwd", "MRCNN_H16_FUSED_BWD", True, _on, "t"),   # 16-bit data gradients carry the lower layer's epilogue backward
    ("h16_roialign", "MRCNN_H16_ROIALIGN", True, _on, "ti"),    # ROI heads gather from the 16-bit pyramid (mrcnn_roialign_*_h16)
    # the persistent 256 x 256 16-bit kernel for the mask head's DATA gradients too (they run beside the weight gradients of the
    # other stream; False keeps them on the small-LDS kernel that shares CUs)
    ("h16_phase_bwd", "MRCNN_H16_PHASE_BWD", True, _on, "t"),
    # Winograd F(2x2, 3x3) for the float32 3x3 convolutions of the mask head (forward and data gradients): 2.25 x fewer
    # matrix-core flops through three launches per layer; False keeps the direct kernels
    ("winograd", "MRCNN_WINOGRAD", True, _on, "ti"),
    ("winograd_wgrad", "MRCNN_WINOGRAD_WGRAD", True, _on, "t"),     # weight gradients through the same domain
    # training mask head: a layer's output transform, epilogue and the next layer's input transform in one launch; the activated
    # output in between is not written (ops.conv2d_winograd_chain).  False: the separate launches (A/B)
    ("winograd_chain", "MRCNN_WINOGRAD_CHAIN", True, _on, "t"),
    # its backward twin: the data gradient's output transform + epilogue backward and BOTH transforms of that dz (the next data
    # gradient's input transform, the weight gradient's A dz A^T) in one launch; dz in between is not written
    # (ops.conv2d_dgrad_ep_winograd's chain form).  False: the separate launches (A/B)
    ("winograd_bwd_chain", "MRCNN_WINOGRAD_BWD_CHAIN", True, _on, "t"),
    # the trunk's large 3x3 layers (FPN smoothing, RPN shared convolution on levels of >= trunk_winograd_min_rows pixels)
    # through F(2x2, 3x3) in the forward pass (A/B switch, see DESIGN 4.1e for the measurement)
    ("trunk_winograd", "MRCNN_WINOGRAD_TRUNK", True, _on, "ti"),
    ("trunk_winograd_min_rows", "MRCNN_WINOGRAD_TRUNK_MIN_ROWS", 4096, int, "ti"),
    # the mask head of the inference graph: 4 = uniform F(4x4, 3x3) tiles (16 overhanging tiles per 14 x 14 map: 36 x 1600 GEMM rows
    # for 100 detections where F(2x2) has 16 x 4900; 1.3e-5 of the result's range instead of 1.6e-6, on probabilities that are
    # thresholded at 0.5) -- detect graph 2.73 -> 2.60 ms; 2 = F(2x2) as in rounds 1-2
    ("infer_mask_tile", "MRCNN_WINOGRAD_INFER_MASK_TILE", 4, int, "i"),
    # the 16 x 16-tile single-launch kernel for the layers of a few hundred pixels of the inference trunk (see infer)
    ("sk16_infer", "MRCNN_SK16_INFER", True, _on, "i"),
    # float32 mask head: the mrcnn_mask 1x1 convolution and its sigmoid in the epilogue of the deconvolution's GEMM
    # (ops.deconv2x2_mask); False: the two launches (A/B)
    ("fused_mask_out_fwd", "MRCNN_MASK_OUT_FWD_FUSED", True, _on, "ti"),
    ("fused_mask_out_bwd", None, True, None, "t"),              # single-pass backward of the mask-head output stage
    ("fused_dgrad_epilogue", None, True, None, "t"),            # mask-head data-gradient convs apply the lower layer's epilogue bwd
    ("gather_roialign_bwd", "MRCNN_GATHER_ROIALIGN_BWD", True, _on, "t"),   # class-head ROIAlign adjoint in gather form
    ("multi_launch", "MRCNN_MULTI_LAUNCH", True, _on, "ti"),    # independent small convolutions share launches
    # stream priorities (HIP: -1 high, 0 normal, 1 low where the runtime has three levels): the weight gradients are off the
    # critical path, so their stream may be given a lower priority than the chain of data gradients it runs beside
    ("wgrad_prio", "MRCNN_WGRAD_PRIO", 0, int, ""),
    ("aux_prio", "MRCNN_AUX_PRIO", 0, int, ""),
)
_TRAIN_SWITCHES = operator.attrgetter(*(s[0] for s in SWITCHES if "t" in s[4]))
_INFER_SWITCHES = operator.attrgetter(*(s[0] for s in SWITCHES if "i" in s[4]))
# config values infer() passes by value into its launches (with RPN_BBOX_STD_DEV / BBOX_STD_DEV: infer_graphed's key)
_INFER_CFG = operator.attrgetter("PRE_NMS_LIMIT", "POST_NMS_ROIS_INFERENCE", "RPN_NMS_THRESHOLD", "DETECTION_MAX_INSTANCES",
                                 "DETECTION_MIN_CONFIDENCE", "DETECTION_NMS_THRESHOLD")


@contextlib.contextmanager
def _capture(graph):
    """torch.cuda.graph(graph) with the garbage collector out of the way: this torch no longer collects before a capture
    (torch.compiler.config.force_cudagraph_gc), and a dead cycle that owns a CUDAGraph, a stream or device memory (an earlier
    engine) freed by a collection that happens to run INSIDE the capture makes hipGraphExecDestroy / hipFree fail under the global
    capture mode -- thrown from a destructor, which aborts the process.  Collect before, keep the collector off while capturing."""
    gc.collect()
    was = gc.isenabled()
    gc.disable()
    try:
        with torch.cuda.graph(graph):
            yield
    finally:
        if was:
            gc.enable()


@contextlib.contextmanager
def _tuning(key, value, restore, on=True):
    """A process-wide tuning value of the kernel library (ops.tuning_set) for the launches issued inside, put back to
    `restore` afterwards; on=False leaves it alone."""
    if on:
        ops.tuning_set(key, value)
    try:
        yield
    finally:
        if on:
            ops.tuning_set(key, restore)


class ConvOp(object):
    """One named Conv2D/Dense(+BatchNorm) layer: views into the flat buffers + fwd/bwd launches."""

    def __init__(self, model, spec):
        L = model.layout
        self.model = model
        self.spec = spec
        self.name = spec.name
        off, n, shape = L.offsets[spec.name + "/kernel"]
        if spec.kind == "deconv":                       # [Cin, (a,b,co)] GEMM == 1x1 conv Cin -> 4*Cd
            self.wshape = (1, 1, shape[0], shape[1] * shape[2] * shape[3])
        else:
            self.wshape = tuple(shape)
        kh, kw, cin, cout = self.wshape
        self.w = model.params[off:off + n].view(self.wshape)
        self.dw = model.grads[off:off + n].view(self.wshape)
        self.wt = model.wt[off:off + n].view(kh, kw, cout, cin)
        boff, bn_, _ = L.offsets[spec.name + "/bias"]
        self.b = model.params[boff:boff + bn_]
        self.db = model.grads[boff:boff + bn_]
        self.stride, self.padding = spec.stride, spec.padding
        self.bn = spec.bn
        self.scale = self.shift = self.mean = self.rstd = self.dgamma = self.dbeta = None
        if spec.bn:
            c0, c = L.bn_channel_offset[spec.bn], spec.shape[3]
            self.scale, self.shift = model.bn_scale[c0:c0 + c], model.bn_shift[c0:c0 + c]
            self.mean, self.rstd = model.bn_mean[c0:c0 + c], model.bn_rstd[c0:c0 + c]
            self.dgamma = model.grads[L.gamma_offset + c0:L.gamma_offset + c0 + c]
            self.dbeta = model.grads[L.beta_offset + c0:L.beta_offset + c0 + c]

    @property
    def dgrad_padding(self):
        """Padding of this layer's stride-1 data-gradient convolution (the flipped / transposed kernel over dz)."""
        kh, kw = self.wshape[:2]
        return ((kh - 1) // 2, (kw - 1) // 2) if self.padding == "same" else "valid"

    # ---- forward ---------------------------------------------------------------------------
    def forward(self, x, act=ACT_NONE, res=None, res_mode=RES_NONE, train=False):
        z = None
        d = ops.conv_desc(tuple(x.shape), self.wshape, self.stride, self.padding, act, res_mode)
        out = ops.empty((d.N, d.OH, d.OW, d.Cout), torch.float32, x.device)
        if train and self.bn:
            z = ops.empty_like(out)
        ops.conv2d(x, self.w, self.b, self.scale, self.shift, res, out=out, z_out=z, desc=d)
        return out, (Ctx(x, z, out, act) if train else None)

    # ---- backward pieces ---------------------------------------------------------------------
    def epilogue_bwd(self, dout, ctx, want_dy=False):
        """Returns (dz, dy): gradient w.r.t. the raw conv output, and (optionally) the gradient after
        the activation mask, which is what a residual input receives."""
        if self.bn is None and ctx.act == ACT_NONE:
            ops.epilogue_bwd(dout, dbias=self.db)
            return dout, dout
        dz = ops.empty_like(dout)
        dy = ops.empty_like(dout) if want_dy else None
        ops.epilogue_bwd(dout, ctx.out if ctx.act != ACT_NONE else None, ctx.z, self.scale, self.mean, self.rstd, dy, dz,
                         self.dgamma, self.dbeta, self.db, ctx.act)
        return dz, dy

    def wgrad(self, dz, ctx, accumulate=False):
        self.model.wgrad_async(ctx.x, dz, self.wshape, self.stride, self.padding, self.dw, accumulate)

    def wgrad_item(self, dz, ctx, accumulate=False):
        """The arguments of this layer's weight gradient, for MaskRCNNEngine.wgrad_group."""
        return (ctx.x, dz, self.wshape, self.stride, self.padding, self.dw, accumulate)

    def dgrad(self, dz, ctx, out=None, accumulate=False):
        """dx = adjoint of the convolution applied to dz.  `out` (shape of x) receives the result;
        accumulate=True adds to what `out` already holds (in place)."""
        x = ctx.x
        kh, kw, cin, cout = self.wshape
        N, H, W, _ = x.shape
        res = out if accumulate else None
        rm = RES_SAME if accumulate else RES_NONE
        if self.stride == 1 and (self.padding == "same" or (kh == 1 and kw == 1)):
            if out is None:
                out = ops.empty_like(x)
            ops.conv2d(dz, self.wt, res=res, stride=1, padding=self.dgrad_padding, res_mode=rm, out=out)
        elif kh == 1 and kw == 1 and self.stride == 2:
            if out is None:
                out = ops.empty_like(x)
                ops.fill_zero(out)
            d = ops.conv_desc(tuple(dz.shape), (1, 1, cout, cin), 1, "valid", ACT_NONE, rm)
            d.out_w_stride, d.out_h_stride, d.out_n_stride = 2 * cin, 2 * W * cin, H * W * cin
            ops.conv2d(dz, self.wt, res=res, out=out, desc=d)
        elif self.padding == "valid" and x.shape[1] == kh and x.shape[2] == kw:
            # "FC as VALID conv" (mrcnn_class_conv1): dx[M, (kh,kw,ci)] = dz[M, Cout] . W^T
            if out is None:
                out = ops.empty_like(x)
            wt2 = self.wt.view(1, 1, cout, kh * kw * cin)
            ops.conv2d(dz.view(N, 1, 1, cout), wt2, res=None if res is None else res.view(N, 1, 1, -1), stride=1,
                       padding="valid", res_mode=rm, out=out.view(N, 1, 1, kh * kw * cin))
        else:
            raise NotImplementedError("dgrad for layer %s" % self.name)
        return out


class Block(object):
    def __init__(self, model, stage, letter, has_shortcut, stride):
        base = "res%d%s_branch" % (stage, letter)
        self.c2a, self.c2b, self.c2c = model.op(base + "2a"), model.op(base + "2b"), model.op(base + "2c")
        self.c1 = model.op(base + "1") if has_shortcut else None
        self.stage, self.stride = stage, stride


_SIDE_STREAMS = {}


def _side_streams(device, wprio=0, aprio=0):
    """The weight-gradient and auxiliary streams of a device: ONE pair per process, shared by every engine.  HIP maps streams
    onto a handful of hardware queues (4 by default) in the order they are first used, and two streams that land on the same
    queue run one after the other.  The first pair created in a process gets queues of its own beside the default stream's;
    a later engine that took fresh streams of its own could land its weight-gradient stream on the main stream's queue --
    measured: the 512 x 512 16-bit step 24.0 -> 29.1 ms for the third model built in one process (bench.py's configs[4] leg
    behind the detect / train-loop legs), back to 24.6 with GPU_MAX_HW_QUEUES=8.  Engines never run concurrently with each
    other on one device, so sharing costs nothing."""
    dev = torch.device(device)
    if dev.type != "cuda":
        return None, None
    key = (dev.index if dev.index is not None else torch.cuda.current_device(), wprio, aprio)
    if key not in _SIDE_STREAMS:
        _SIDE_STREAMS[key] = (torch.cuda.Stream(device=dev, priority=wprio), torch.cuda.Stream(device=dev, priority=aprio))
    return _SIDE_STREAMS[key]


class MaskRCNNEngine(object):
    def __init__(self, config, device, weights=None, seed=0):
        self.cfg = config
        self.dev = device
        self.layout = L = ParamLayout(config)
        n = L.total
        f = dict(dtype=torch.float32, device=device)
        self.params = torch.zeros(n, **f)
        self.grads = torch.zeros(n, **f)
        self.momentum = torch.zeros(n, **f)
        self.wt = torch.empty(n, **f)
        c = max(L.bn_channels, 64)
        self.bn_mean, self.bn_var = torch.zeros(c, **f), torch.ones(c, **f)
        self.bn_scale, self.bn_shift, self.bn_rstd = torch.empty(c, **f), torch.empty(c, **f), torch.empty(c, **f)
        self.sumsq = torch.zeros(1, **f)
        self._ops = {}
        for l in L.layers:
            self._ops[l.name] = ConvOp(self, l)
        arch = config.BACKBONE
        n4 = {"resnet50": 5, "resnet101": 22, "custom": 1}[arch]
        letters = {2: "abc", 3: "abcd", 4: "a" + "".join(chr(98 + i) for i in range(n4)), 5: "abc"}
        self.stages = [[Block(self, s, b, i == 0, 2 if (i == 0 and s > 2) else 1) for i, b in enumerate(letters[s])]
                       for s in (2, 3, 4, 5)]
        # data-gradient operands (flipped / transposed kernels) of all layers: one table-driven launch per step
        entries = []
        for l in L.layers:
            o = self._ops[l.name]
            kh, kw, cin, cout = o.wshape
            off = L.offsets[l.name + "/kernel"][0]
            if o.padding == "valid" and kh > 1:                    # FC as VALID conv: plain [K, Cout] transpose
                entries.append((off, 1, 1, kh * kw * cin, cout))
            else:
                entries.append((off, kh, kw, cin, cout))
        self._flip_table = ops.flip_table(entries, device) if torch.device(device).type == "cuda" else None
        self.arena = ops.StepArena()               # tensors of a training step, reused step after step
        if torch.device(device).type == "cuda":
            from . import _hip
            _hip.set_device_index(torch.device(device).index if torch.device(device).index is not None
                                  else torch.cuda.current_device())
        self._gen, self._wt_gen = 0, -1     # weight generation (params_changed) and the one the flipped kernels were built from
        self.set_trainable("all")
        self.set_weights(weights if weights is not None else init_weights(L, seed))
        self._anchor_cache = {}
        self._infer_graphs = {}
        self._train_graphs = {}
        self._train_tapes = {}
        # contiguous gradient ranges in the order the backward pass finalises them (for overlapped
        # data-parallel reduction): heads+RPN+FPN kernels, then res5..res2, then conv1 + BatchNorm blocks
        first = lambda prefix: min(o for n_, (o, _, _) in L.offsets.items() if n_.startswith(prefix) and "/kernel" in n_)
        s2, s3, s4, s5, fp = first("res2"), first("res3"), first("res4"), first("res5"), first("fpn_")
        hd = first("mrcnn_")
        self.grad_ranges = {"heads": (hd, L.gamma_offset), "tail": (fp, hd), 5: (s5, fp), 4: (s4, s5), 3: (s3, s4),
                            2: (s2, s3), "head": (0, s2), "bn": (L.gamma_offset, L.total)}
        self.grad_ready = None          # callable(start, end) or None
        self.class_weights = None       # [C] device buffer of set_class_weights, or None: the head losses are unweighted
        self.forced_rpn_rois = None     # test hook: [B, POST_NMS_ROIS_TRAINING, 4] used instead of the ProposalLayer's output
        self.loss_scale = 4096.0
        self.skipped_steps = torch.zeros(1, dtype=torch.int32, device=device)   # steps the guarded optimiser refused (float16)
        self._skipped_seen = 0
        for name, env, default, parse, _ in SWITCHES:
            v = os.environ.get(env) if env else None
            setattr(self, name, default if v is None else parse(v))
        self._h16, self._h16_gen = {}, None     # 16-bit images of head_dtype, and the (weight generation, dtype) they hold
        self._wino = {}                 # (layer, tile, 0 forward / 1 data gradient) -> [U, weight generation]; stable addresses
        self._wino_reads = set()        # keys of _wino read since infer_graphed last cleared it
        self._h16_store = {}            # dtype -> {layer: (W^T image, data-gradient image)}, stable addresses
        self._h16_tables = {}           # (dtype, layer names) -> table of the one-launch refresh (ops.h16_image_table)
        self.wgrad_stream, self.aux_stream = _side_streams(device, self.wgrad_prio, self.aux_prio)
        if self.wgrad_stream is None:           # the step is written for three streams: there is no single-stream form of it
            raise _hip_mod.HipPathError("MaskRCNNEngine needs a GPU device for its side streams, not %r" % (device,))

    def op(self, name):
        return self._ops[name]

    # ---- work on a side stream ---------------------------------------------------------------------
    def _fork(self, side, body, *operands):
        """body() on the stream `side`, behind everything the current stream has been given so far; returns what body returns.
        `operands`: the tensors of the current stream that body reads, kept from reuse until `side` is done with them.  The ONE
        place where work leaves the main stream; joining again -- join_wgrad, a stream_wait -- is the caller's."""
        ev = _hip_mod.ev_record(torch.cuda.current_stream(self.dev))
        with torch.cuda.stream(side):
            _hip_mod.ev_wait(side, ev)
            out = body()
        for t in operands:
            t.record_stream(side)
        return out

    def _settle(self, body):
        """body() on a fresh stream beside the current one, which then waits for it: the eager passes before a capture."""
        side = torch.cuda.Stream(device=self.dev)
        self._fork(side, body)
        _hip_mod.stream_wait(torch.cuda.current_stream(self.dev), side)

    # ---- weight gradients on a second stream -------------------------------------------------------
    def wgrad_async(self, x, dz, wshape, stride, padding, dw, accumulate):
        """A layer's weight gradient depends only on (x, dz); nothing in the backward chain reads it.  It is
        launched on a side stream so that it overlaps the data-gradient convolution of the same layer: the
        partial last round of one grid (and the small grids of the backbone) fill the CUs the other leaves
        idle.  All weight gradients share that one stream (and its slab workspace), in program order."""
        self._fork(self.wgrad_stream, partial(ops.conv2d_wgrad, x, dz, wshape, stride, padding, dw=dw, accumulate=accumulate),
                   x, dz)

    def wgrad_group(self, items):
        """Weight gradients of several layers (ConvOp.wgrad_item) behind one event: one shared launch when they all
        fit the LDS-DMA kernel (the three convolutions of a bottleneck block on the small feature maps), else one by one."""
        def run():
            if not (self.multi_launch and 1 < len(items) <= 4 and ops.conv2d_wgrad_multi(items)):
                for x, dz, wshape, stride, padding, dw, acc in items:
                    ops.conv2d_wgrad(x, dz, wshape, stride, padding, dw=dw, accumulate=acc)
        self._fork(self.wgrad_stream, run, *(t for item in items for t in item[:2]))

    # ---- images derived from the weights ------------------------------------------------------------
    # The flipped / transposed kernels (wt), the 16-bit operand images and the Winograd-domain kernels U remember the weight
    # generation they were built from; where one is read while stale it is rebuilt in place (captured graphs and recorded
    # tapes hold its address).  The folded BatchNorm is rebuilt at once.
    def params_changed(self, fold=True):
        """The one way a change of `params` (set_weights, the optimiser step, a replayed step, a roll-back) reaches the derived
        images: a new weight generation.  fold=False: the replayed step already folded BatchNorm inside the recording."""
        self._gen += 1
        if fold:
            self.fold_bn()

    # compatibility shim: an assignment to either marks every derived image stale (`eng.wt_valid = eng._h16_valid = False`,
    # then fold_bn(), after writing params directly)
    wt_valid = _h16_valid = property(fset=lambda self, _: self.params_changed(fold=False))

    def refresh_wt(self):
        """Flipped / transposed kernels of every layer from the current parameters (one launch), when stale."""
        if self._wt_gen != self._gen:
            ops.weight_flip_transpose_batched(self.params, self.wt, self._flip_table)
            self._wt_gen = self._gen

    def _wino_U(self, op, which, xshape, train=True, infer_tile=2):
        """Winograd-domain kernel of layer `op` for an input of shape xshape (in training the shape picks the tile size; inference
        takes `infer_tile`, whatever the batch: F(2x2, 3x3) for the trunk -- the RPN scores feed index-exact proposal selection --,
        the uniform F(4x4, 3x3) tiling for the mask head, whose output is thresholded at 0.5): which = 0 forward, 1 data gradient."""
        key = (op.name, ops.winograd_tile(tuple(xshape)) if train else infer_tile, which)
        self._wino_reads.add(key)
        return self._wino_fresh(key)

    def _wino_fresh(self, key):
        """The U of `key`, rebuilt in place when stale: from op.w (forward) or from the flipped / transposed op.wt."""
        ent = self._wino.setdefault(key, [None, None])
        if ent[1] != self._gen:
            name, tile, which = key
            op = self.op(name)
            assert which == 0 or self._wt_gen == self._gen
            ent[0] = ops.winograd_weights(op.w if which == 0 else op.wt, out=ent[0], tile=tile)
            ent[1] = self._gen
        return ent[0]

    def _wino_ok(self, op, xshape, min_rows=None):
        return (self.winograd and self.head_dtype is None and
                ops.winograd_ok(tuple(xshape), op.wshape, op.stride, op.padding, min_rows))

    def _wino_trunk_ok(self, op, xshape):
        """Trunk layers (FPN smoothing, RPN shared convolution) take the F(2x2, 3x3) path from 4 096 pixels on (P3 at 256 x 256
        x 4 images, P2 at batch-1 detect): measured product default 20.22 -> 20.03 ms, detect 3.14 -> 3.10 ms, ResNet-50 step
        19.67 -> 19.50 ms, headline level; the mask head keeps its own threshold (ops._WINO_MIN_ROWS)."""
        return self.trunk_winograd and self._wino_ok(op, xshape, self.trunk_winograd_min_rows)

    def _ensure_h16(self):
        """16-bit operand images (W^T and the rotated data-gradient image) of the mask-head convolutions."""
        if self._h16_gen == (self._gen, self.head_dtype):
            return
        # one set of images per dtype, allocated once and refreshed IN PLACE: captured HIP graphs (infer_graphed) hold
        # their addresses, so a weight update must never move them
        imgs = self._h16_store.setdefault(self.head_dtype, {})
        names = ["mrcnn_mask_conv%d" % i for i in range(1, 5)] + ["mrcnn_mask_deconv"]   # deconv: GEMM matrix [Cin, 4*Cd]
        if self.h16_wide:
            names += [n for n in H16_WIDE_LAYERS if self._h16_shape_ok(self.op(n))]
            for stage in self.stages:
                for blk in stage:
                    if self._h16_block(blk):
                        names += [blk.c2a.name, blk.c2b.name, blk.c2c.name] + ([blk.c1.name] if blk.c1 is not None else [])
        # steady state: every image exists (addresses stable) -> ONE table-driven launch refreshes them all; only the
        # class-head FC layers' second image (a plain cast of the HWIO kernel) keeps its own launch
        tkey = (self.head_dtype, tuple(names))
        tab = self._h16_tables.get(tkey)
        if tab is not None:
            ops.weights_to_h16_batched(self.params, tab[0], self.head_dtype)
            for op, wn in tab[1]:
                kh, kw, cin, cout = op.wshape
                ops.cast_to_h16(op.w.view(kh * kw * cin, cout), self.head_dtype, out=wn)
            self._h16, self._h16_gen = imgs, (self._gen, self.head_dtype)
            return
        for name in names:
            op = self.op(name)
            if op.padding == "valid" and op.wshape[0] > 1:
                # "FC as VALID conv" (mrcnn_class_conv1): forward image W^T as usual; its data gradient is the GEMM
                # dx[M, K] = dz[M, Cout] . W^T, whose operand image [K][Cout] is the HWIO kernel itself, in 16 bits
                kh, kw, cin, cout = op.wshape
                old = imgs.get(name)
                wf, _ = ops.weights_to_h16(op.w, self.head_dtype, want_dgrad=False, out=None if old is None else (old[0], None))
                wn = old[1] if old is not None else torch.empty((kh * kw * cin, cout), dtype=self.head_dtype, device=self.dev)
                ops.cast_to_h16(op.w.view(kh * kw * cin, cout), self.head_dtype, out=wn)   # never from the step arena
                imgs[name] = (wf, wn)
            else:
                imgs[name] = ops.weights_to_h16(op.w, self.head_dtype, out=imgs.get(name))
        entries, casts = [], []
        for name in names:
            op = self.op(name)
            if op.padding == "valid" and op.wshape[0] > 1:
                entries.append((op.w, imgs[name][0], None))
                casts.append((op, imgs[name][1]))
            else:
                entries.append((op.w, imgs[name][0], imgs[name][1]))
        try:
            self._h16_tables[tkey] = (ops.h16_image_table(self.params, entries, self.dev), casts)
        except AssertionError:
            pass                                            # a kernel that is not a view into the flat buffer: stay layer by layer
        self._h16, self._h16_gen = imgs, (self._gen, self.head_dtype)

    @staticmethod
    def _h16_shape_ok(op):
        """Shapes ALL 16-bit kernels take: forward Cin % 32 == 0, Cout % 128 == 0; weight gradient Cin % 256 == 0."""
        kh, kw, cin, cout = op.wshape
        return op.stride == 1 and cin % 256 == 0 and cout % 128 == 0 and kh * kw <= 64

    @staticmethod
    def _h16_fwd_ok(op):
        """Shapes the small-tile forward / data-gradient kernel takes (both directions: Cin and Cout multiples of 64)."""
        kh, kw, cin, cout = op.wshape
        return cin % 64 == 0 and cout % 64 == 0 and kh * kw <= 64 and (op.stride == 1 or (kh == 1 and kw == 1))

    def _h16_layer(self, name):
        """True when layer `name` runs on the 16-bit matrix cores in the current mode."""
        return self.head_dtype is not None and self.h16_wide and name in H16_WIDE_LAYERS and self._h16_shape_ok(self.op(name))

    def _h16_fwd(self, op, x16, act, train, res=None):
        """conv + bias + frozen BN (+ 16-bit residual) + activation of layer `op` on a 16-bit input: 16-bit result; ctx for
        _h16_bwd."""
        d = ops.conv_desc(tuple(x16.shape), op.wshape, op.stride, op.padding, act)
        z = ops.empty((d.N, d.OH, d.OW, d.Cout), x16.dtype, x16.device) if (train and op.bn) else None
        y = ops.conv2d_h16(x16, self._h16[op.name][0], op.wshape, op.b, op.scale, op.shift, op.stride, op.padding, act, z_out=z,
                           res=res)
        return y, (Ctx(x16, z, y, act, H16) if train else None)

    def _h16_bwd(self, op, d16, ctx, S, accumulate_w=False, need_dx=True, want_dy=False, dx_res=None):
        """Backward of _h16_fwd.  d16: gradient w.r.t. the activated output, 16 bit, times the loss scale S.  Bias / BN
        sums and the weight gradient land unscaled in the float32 gradient buffer; returns dx (16 bit, times S; plus
        dx_res when given), or (dx, dy) with want_dy: dy = d16 * act' is what a shortcut into this layer's Add receives."""
        got = ops.epilogue_bwd_h16(d16, ctx.out if ctx.act != ACT_NONE else None, ctx.z, op.scale, op.mean, op.rstd, op.dgamma,
                                   op.dbeta, op.db, ctx.act, 1.0 / S, want_dy=want_dy)
        dz, dy = got if want_dy else (got, None)
        self._h16_wgrad(op, ctx.x, dz, S, accumulate_w)
        if not need_dx:
            return (dz, dy) if want_dy else dz                    # the caller issues the data gradient itself
        dx = self._h16_dgrad(op, dz, dx_res)
        return (dx, dy) if want_dy else dx

    def _h16_dgrad(self, op, dz, dx_res=None, out=None, out_strides=None):
        kh, kw, cin, cout = op.wshape
        if op.padding == "valid" and kh > 1:                     # FC as VALID conv: one GEMM over the flattened window
            M = dz.shape[0]
            dx = ops.conv2d_h16(dz.view(M, 1, 1, cout), self._h16[op.name][1], (1, 1, cout, kh * kw * cin), None, None, None, 1,
                                "valid", ACT_NONE)
            return dx.view(M, kh, kw, cin)
        return ops.conv2d_h16(dz, self._h16[op.name][1], (kh, kw, cout, cin), None, None, None, 1, op.dgrad_padding, ACT_NONE,
                              res=dx_res, out=out, out_strides=out_strides)

    # ---- identity bottleneck blocks in 16 bits (configs[4], stage 4) ------------------------------------------
    def _h16_block(self, blk):
        """A bottleneck block (mrcnn/model.py:99-172) that runs in 16 bits: every block whose convolutions fit the small-tile
        kernel (channel counts multiples of 64: all of ResNet-50 / 101's 16 / 33 blocks) -- identity blocks and the first
        block of each stage (projection shortcut, stride 2 on the 1x1 convolutions)."""
        ops_ = [blk.c2a, blk.c2b, blk.c2c] + ([blk.c1] if blk.c1 is not None else [])
        return (self.head_dtype is not None and self.h16_wide and self.h16_blocks and
                all(self._h16_fwd_ok(o) for o in ops_) and (self.h16_all_blocks or
                                                             (blk.c1 is None and all(self._h16_shape_ok(o) for o in ops_))))

    def _block_fwd_h16(self, blk, x16, train):
        a, ca = self._h16_fwd(blk.c2a, x16, ACT_RELU, train)
        b, cb = self._h16_fwd(blk.c2b, a, ACT_RELU, train)
        sc, c1c = (x16, None) if blk.c1 is None else self._h16_fwd(blk.c1, x16, ACT_NONE, train)
        y, cc = self._h16_fwd(blk.c2c, b, ACT_RELU, train, res=sc)
        return y, BlockCtx(ca, cb, cc, c1c, True)

    def _h16_wgrad(self, op, x16, dz, S, accumulate=False):
        """Weight gradient of a 16-bit layer from its input and dz (16 bit, times S), on the weight-gradient stream.  A layer
        whose channel counts are below the 16-bit weight-gradient kernel's 256-channel tile (res2 / res3, the first block of a
        stage) has both operands widened to float32 ON THAT STREAM and takes the float32 kernel there -- off the critical
        path, which stays in 16 bits."""
        if self._h16_shape_ok(op):
            launch = partial(ops.conv2d_wgrad_h16, x16, dz, op.wshape, 1, op.padding, dw=op.dw, accumulate=accumulate,
                             multiplier=1.0 / S)
        else:
            def launch():
                ops.conv2d_wgrad(ops.cast_from_h16(x16), ops.cast_from_h16(dz, 1.0 / S), op.wshape, op.stride, op.padding,
                                 dw=op.dw, accumulate=accumulate)
        self._fork(self.wgrad_stream, launch, x16, dz)

    def _h16_dgrad_ep(self, op, dz, below, below_ctx, S):
        """dz of layer `below` from the dz of layer `op` above it: the 16-bit data gradient with `below`'s epilogue
        backward in its own epilogue (mrcnn_conv2d_dgrad_ep_h16); the two launches when the shape has no fused kernel."""
        kh, kw, cin, cout = op.wshape
        z, y, act = below_ctx.z, below_ctx.out, below_ctx.act
        if self.h16_fused_bwd and op.stride == 1:
            got = ops.conv2d_dgrad_ep_h16(dz, self._h16[op.name][1], (kh, kw, cout, cin), op.dgrad_padding, y if act != ACT_NONE else None, z,
                                          below.scale, below.mean, below.rstd, below.dgamma, below.dbeta, below.db, act, 1.0 / S)
            if got is not None:
                return got
        d = self._h16_dgrad(op, dz)
        return ops.epilogue_bwd_h16(d, y if act != ACT_NONE else None, z, below.scale, below.mean, below.rstd, below.dgamma,
                                    below.dbeta, below.db, act, 1.0 / S)

    def _block_bwd_h16(self, blk, d16, ctxs, S):
        """d16: gradient w.r.t. the block output (16 bit, times S) -> gradient w.r.t. the block input.  Four launches on the
        main stream for an identity block (output-stage backward, two data gradients that carry the backward epilogue of the
        layer below, the last data gradient with the shortcut's gradient on its residual port); weight gradients on the side
        stream."""
        ca, cb, cc, c1c = ctxs.a, ctxs.b, ctxs.c, ctxs.shortcut
        c2a, c2b, c2c = blk.c2a, blk.c2b, blk.c2c
        dzc, dy = ops.epilogue_bwd_h16(d16, cc.out, cc.z, c2c.scale, c2c.mean, c2c.rstd, c2c.dgamma, c2c.dbeta, c2c.db, ACT_RELU,
                                       1.0 / S, want_dy=True)
        self._h16_wgrad(c2c, cc.x, dzc, S)
        dzb = self._h16_dgrad_ep(c2c, dzc, c2b, cb, S)
        self._h16_wgrad(c2b, cb.x, dzb, S)
        dza = self._h16_dgrad_ep(c2b, dzb, c2a, ca, S)
        self._h16_wgrad(c2a, ca.x, dza, S)
        if blk.c1 is None:
            return self._h16_dgrad(c2a, dza, dx_res=dy)           # identity shortcut: dx = dgrad_2a + dy
        # projection shortcut: dx = dgrad_1(dy) + dgrad_2a(dza); with stride 2 both 1x1 data gradients scatter into the
        # even pixels of a zeroed tensor (the second adds through the residual port, same strides)
        x16 = ca.x
        N, H, W, C = x16.shape
        st = c2a.stride
        dz1 = self._h16_bwd(blk.c1, dy, c1c, S, need_dx=False)
        dx = ops.empty((N, H, W, C), x16.dtype, x16.device)
        strides = None
        if st != 1:
            ops.fill_zero(dx)
            strides = (H * W * C, st * W * C, st * C)
        self._h16_dgrad(blk.c1, dz1, out=dx, out_strides=strides)
        self._h16_dgrad(c2a, dza, dx_res=dx, out=dx, out_strides=strides)
        return dx

    def _S(self):
        return float(self.loss_scale) if self.head_dtype == torch.float16 else 1.0

    def _wino_fwd(self, op, x, act, train, infer_tile=2):
        """ConvOp.forward(x, act) of a 3 x 3 layer through the Winograd domain (tile: see _wino_U).  With winograd_wgrad the training
        context keeps the input transform V: the layer's weight gradient contracts it with the transformed dz."""
        out = ops.empty(tuple(x.shape[:3]) + (op.wshape[3],), torch.float32, x.device)
        z = ops.empty_like(out) if (train and op.bn) else None
        V = ops.winograd_v_empty(tuple(x.shape), x.device) if (train and self.winograd_wgrad) else None
        ops.conv2d_winograd(x, self._wino_U(op, 0, x.shape, train, infer_tile), op.b, op.scale, op.shift, act, out=out, z_out=z, keep_v=V)
        return out, (Ctx(x, z, out, act, WINO, V) if train else None)

    def _wino_link_ok(self, op, nxt, xshape):
        """Whether layer `op` (input shape xshape) hands its output to `nxt` in the transform domain.  Both take the Winograd path
        with the mixed tiling; the successor keeps its V (its weight gradient then needs no x) and the backward takes op's ReLU
        mask from z (the fused data-gradient epilogue of a BatchNorm layer), so nobody reads the activated output."""
        tile = ops.winograd_tile(tuple(xshape))
        oshape = tuple(xshape[:3]) + (op.wshape[3],)
        return (self.winograd_chain and self.winograd_wgrad and self.fused_dgrad_epilogue and op.bn is not None and
                ops.winograd_chain_ok(tuple(xshape), op.wshape[3], tile) and
                self._wino_ok(nxt, oshape) and ops.winograd_tile(oshape) == tile)

    def _wino_bwd_link_ok(self, ctx, below, bctx, shape, bshape):
        """Whether the data gradient of a layer (context ctx, its dz of `shape`) hands dz of the layer `below` (of bshape) on in the
        transform domain only.  Both layers ran the Winograd path with the mixed tiling, the layer below has BatchNorm and ReLU with
        a kept z (its mask comes from z) and kept its forward V (its weight gradient takes A dz A^T as it is), so dz has exactly
        two readers, both transforms of it."""
        tile = ops.winograd_tile(shape)
        return (self.winograd_bwd_chain and self.fused_dgrad_epilogue and ctx.path == WINO and bctx.path == WINO and
                below.bn is not None and bctx.act == ACT_RELU and bctx.z is not None and bctx.V is not None and
                ops.winograd_tile(bshape) == tile and ops.winograd_chain_ok(shape, bshape[3], tile))

    def _wino_chained_fwd(self, layers, x, act):
        """Training forward of consecutive 3 x 3 layers, [(x, ctx) = _wino_fwd(op, x, act, True) or op.forward(...)] with the layers
        that _wino_link_ok allows linked: a linked layer writes its successor's input transform V instead of its activated output,
        so its context has out = None and its successor's x = None (and V always)."""
        ctxs = []
        shape, V = tuple(x.shape), None             # V: the current layer's input transform where the layer below wrote it
        for i, op in enumerate(layers):
            if V is None and not self._wino_ok(op, shape):
                x, c = op.forward(x, act, train=True)
                ctxs.append(c)
                shape = tuple(x.shape)
                continue
            nxt = layers[i + 1] if i + 1 < len(layers) else None
            oshape = shape[:3] + (op.wshape[3],)
            ready = V is not None
            U = self._wino_U(op, 0, shape)
            z = ops.empty(oshape, torch.float32, self.dev) if op.bn else None
            if not ready and self.winograd_wgrad:
                V = ops.winograd_v_empty(shape, self.dev)
            if nxt is not None and self._wino_link_ok(op, nxt, shape):
                Vn = ops.winograd_v_empty(oshape, self.dev)
                out = ops.conv2d_winograd_chain(shape if ready else x, U, Vn, op.b, op.scale, op.shift, act, z_out=z, keep_v=V, v_ready=ready)
            else:
                Vn = None
                out = ops.empty(oshape, torch.float32, self.dev)
                ops.conv2d_winograd(shape if ready else x, U, op.b, op.scale, op.shift, act, out=out, z_out=z, keep_v=V, v_ready=ready)
            ctxs.append(Ctx(x, z, out, act, WINO, V))
            x, shape, V = out, oshape, Vn
        return x, ctxs

    # ---- independent small convolutions in one launch (mrcnn_conv2d_fwd_multi) ------------------------
    def _forward_multi(self, layers, xs, act=ACT_NONE, train=False):
        """[ConvOp.forward(x, act) for layer, x in zip(layers, xs)] as one launch; falls back to the loop.  With trunk_winograd the
        3 x 3 layers large enough for the Winograd path (FPN smoothing / RPN shared convolution on P2, P3 of big inputs) leave the
        group and run F(2x2, 3x3) on their own; _bwd_group takes those that kept their input transform through it again."""
        if self.trunk_winograd and any(self._wino_trunk_ok(op, x.shape) for op, x in zip(layers, xs)):
            res = [None] * len(layers)
            rest = []
            for i, (op, x) in enumerate(zip(layers, xs)):
                if self._wino_trunk_ok(op, x.shape):
                    res[i] = self._wino_fwd(op, x, act, train)
                else:
                    rest.append(i)
            if rest:
                sub = self._forward_multi([layers[i] for i in rest], [xs[i] for i in rest], act, train) if len(rest) > 1 else \
                    [layers[rest[0]].forward(xs[rest[0]], act, train=train)]
                for i, r in zip(rest, sub):
                    res[i] = r
            return res
        if self.multi_launch and 1 < len(layers) <= 5:
            probs, zs = [], []
            for op, x in zip(layers, xs):
                d = ops.conv_desc(tuple(x.shape), op.wshape, op.stride, op.padding, act)
                out = ops.empty((d.N, d.OH, d.OW, d.Cout), torch.float32, x.device)
                z = ops.empty_like(out) if (train and op.bn) else None
                zs.append(z)
                probs.append(dict(x=x, w=op.w, bias=op.b, scale=op.scale, shift=op.shift, stride=op.stride,
                                  padding=op.padding, act=act, out=out, z_out=z))
            outs = ops.conv2d_multi(probs)
            if outs is not None:
                return [(o, Ctx(x, z, o, act) if train else None) for o, x, z in zip(outs, xs, zs)]
        return [op.forward(x, act, train=train) for op, x in zip(layers, xs)]

    def _dgrad_multi(self, layers, dzs, ctxs, outs=None, accumulate=False):
        """[ConvOp.dgrad(dz, ctx, out, accumulate)] for stride-1 SAME / 1x1 layers as one launch (else the loop)."""
        outs = list(outs) if outs is not None else [None] * len(layers)
        accs = list(accumulate) if isinstance(accumulate, (list, tuple)) else [accumulate] * len(layers)
        ok = self.multi_launch and 1 < len(layers) <= 5 and all(
            op.stride == 1 and (op.padding == "same" or (op.wshape[0] == 1 and op.wshape[1] == 1)) for op in layers)
        if ok:
            probs = []
            for i, (op, dz, ctx) in enumerate(zip(layers, dzs, ctxs)):
                if outs[i] is None:
                    assert not accs[i]
                    outs[i] = ops.empty_like(ctx.x)
                probs.append(dict(x=dz, w=op.wt, padding=op.dgrad_padding, res=outs[i] if accs[i] else None,
                                  res_mode=RES_SAME if accs[i] else RES_NONE, out=outs[i]))
            if ops.conv2d_multi(probs) is not None:
                return outs
        return [op.dgrad(dz, ctx, out=o, accumulate=a) for op, dz, ctx, o, a in zip(layers, dzs, ctxs, outs, accs)]

    def _bwd_group(self, layers, dzs, ctxs, outs=None, accumulate=False, wgrad_acc=None):
        """Weight gradients (weight-gradient stream) and data gradients of a group of stride-1 convolutions from their dz.  Layers
        whose forward went through the Winograd path and kept its input transform (trunk_winograd: a context with a V) take it
        here too -- weight gradient from V, data gradient F(2x2, 3x3) and, where the destination accumulates, one add pass --,
        the others share the multi-problem launches as before.  wgrad_acc[i]: the layer's weight gradient adds to dw (shared
        weights: the RPN convolution over the pyramid levels)."""
        n = len(layers)
        outs = list(outs) if outs is not None else [None] * n
        accs = list(accumulate) if isinstance(accumulate, (list, tuple)) else [accumulate] * n
        wacc = list(wgrad_acc) if wgrad_acc is not None else [False] * n
        Vs = [c.V for c in ctxs]
        rest = [i for i in range(n) if Vs[i] is None]
        if rest and not any(wacc):                          # independent weights: the direct ones of the group share a launch as before
            self.wgrad_group([layers[i].wgrad_item(dzs[i], ctxs[i]) for i in rest])
        for i in range(n):                                  # (shared weights: in layer order, each adding to the one before)
            if Vs[i] is not None:
                self._fork(self.wgrad_stream, partial(ops.conv2d_wgrad_winograd, Vs[i], tuple(ctxs[i].x.shape), dzs[i],
                                                      layers[i].dw, accumulate=wacc[i]), Vs[i], dzs[i])
            elif any(wacc):
                self.wgrad_async(*layers[i].wgrad_item(dzs[i], ctxs[i], accumulate=wacc[i]))
        if rest:
            sub = self._dgrad_multi([layers[i] for i in rest], [dzs[i] for i in rest], [ctxs[i] for i in rest],
                                    outs=[outs[i] for i in rest], accumulate=[accs[i] for i in rest])
            for i, o in zip(rest, sub):
                outs[i] = o
        for i in range(n):
            if Vs[i] is None:
                continue
            op = layers[i]
            d = ops.conv2d_winograd(dzs[i], self._wino_U(op, 1, dzs[i].shape))
            if accs[i]:
                ops.add_inplace(outs[i], d)
            else:
                outs[i] = d
        return outs

    def join_wgrad(self):
        _hip_mod.stream_wait(torch.cuda.current_stream(self.dev), self.wgrad_stream)

    # ---- weights in / out (Keras layouts at this boundary) --------------------------------------
    def set_weights(self, weights, strict=True):
        L = self.layout
        for name, (off, n, shape) in L.offsets.items():
            if name not in weights:
                if strict:
                    raise KeyError("missing weight tensor " + name)
                continue
            a = np.asarray(weights[name], dtype=np.float32)
            if name == "mrcnn_mask_deconv/kernel" and a.shape == (2, 2, shape[3], shape[0]):
                a = deconv_keras_to_gemm(a)
            if a.size != n:
                hint = ""
                if name == "conv1/kernel":      # weights of a model with another number of input channels (RGB <-> gray)
                    hint = "; the first layer depends on the image's channels: load the rest with load_weights(..., exclude=\"conv1\") " \
                           "(run.py --exclude_first_layer_weights)"
                raise ValueError("shape mismatch for %s: %s vs %s%s" % (name, a.shape, shape, hint))
            self.params[off:off + n].copy_(torch.from_numpy(np.ascontiguousarray(a).reshape(-1)))
        for l in L.bn_layers:
            c0, c = L.bn_channel_offset[l.bn], l.shape[3]
            for key, buf in (("moving_mean", self.bn_mean), ("moving_variance", self.bn_var)):
                if l.bn + "/" + key in weights:
                    buf[c0:c0 + c].copy_(torch.from_numpy(np.asarray(weights[l.bn + "/" + key], dtype=np.float32)))
                elif strict:
                    raise KeyError("missing weight tensor %s/%s" % (l.bn, key))
        self.params_changed()

    def get_weights(self, grads=False):
        L = self.layout
        src = (self.grads if grads else self.params).detach().cpu().numpy()
        out = {}
        for name, (off, n, shape) in L.offsets.items():
            a = src[off:off + n].reshape(shape).copy()
            if name == "mrcnn_mask_deconv/kernel":
                a = deconv_gemm_to_keras(a)
            out[name] = a
        if not grads:
            mean, var = self.bn_mean.cpu().numpy(), self.bn_var.cpu().numpy()
            for l in L.bn_layers:
                c0, c = L.bn_channel_offset[l.bn], l.shape[3]
                out[l.bn + "/moving_mean"] = mean[c0:c0 + c].copy()
                out[l.bn + "/moving_variance"] = var[c0:c0 + c].copy()
        return out

    def fold_bn(self):
        L = self.layout
        if L.bn_channels:
            g = self.params[L.gamma_offset:L.gamma_offset + L.bn_channels]
            b = self.params[L.beta_offset:L.beta_offset + L.bn_channels]
            ops.bn_fold(g, b, self.bn_mean[:L.bn_channels], self.bn_var[:L.bn_channels],
                        self.bn_scale[:L.bn_channels], self.bn_shift[:L.bn_channels], self.bn_rstd[:L.bn_channels])

    def set_trainable(self, layer_regex):
        mask = self.layout.trainable_mask(layer_regex)
        self.trainable_host = mask
        coef = torch.tensor(granule_coefficients(self.layout, self.cfg.WEIGHT_DECAY, mask), dtype=torch.float32)
        # ONE buffer for the life of the engine, refreshed in place: recorded launch tapes and captured step graphs carry its
        # address in their grad_prepare / sgd_momentum calls (a second train(..., layers=...) on the same model replays them)
        if getattr(self, "gran_coef", None) is None or self.gran_coef.numel() != coef.numel():
            self.gran_coef = torch.empty(coef.numel(), dtype=torch.float32, device=self.dev)
            self._train_tapes, self._train_graphs = {}, {}
        self.gran_coef.copy_(coef)           # (the backward pass computes every gradient whatever the mask: the mask acts here only)

    def set_class_weights(self, vector):
        """Class weights of the three head losses: a float32 [NUM_CLASSES] vector of positive finite weights
        (utils.class_weight_vector), or None for the unweighted losses."""
        if vector is None:
            self.class_weights = None                # (_mode_key: recordings made with weights are not replayed without)
            return
        cw = torch.as_tensor(np.asarray(vector, dtype=np.float32))
        if tuple(cw.shape) != (self.cfg.NUM_CLASSES,):
            raise ValueError("class weights must have shape [%d] (got %s)" % (self.cfg.NUM_CLASSES, tuple(cw.shape)))
        # ONE buffer for the life of the engine, refreshed in place like gran_coef: recorded launch tapes and captured step
        # graphs carry its address in their loss call, so they survive a change of the values
        if getattr(self, "_class_weights_buf", None) is None:
            self._class_weights_buf = torch.empty(self.cfg.NUM_CLASSES, dtype=torch.float32, device=self.dev)
        self._class_weights_buf.copy_(cw)
        self.class_weights = self._class_weights_buf

    # ---- anchors -------------------------------------------------------------------------------
    def anchors(self, image_shape):
        from . import utils
        key = tuple(int(v) for v in image_shape)
        if key not in self._anchor_cache:
            a = utils.get_anchors(self.cfg, key)
            self._anchor_cache[key] = torch.tensor(a, dtype=torch.float32, device=self.dev)
        return self._anchor_cache[key]

    # =========================================================================================
    #  forward
    # =========================================================================================
    def _trunk_fwd(self, images, train):
        """resnet_graph + FPN (model.py:175-210, 2005-2026).  Returns the pyramid [P2..P6], its 16-bit twin (None unless the FPN
        smoothing ran in 16 bits), the 16-bit P2..P5 for the ROI heads' 16-bit ROIAlign (configs[4]; None: float32 gathers) and
        the tape."""
        tape = {}
        c1 = self.op("conv1")
        x, tape["conv1"] = c1.forward(images, ACT_RELU, train=train)
        if train:
            x, am = ops.maxpool3x3s2(x, want_argmax=True)
            tape["pool"] = (am, tuple(tape["conv1"].out.shape))
        else:
            x = ops.maxpool3x3s2(x)
        feats = []
        x16 = None                                  # the running activation in 16 bits (valid beside or instead of x)
        for stage in self.stages:
            for blk in stage:
                if self._h16_block(blk):
                    if x16 is None:
                        self._ensure_h16()
                        x16 = ops.cast_to_h16(x, self.head_dtype)
                    x16, ctx = self._block_fwd_h16(blk, x16, train)
                    x = None
                    if train:
                        tape[id(blk)] = ctx
                    continue
                if x is None:
                    x = ops.cast_from_h16(x16)
                x16 = None
                a, ca = blk.c2a.forward(x, ACT_RELU, train=train)
                b, cb = blk.c2b.forward(a, ACT_RELU, train=train)
                if blk.c1 is not None:
                    sc, c1c = blk.c1.forward(x, ACT_NONE, train=train)
                else:
                    sc, c1c = x, None
                x, cc = blk.c2c.forward(b, ACT_RELU, res=sc, res_mode=RES_SAME, train=train)
                if train:
                    tape[id(blk)] = BlockCtx(ca, cb, cc, c1c, False)
            if x is None:                           # stage output in float32 for the FPN lateral (x16 stays valid for the next block)
                x = ops.cast_from_h16(x16)
            feats.append(x)
        C2, C3, C4, C5 = feats
        P5s, tape["fpn_c5p5"] = self.op("fpn_c5p5").forward(C5, train=train)
        P4s, tape["fpn_c4p4"] = self.op("fpn_c4p4").forward(C4, res=P5s, res_mode=RES_UP2, train=train)
        P3s, tape["fpn_c3p3"] = self.op("fpn_c3p3").forward(C3, res=P4s, res_mode=RES_UP2, train=train)
        P2s, tape["fpn_c2p2"] = self.op("fpn_c2p2").forward(C2, res=P3s, res_mode=RES_UP2, train=train)
        names = ("fpn_p2", "fpn_p3", "fpn_p4", "fpn_p5")
        if all(self._h16_layer(n) for n in names):
            self._ensure_h16()
            outs, p16 = [], []
            for n, x in zip(names, (P2s, P3s, P4s, P5s)):
                y16, tape[n] = self._h16_fwd(self.op(n), ops.cast_to_h16(x, self.head_dtype), ACT_NONE, train)
                p16.append(y16)
                outs.append(ops.cast_from_h16(y16))             # float32 copies for ROIAlign and P6
            P2, P3, P4, P5 = outs
            P6 = ops.subsample2(P5)
            p16h = p16 if self.h16_roialign and all(t.shape[3] % 4 == 0 for t in p16) else None
            return [P2, P3, P4, P5, P6], p16 + [ops.cast_to_h16(P6, self.head_dtype)], p16h, tape
        res = self._forward_multi([self.op(n) for n in names], [P2s, P3s, P4s, P5s], train=train)
        (P2, P3, P4, P5) = [r[0] for r in res]
        for n, r in zip(names, res):
            tape[n] = r[1]
        P6 = ops.subsample2(P5)
        return [P2, P3, P4, P5, P6], None, None, tape

    def _rpn_fwd(self, pyramid, p16, train):
        """rpn_graph over the 5 levels with shared weights, outputs concatenated level-major
        (model.py:916-957, 2040-2055).  p16: the pyramid in 16 bits where _trunk_fwd has it, else None."""
        B = pyramid[0].shape[0]
        na = len(self.cfg.RPN_ANCHOR_RATIOS)
        A = sum(p.shape[1] * p.shape[2] * na for p in pyramid)
        logits = ops.empty((B, A, 2), torch.float32, self.dev)
        bbox = ops.empty((B, A, 4), torch.float32, self.dev)
        shared, cls, box = self.op("rpn_conv_shared"), self.op("rpn_class_raw"), self.op("rpn_bbox_pred")
        tape, off = [], 0
        if self.multi_launch and len(pyramid) <= 5:
            # the levels are independent and P3..P6 are a handful of workgroups each: one launch per layer for all levels
            if self._h16_layer("rpn_conv_shared"):
                self._ensure_h16()
                s16, cs_ = zip(*[self._h16_fwd(shared, x16, ACT_RELU, train)
                                 for x16 in (p16 if p16 is not None else [ops.cast_to_h16(p, self.head_dtype) for p in pyramid])])
                ss = [ops.cast_from_h16(y) for y in s16]            # the two small heads (6 / 12 columns) stay float32
            elif self.trunk_winograd and any(self._wino_trunk_ok(shared, p.shape) for p in pyramid):
                ss, cs_ = zip(*self._forward_multi([shared] * len(pyramid), pyramid, ACT_RELU, train))
            else:
                ss = ops.conv2d_multi([dict(x=p, w=shared.w, bias=shared.b, act=ACT_RELU) for p in pyramid])
                assert ss is not None                   # one weight tensor: the levels always share a launch shape
                cs_ = [Ctx(p, None, s, ACT_RELU) if train else None for p, s in zip(pyramid, ss)]
            offs = []
            for p in pyramid:
                offs.append(off)
                off += p.shape[1] * p.shape[2] * na
            ops.conv2d_multi([dict(x=s, w=cls.w, bias=cls.b, padding="valid", out_ptr=logits.data_ptr() + o * 2 * 4,
                                   out_strides=(A * 2, s.shape[2] * 2 * na, 2 * na)) for s, o in zip(ss, offs)])
            ops.conv2d_multi([dict(x=s, w=box.w, bias=box.b, padding="valid", out_ptr=bbox.data_ptr() + o * 4 * 4,
                                   out_strides=(A * 4, s.shape[2] * 4 * na, 4 * na)) for s, o in zip(ss, offs)])
            for p, s, cs, o in zip(pyramid, ss, cs_, offs):
                tape.append((cs, Ctx(s, None, None, ACT_NONE), o, p.shape[1], p.shape[2]))
            return logits, ops.softmax_rows(logits), bbox, tape
        for p in pyramid:
            s, cs = shared.forward(p, ACT_RELU, train=train)
            H, W = p.shape[1], p.shape[2]
            ops.conv2d_into(s, cls.w, cls.b, logits.data_ptr() + off * 2 * 4, A * 2, W * 2 * na, 2 * na, 1, "valid")
            ops.conv2d_into(s, box.w, box.b, bbox.data_ptr() + off * 4 * 4, A * 4, W * 4 * na, 4 * na, 1, "valid")
            tape.append((cs, Ctx(s, None, None, ACT_NONE), off, H, W))
            off += H * W * na
        probs = ops.softmax_rows(logits)
        return logits, probs, bbox, tape

    def _class_head_fwd(self, rois, fms, p16h, image_area, train):
        """fpn_classifier_graph (model.py:986-1039).  fms: P2..P5; p16h: the same in 16 bits for the 16-bit ROIAlign, or None."""
        cfg = self.cfg
        B, R = rois.shape[0], rois.shape[1]
        h16 = self._h16_layer("mrcnn_class_conv1") and self._h16_layer("mrcnn_class_conv2")
        if not h16:
            p16h = None
        if p16h is not None:                       # 16-bit pyramid -> 16-bit pooled features: no float32 gather, no cast pass
            x16 = ops.roialign_h16(rois, p16h, cfg.POOL_SIZE, image_area).view(B * R, cfg.POOL_SIZE, cfg.POOL_SIZE, -1)
        else:
            pooled = ops.roialign(rois, fms, cfg.POOL_SIZE, image_area)
            x = pooled.view(B * R, cfg.POOL_SIZE, cfg.POOL_SIZE, -1)
        if h16:
            self._ensure_h16()
            if p16h is None:
                x16 = ops.cast_to_h16(x, self.head_dtype)
            h1, c1 = self._h16_fwd(self.op("mrcnn_class_conv1"), x16, ACT_RELU, train)
            h2_16, c2 = self._h16_fwd(self.op("mrcnn_class_conv2"), h1, ACT_RELU, train)
            h2 = ops.cast_from_h16(h2_16)                        # the C- / 4C-column output layers (C = NUM_CLASSES) stay float32
        else:
            h1, c1 = self.op("mrcnn_class_conv1").forward(x, ACT_RELU, train=train)
            h2, c2 = self.op("mrcnn_class_conv2").forward(h1, ACT_RELU, train=train)
        lg, c3 = self.op("mrcnn_class_logits").forward(h2, train=train)
        bb, c4 = self.op("mrcnn_bbox_fc").forward(h2, train=train)
        logits = lg.view(B, R, cfg.NUM_CLASSES)
        probs = ops.softmax_rows(logits)
        return logits, probs, bb.view(B, R, cfg.NUM_CLASSES, 4), (c1, c2, c3, c4)

    def _mask_head_fwd(self, rois, fms, p16h, image_area, train):
        """build_fpn_mask_graph (model.py:1042-1091).  fms, p16h: as for _class_head_fwd."""
        cfg = self.cfg
        B, R = rois.shape[0], rois.shape[1]
        if p16h is not None:
            x = None
            x16 = ops.roialign_h16(rois, p16h, cfg.MASK_POOL_SIZE, image_area).view(B * R, cfg.MASK_POOL_SIZE, cfg.MASK_POOL_SIZE, -1)
        else:
            pooled = ops.roialign(rois, fms, cfg.MASK_POOL_SIZE, image_area)
            x = pooled.view(B * R, cfg.MASK_POOL_SIZE, cfg.MASK_POOL_SIZE, -1)
        ctxs = []
        if self.head_dtype is None and train:
            x, ctxs = self._wino_chained_fwd([self.op("mrcnn_mask_conv%d" % i) for i in range(1, 5)], x, ACT_RELU)
        elif self.head_dtype is None:
            for i in range(1, 5):
                op = self.op("mrcnn_mask_conv%d" % i)
                if self._wino_ok(op, x.shape):
                    x, c = self._wino_fwd(op, x, ACT_RELU, train, self.infer_mask_tile)
                else:
                    x, c = op.forward(x, ACT_RELU, train=train)
                ctxs.append(c)
        else:                                   # 16-bit matrix cores; float32 again from the deconvolution on
            self._ensure_h16()
            h = x16 if p16h is not None else ops.cast_to_h16(x, self.head_dtype)
            for i in range(1, 5):
                h, c = self._h16_fwd(self.op("mrcnn_mask_conv%d" % i), h, ACT_RELU, train)
                ctxs.append(c)
            dc, mop = self.op("mrcnn_mask_deconv"), self.op("mrcnn_mask")
            Cd = dc.wshape[3] // 4
            C_ = mop.wshape[3]
            if Cd % 256 == 0 and C_ <= 16:             # deconvolution + mask 1x1 conv + sigmoid on the 16-bit tensors too
                up = ops.deconv2x2_h16(h, self._h16[dc.name][0], dc.b, Cd, ACT_RELU)
                m = ops.mask_out_fwd_h16(up, mop.w.view(mop.wshape[2], C_), mop.b)
                ctxs.append(Ctx(h, None, up, ACT_RELU, H16) if train else None)
                ctxs.append(Ctx(up, None, m, ACT_SIGMOID, H16) if train else None)
                return m.view(B, R, m.shape[1], m.shape[2], m.shape[3]), ctxs
            x = ops.cast_from_h16(h)
        dc, mop = self.op("mrcnn_mask_deconv"), self.op("mrcnn_mask")
        if self.fused_mask_out_fwd:                # the 1x1 convolution and the sigmoid in the deconvolution's epilogue; inference
            up, m = ops.deconv2x2_mask(x, dc.w.view(dc.wshape[2], dc.wshape[3]), dc.b, mop.w.view(mop.wshape[2], mop.wshape[3]),
                                       mop.b, ACT_RELU, want_up=train)             # does not store `up`
            cm = Ctx(up, None, m, ACT_SIGMOID) if train else None
        else:
            up = ops.deconv2x2(x, dc.w.view(dc.wshape[2], dc.wshape[3]), dc.b, ACT_RELU)
            m, cm = mop.forward(up, ACT_SIGMOID, train=train)
        ctxs.append(Ctx(x, None, up, ACT_RELU) if train else None)
        ctxs.append(cm)
        return m.view(B, R, m.shape[1], m.shape[2], m.shape[3]), ctxs

    def infer(self, images, windows_norm):
        """Inference graph (model.py:2133-2159).  images [B,H,W,3] float32 device tensor (molded);
        windows_norm [B,4] device.  Returns the 7 outputs of the Keras inference model."""
        cfg = self.cfg
        B, H, W = images.shape[0], images.shape[1], images.shape[2]
        area = float(H * W)
        # layers of a few hundred pixels (res4 / res5 / P5 / P6 at batch 1) take the 16 x 16-tile single-launch kernel while the
        # inference trunk is issued: detect graph 3.01 -> 2.73 ms (ResNet-101), 2.35 -> 2.23 (ResNet-50).  Training keeps its kernels.
        with _tuning("sk16", 1 if self.sk16_infer else 0, 0):
            pyr, p16, p16h, _ = self._trunk_fwd(images, False)
            _, rpn_probs, rpn_bbox, _ = self._rpn_fwd(pyr, p16, False)
        anchors = self.anchors((H, W, images.shape[3]))
        rois = ops.proposals(rpn_probs, rpn_bbox, anchors, cfg.PRE_NMS_LIMIT, cfg.POST_NMS_ROIS_INFERENCE,
                             cfg.RPN_NMS_THRESHOLD, np.asarray(cfg.RPN_BBOX_STD_DEV, np.float32))
        _, probs, bbox, _ = self._class_head_fwd(rois, pyr[:4], p16h, area, False)
        det = ops.detections(rois, probs, bbox, windows_norm, cfg.DETECTION_MAX_INSTANCES,
                             cfg.DETECTION_MIN_CONFIDENCE, cfg.DETECTION_NMS_THRESHOLD,
                             np.asarray(cfg.BBOX_STD_DEV, np.float32))
        det_boxes = ops.empty((B, cfg.DETECTION_MAX_INSTANCES, 4), torch.float32, self.dev)
        ops.copy2d(det_boxes.data_ptr(), 16, det.data_ptr(), 24, 16, B * cfg.DETECTION_MAX_INSTANCES)
        masks, _ = self._mask_head_fwd(det_boxes, pyr[:4], p16h, area, False)
        return {"detections": det, "mrcnn_class": probs, "mrcnn_bbox": bbox, "mrcnn_mask": masks, "rpn_rois": rois,
                "rpn_class": rpn_probs, "rpn_bbox": rpn_bbox, "pyramid": pyr}

    def infer_graphed(self, images, windows_norm):
        """infer() replayed from a HIP graph (one capture per input shape and mode): the ~450 launches of a
        batch-1 detect pass are host-bound when issued one by one.  `images` / `windows_norm` may be host
        or device tensors; they are copied into the graph's static input buffers."""
        cfg = self.cfg              # the key: what the capture bakes in besides its buffers (cfg is mutable: patched in place)
        key = (tuple(images.shape), tuple(windows_norm.shape), id(cfg), _INFER_SWITCHES(self), _INFER_CFG(cfg),
               np.asarray(cfg.RPN_BBOX_STD_DEV, np.float32).tobytes(), np.asarray(cfg.BBOX_STD_DEV, np.float32).tobytes())
        entry = self._infer_graphs.get(key)
        if self.head_dtype is not None:
            self._ensure_h16()      # outside the graph: the 16-bit weight images follow set_weights / apply_gradients in place
        if entry is None:
            sx = ops.empty(tuple(images.shape), torch.float32, self.dev)
            sw = ops.empty(tuple(windows_norm.shape), torch.float32, self.dev)
            sx.copy_(images)
            sw.copy_(windows_norm)
            def settle():
                for _ in range(2):                      # sizes every workspace / caches the anchors
                    self.infer(sx, sw)
            self._settle(settle)
            graph = torch.cuda.CUDAGraph()
            self._wino_reads.clear()
            with _capture(graph):
                out = self.infer(sx, sw)
            entry = (graph, sx, sw, out, tuple(self._wino_reads))
            self._infer_graphs[key] = entry
        graph, sx, sw, out, wino_keys = entry
        for k in wino_keys:         # and so do the Winograd-domain kernels the capture reads
            self._wino_fresh(k)
        sx.copy_(images, non_blocking=True)
        sw.copy_(windows_norm, non_blocking=True)
        graph.replay()
        return out

    # =========================================================================================
    #  training step: forward + backward (gradients left in self.grads)
    # =========================================================================================
    def loss_weights(self):
        cfg = self.cfg
        return [float(cfg.LOSS_WEIGHTS.get(n, 1.)) if cfg.USE_LOSSES.get(n, True) else 0.0 for n in LOSS_NAMES]

    def forward_backward(self, *args, **kwargs):
        """forward_backward_impl with the step arena active: every tensor the step allocates is the one the
        previous step used at the same point (ops.StepArena).  Tensors of `self.last` (keep_outputs) are
        therefore valid until the next step."""
        ops.set_arena(self.arena)
        self.arena.begin()
        try:
            return self._forward_backward(*args, **kwargs)
        finally:
            self.arena.end()

    def _forward_backward(self, images, rpn_match, rpn_bbox_t, gt_class_ids, gt_boxes_norm, gt_masks, active_class_ids,
                          rand_keys, keep_outputs=False):
        """One training forward/backward on this rank's batch.  All arguments are device tensors:
        images [B,H,W,3] f32, rpn_match [B,A,1] i32, rpn_bbox_t [B,Np,4] f32, gt_class_ids [B,G] i32,
        gt_boxes_norm [B,G,4] f32 (norm_boxes_graph applied), gt_masks [B,H,W,G] u8,
        active_class_ids [C] i32 (row 0 of the batch, model.py:1182), rand_keys [B,R] f32.
        Returns losses[5] (device)."""
        cfg = self.cfg
        B, H, W = images.shape[0], images.shape[1], images.shape[2]
        area = float(H * W)
        # gradient zeroing and the flipped / transposed weight images are only needed by the backward pass: they run on
        # the weight-gradient stream beside the forward pass (0.2 ms off the critical path)
        main, aux = torch.cuda.current_stream(self.dev), self.aux_stream

        def prep():
            h16_ev = None
            if self.head_dtype is not None:
                self._ensure_h16()                     # 16-bit weight images: first needed by the FPN (wide mode) / after the trunk
                h16_ev = _hip_mod.ev_record(self.wgrad_stream)
            ops.fill_zero(self.grads)
            self.refresh_wt()
            return h16_ev
        h16_ev = self._fork(self.wgrad_stream, prep)
        prep_ev = _hip_mod.ev_record(self.wgrad_stream)
        if h16_ev is not None and self.h16_wide:
            _hip_mod.ev_wait(main, h16_ev)
        pyr, p16, p16h, tape = self._trunk_fwd(images, True)
        rpn_logits, rpn_probs, rpn_bbox, rpn_tape = self._rpn_fwd(pyr, p16, True)
        anchors = self.anchors((H, W, images.shape[3]))
        rpn_rois = ops.proposals(rpn_probs, rpn_bbox, anchors, cfg.PRE_NMS_LIMIT, cfg.POST_NMS_ROIS_TRAINING,
                                 cfg.RPN_NMS_THRESHOLD, np.asarray(cfg.RPN_BBOX_STD_DEV, np.float32))
        if self.forced_rpn_rois is not None:     # tests: compare two precisions of the differentiable part on one ROI set
            rpn_rois = self.forced_rpn_rois
        rois, tcls, tbbox, tmask, assign, counts = ops.detection_targets(
            rpn_rois, gt_class_ids, gt_boxes_norm, gt_masks, rand_keys, cfg.TRAIN_ROIS_PER_IMAGE,
            cfg.ROI_POSITIVE_RATIO, cfg.BBOX_STD_DEV, cfg.MASK_SHAPE, cfg.USE_MINI_MASK)
        # the two heads are independent: the (small) class/box head runs on the auxiliary stream beside the
        # mask head, forward and backward
        # The mask loss only sees positive ROIs (mrcnn_mask_loss_graph, model.py:1250-1257) and
        # DetectionTargetLayer puts them first (model.py:696), at most int(T * ROI_POSITIVE_RATIO) per image:
        # the mask-head outputs of every other row are never read and their gradient rows are exactly zero.
        # With ``sparse_mask_bwd`` (default) the mask head -- forward and backward -- therefore runs on rows
        # [0, quota) of each image only: same losses, same gradients, ~1/3 of the mask-head FLOPs, no host
        # synchronisation.  ``sparse_mask_bwd = False`` computes (and multiplies the zeros of) all rows like TF.
        T = rois.shape[1]
        quota = min(T, int(T * cfg.ROI_POSITIVE_RATIO))
        sparse = self.sparse_mask_bwd and 0 < quota < T
        if sparse:
            rois_m = ops.empty((B, quota, 4), torch.float32, self.dev)
            ops.copy2d(rois_m.data_ptr(), quota * 16, rois.data_ptr(), T * 16, quota * 16, B)
        else:
            rois_m = rois
        if self.head_dtype is not None:
            _hip_mod.ev_wait(main, prep_ev)                    # the mask head reads the 16-bit weight images prepared on the side stream
        logits, probs, mbbox, ctx_cls = self._fork(aux, lambda: self._class_head_fwd(rois, pyr[:4], p16h, area, True), rois)
        mmask, ctx_mask = self._mask_head_fwd(rois_m, pyr[:4], p16h, area, True)
        _hip_mod.stream_wait(main, aux)
        for t in (logits, probs, mbbox):
            t.record_stream(main)
        if sparse:                                   # rows [quota, T) of the loss input: zeros, never read as positives
            row = int(np.prod(mmask.shape[2:])) * 4
            full = ops.empty((B, T) + tuple(mmask.shape[2:]), torch.float32, self.dev)
            ops.fill_zero(full)
            ops.copy2d(full.data_ptr(), T * row, mmask.data_ptr(), quota * row, quota * row, B)
            mmask = full
        out = ops.losses_fwd_bwd(rpn_match, rpn_bbox_t, rpn_logits, rpn_bbox, tcls, tbbox, tmask, active_class_ids,
                                 logits, mbbox, mmask, self.loss_weights(),
                                 cfg.MASK_LOSS_FUNCTION == "dice_coef_loss", class_weights=self.class_weights)
        losses, d_rpn_logits, d_rpn_bbox, d_logits, d_mbbox, d_mmask = out
        _hip_mod.ev_wait(main, prep_ev)
        assert self._wt_gen == self._gen, "the backward pass reads the flipped kernels of the current weights"

        # ---- pyramid gradient accumulators ------------------------------------------------------
        dP = [ops.empty_like(p) for p in pyr[:4]]
        for t in dP:
            ops.fill_zero(t)

        def heads_bwd():
            self._class_head_bwd(d_logits, d_mbbox, ctx_cls, rois, dP, area)
            # the RPN backward needs nothing from the heads: it follows the class head on this stream, beside the
            # (much longer) mask head.  Its data gradients add to dP with plain read-modify-writes, so the mask head's
            # ROIAlign adjoint (atomics on the same maps, last thing on the main stream) waits for this event.
            return self._rpn_bwd(d_rpn_logits, d_rpn_bbox, rpn_tape, dP), _hip_mod.ev_record(aux)
        dP6, ev_aux = self._fork(aux, heads_bwd, d_logits, d_mbbox, d_rpn_logits, d_rpn_bbox)
        self._mask_head_bwd(d_mmask, ctx_mask, rois_m, dP, area, ev_aux)
        _hip_mod.stream_wait(main, aux)
        if self.grad_ready:                      # ~2/3 of the gradient bytes (FC1 alone is 51 MB) are final here,
            self.join_wgrad()
            self.grad_ready(*self.grad_ranges["heads"])     # with the whole FPN/backbone backward left to hide them
        self._trunk_bwd(dP, dP6, tape)
        if keep_outputs:
            self.last = {"rpn_class_logits": rpn_logits, "rpn_class": rpn_probs, "rpn_bbox": rpn_bbox,
                         "rpn_rois": rpn_rois, "rois": rois, "target_class_ids": tcls, "target_bbox": tbbox,
                         "target_mask": tmask, "mrcnn_class_logits": logits, "mrcnn_class": probs,
                         "mrcnn_bbox": mbbox, "mrcnn_mask": mmask, "counts": counts, "pyramid": pyr}
        return losses

    # ---- head backward --------------------------------------------------------------------------
    def _mask_head_bwd(self, d_mmask, ctxs, rois, dP, area, before_adjoint):
        """Backward of build_fpn_mask_graph on the rows the forward ran on: ``rois`` is [B, R, 4] with R = T
        (all train ROIs) or the positive quota (see forward_backward); d_mmask is always [B, T, ...].  The ROIAlign adjoint
        at its end waits for the event ``before_adjoint``."""
        B, T, R = d_mmask.shape[0], d_mmask.shape[1], rois.shape[1]
        if R == T:
            g = d_mmask
        else:
            row = int(np.prod(d_mmask.shape[2:])) * 4
            g = ops.empty((B, R) + tuple(d_mmask.shape[2:]), torch.float32, self.dev)
            ops.copy2d(g.data_ptr(), R * row, d_mmask.data_ptr(), T * row, R * row, B)
        with _tuning("h16_phase", 0, 1, on=not self.h16_phase_bwd):
            self._mask_head_bwd_rows(g.view((B * R,) + tuple(g.shape[2:])), ctxs, rois, dP, area, before_adjoint)

    def _mask_head_bwd_rows(self, g, ctxs, rois, dP, area, before_adjoint):
        cfg = self.cfg
        c1, c2, c3, c4, cdec, cm = ctxs
        mop, dc = self.op("mrcnn_mask"), self.op("mrcnn_mask_deconv")
        x_in, up = cdec.x, cdec.out
        C_ = cm.out.shape[-1]
        S = self._S()
        wgrad = lambda launch, *operands: self._fork(self.wgrad_stream, launch, *operands)
        d16 = None
        if cdec.path == H16:
            # output stage and deconvolution on the 16-bit tensors: dzg comes out scaled, in 16 bits
            dzg = ops.mask_out_bwd_h16(g, cm.out, up, mop.w.view(mop.wshape[2], mop.wshape[3]),
                                       mop.dw.view(mop.wshape[2], mop.wshape[3]), mop.db, dc.db, S)
            wgrad(partial(ops.conv2d_wgrad_h16, x_in, dzg, dc.wshape, 1, "same", dw=dc.dw, multiplier=1.0 / S), x_in, dzg)
            d16 = ops.conv2d_h16(dzg, self._h16[dc.name][1], (1, 1, dc.wshape[3], dc.wshape[2]), None, None, None, 1, "valid",
                                 ACT_NONE)
        elif self.fused_mask_out_bwd and C_ <= 16 and up.shape[-1] % 64 == 0 and up.shape[-1] <= 1024:
            # one pass over `up`: sigmoid', 1x1 conv wgrad/dgrad/bias, ReLU mask, deconv bias, GEMM regrouping
            # (dw accumulates: the flat gradient buffer was zeroed at the start of the step)
            dzg = ops.mask_out_bwd(g, cm.out, up, mop.w.view(mop.wshape[2], mop.wshape[3]),
                                   mop.dw.view(mop.wshape[2], mop.wshape[3]), mop.db, dc.db)
        else:
            dz, _ = mop.epilogue_bwd(g, cm)
            mop.wgrad(dz, cm)
            d_up = mop.dgrad(dz, cm)                                    # [M,28,28,256]
            # deconv: relu mask + bias, regroup to GEMM columns, then the two GEMM adjoints
            dzu = ops.empty_like(d_up)
            ops.epilogue_bwd(d_up, up, None, None, None, None, None, dzu, None, None, dc.db, ACT_RELU)
            dzg = ops.pixel_unshuffle2(dzu)                             # [M,14,14,1024]
        if d16 is None:
            wgrad(partial(ops.conv2d_wgrad, x_in, dzg, dc.wshape, 1, "valid", dw=dc.dw), x_in, dzg)
        chain = [(self.op("mrcnn_mask_conv%d" % i), c) for i, c in ((4, c4), (3, c3), (2, c2), (1, c1))]
        if c4.path != H16:
            # every data-gradient convolution applies the epilogue backward of the layer below in its own epilogue
            # (mrcnn_conv2d_dgrad_ep): the gradient w.r.t. the activated output is never written or re-read
            dz = self._dgrad_ep(dzg, dc.wt, "valid", chain[0][0], chain[0][1])
            # behind a linked boundary (_wino_bwd_link_ok) a layer's dz exists only as its two transforms: Vd = B^T dz B for its
            # data gradient, dM = A dz A^T for its weight gradient (written on this stream, read on the weight-gradient stream:
            # arena tensors, operands of the fork); dz is then None and `shape` stands for it
            shape, Vd, dM = tuple(dz.shape), None, None
            for k, (op, c) in enumerate(chain):
                if dM is not None:
                    wgrad(partial(ops.conv2d_wgrad_winograd, c.V, shape[:3] + (op.wshape[2],), shape, op.dw, dm_ready=dM), c.V, dM)
                elif c.V is not None:
                    wgrad(partial(ops.conv2d_wgrad_winograd, c.V, shape[:3] + (op.wshape[2],), dz, op.dw), c.V, dz)     # (c.x: None behind a linked layer)
                else:
                    wgrad(partial(ops.conv2d_wgrad, c.x, dz, op.wshape, op.stride, op.padding, dw=op.dw), c.x, dz)
                wino = c.path == WINO
                ready = Vd is not None
                src = shape if ready else dz
                assert wino or not ready
                if k + 1 < len(chain):
                    below, bctx = chain[k + 1]
                    bshape = shape[:3] + (op.wshape[2],)
                    if wino and self.fused_dgrad_epilogue and below.bn is not None:
                        Vn = dMn = None
                        if self._wino_bwd_link_ok(c, below, bctx, shape, bshape):
                            Vn, dMn = ops.winograd_v_empty(bshape, self.dev), ops.winograd_v_empty(bshape, self.dev)
                        dz = ops.conv2d_dgrad_ep_winograd(src, self._wino_U(op, 1, shape), bctx.out if bctx.act != ACT_NONE else None,
                                                          bctx.z, below.scale, below.mean, below.rstd, below.dgamma, below.dbeta,
                                                          below.db, bctx.act, fwd_shift=below.shift, next_v=Vn, next_dm=dMn,
                                                          keep_v=Vd, v_ready=ready)
                        Vd, dM = Vn, dMn
                    elif wino:
                        dz = below.epilogue_bwd(ops.conv2d_winograd(src, self._wino_U(op, 1, shape), keep_v=Vd, v_ready=ready), bctx)[0]
                        Vd = dM = None
                    else:
                        dz = self._dgrad_ep(dz, op.wt, op.dgrad_padding, below, bctx)
                    shape = bshape
                elif wino:
                    d = ops.conv2d_winograd(src, self._wino_U(op, 1, shape), keep_v=Vd, v_ready=ready)
                else:
                    d = op.dgrad(dz, c)
        else:
            if d16 is None:
                d = ops.conv2d(dzg, dc.wt, stride=1, padding="valid")
                d16 = ops.cast_to_h16(d, self.head_dtype, multiplier=S)
            for op, c in chain:
                d16 = self._h16_bwd(op, d16, c, S)
            d = None if self.h16_roialign else ops.cast_from_h16(d16, 1.0 / S)
        B, R = rois.shape[0], rois.shape[1]
        _hip_mod.ev_wait(torch.cuda.current_stream(self.dev), before_adjoint)
        if d is None:                           # the 16-bit gradient goes straight into the float32 pyramid gradients
            ops.roialign_bwd_h16(rois, d16.view(B, R, cfg.MASK_POOL_SIZE, cfg.MASK_POOL_SIZE, -1), dP, cfg.MASK_POOL_SIZE, area, 1.0 / S)
            return
        # scatter form here: the gather form measured 2 ms slower on the positive rows (14x14 samples of ~150 overlapping
        # positives: >1000 rows on the hottest pixels) and the dense head relies on the skipping of exactly-zero rows
        ops.roialign_bwd(rois, d.view(B, R, cfg.MASK_POOL_SIZE, cfg.MASK_POOL_SIZE, -1), dP, cfg.MASK_POOL_SIZE, area)

    def _dgrad_ep(self, dz, wt, padding, below, below_ctx):
        """dz of layer `below` from the dz of the layer above: data-gradient convolution with `wt` fused with
        `below`'s epilogue backward when the layer is large enough for that kernel, the two separate calls otherwise."""
        z, out, act = below_ctx.z, below_ctx.out, below_ctx.act
        if self.fused_dgrad_epilogue and below.bn is not None:
            got = ops.conv2d_dgrad_ep(dz, wt, padding, out if act != ACT_NONE else None, z, below.scale, below.mean, below.rstd,
                                      below.dgamma, below.dbeta, below.db, act)
            if got is not None:
                return got
        d = ops.conv2d(dz, wt, stride=1, padding=padding)
        return below.epilogue_bwd(d, below_ctx)[0]

    def _class_head_bwd(self, d_logits, d_mbbox, ctxs, rois, dP, area):
        cfg = self.cfg
        c1, c2, c3, c4 = ctxs
        lo, bo = self.op("mrcnn_class_logits"), self.op("mrcnn_bbox_fc")
        M = d_logits.shape[0] * d_logits.shape[1]
        g1 = d_logits.view(M, 1, 1, -1)
        g2 = d_mbbox.view(M, 1, 1, -1)
        dz, _ = lo.epilogue_bwd(g1, c3)
        lo.wgrad(dz, c3)
        d_h2 = lo.dgrad(dz, c3)
        dz, _ = bo.epilogue_bwd(g2, c4)
        bo.wgrad(dz, c4)
        bo.dgrad(dz, c4, out=d_h2, accumulate=True)
        op2, op1 = self.op("mrcnn_class_conv2"), self.op("mrcnn_class_conv1")
        if c2.path == H16:                                      # the two FC layers ran in 16 bits
            S = self._S()
            d_h1 = self._h16_bwd(op2, ops.cast_to_h16(d_h2, self.head_dtype, multiplier=S), c2, S)
            d_pool = ops.cast_from_h16(self._h16_bwd(op1, d_h1, c1, S), 1.0 / S)
        else:
            dz, _ = op2.epilogue_bwd(d_h2, c2)
            op2.wgrad(dz, c2)
            d_h1 = op2.dgrad(dz, c2)
            dz, _ = op1.epilogue_bwd(d_h1, c1)
            op1.wgrad(dz, c1)
            d_pool = op1.dgrad(dz, c1)
        B, R = rois.shape[0], rois.shape[1]
        ops.roialign_bwd(rois, d_pool.view(B, R, cfg.POOL_SIZE, cfg.POOL_SIZE, -1), dP, cfg.POOL_SIZE, area,
                         dense=self.gather_roialign_bwd)

    def _rpn_bwd(self, d_logits, d_bbox, rpn_tape, dP):
        na = len(self.cfg.RPN_ANCHOR_RATIOS)
        B, A = d_logits.shape[0], d_logits.shape[1]
        shared, cls, box = self.op("rpn_conv_shared"), self.op("rpn_class_raw"), self.op("rpn_bbox_pred")
        dP6 = None
        if self.multi_launch and len(rpn_tape) == 5:
            # level by level only what is elementwise; the data-gradient convolutions of the five levels share launches
            n = len(rpn_tape)
            dzl, dzb, heads = [], [], []
            for lvl, (cs, chead, off, H, W) in enumerate(rpn_tape):
                gl = ops.empty((B, H, W, 2 * na), torch.float32, self.dev)
                gb = ops.empty((B, H, W, 4 * na), torch.float32, self.dev)
                ops.copy2d(gl.data_ptr(), H * W * 2 * na * 4, d_logits.data_ptr() + off * 2 * 4, A * 2 * 4, H * W * 2 * na * 4, B)
                ops.copy2d(gb.data_ptr(), H * W * 4 * na * 4, d_bbox.data_ptr() + off * 4 * 4, A * 4 * 4, H * W * 4 * na * 4, B)
                dz, _ = cls.epilogue_bwd(gl, chead)
                cls.wgrad(dz, chead, accumulate=lvl > 0)             # weights shared by the 5 levels
                dzl.append(dz)
                dz, _ = box.epilogue_bwd(gb, chead)
                box.wgrad(dz, chead, accumulate=lvl > 0)
                dzb.append(dz)
                heads.append(chead)
            d_s = self._dgrad_multi([cls] * n, dzl, heads)
            self._dgrad_multi([box] * n, dzb, heads, outs=d_s, accumulate=True)
            if rpn_tape[0][0].path == H16:
                S = self._S()
                for lvl, (cs, chead, off, H, W) in enumerate(rpn_tape):
                    dx16 = self._h16_bwd(shared, ops.cast_to_h16(d_s[lvl], self.head_dtype, multiplier=S), cs, S, accumulate_w=lvl > 0)
                    if lvl < 4:
                        ops.axpy_from_h16(dx16, dP[lvl], 1.0 / S)       # P2..P5 also feed the ROI heads: add to their gradients
                    else:
                        dP6 = ops.cast_from_h16(dx16, 1.0 / S)
                return dP6
            dzs, ctxs = [], []
            wino = any(t[0].V is not None for t in rpn_tape)
            for lvl, (cs, chead, off, H, W) in enumerate(rpn_tape):
                dz, _ = shared.epilogue_bwd(d_s[lvl], cs)
                if not wino:
                    shared.wgrad(dz, cs, accumulate=lvl > 0)
                dzs.append(dz); ctxs.append(cs)
            if wino:                                        # some level's forward kept its Winograd input transform (trunk_winograd)
                return self._bwd_group([shared] * n, dzs, ctxs, outs=list(dP[:4]) + [None], accumulate=[True] * 4 + [False],
                                       wgrad_acc=[lvl > 0 for lvl in range(n)])[4]
            return self._dgrad_multi([shared] * n, dzs, ctxs, outs=list(dP[:4]) + [None], accumulate=[True] * 4 + [False])[4]
        for lvl, (cs, chead, off, H, W) in enumerate(rpn_tape):
            gl = ops.empty((B, H, W, 2 * na), torch.float32, self.dev)
            gb = ops.empty((B, H, W, 4 * na), torch.float32, self.dev)
            ops.copy2d(gl.data_ptr(), H * W * 2 * na * 4, d_logits.data_ptr() + off * 2 * 4, A * 2 * 4, H * W * 2 * na * 4, B)
            ops.copy2d(gb.data_ptr(), H * W * 4 * na * 4, d_bbox.data_ptr() + off * 4 * 4, A * 4 * 4, H * W * 4 * na * 4, B)
            acc = lvl > 0                                            # weights shared by the 5 levels
            dz, _ = cls.epilogue_bwd(gl, chead)
            cls.wgrad(dz, chead, accumulate=acc)
            d_s = cls.dgrad(dz, chead)
            dz, _ = box.epilogue_bwd(gb, chead)
            box.wgrad(dz, chead, accumulate=acc)
            box.dgrad(dz, chead, out=d_s, accumulate=True)
            dz, _ = shared.epilogue_bwd(d_s, cs)
            shared.wgrad(dz, cs, accumulate=acc)
            if lvl < 4:
                shared.dgrad(dz, cs, out=dP[lvl], accumulate=True)
            else:
                dP6 = shared.dgrad(dz, cs)
        return dP6

    # ---- FPN + backbone backward ------------------------------------------------------------------
    def _trunk_bwd(self, dP, dP6, tape):
        dP2, dP3, dP4, dP5 = dP
        ops.subsample2_bwd_acc(dP6, dP5)
        layers, dzs, cs = [], [], []
        if tape["fpn_p5"].path == H16:                              # smoothing convolutions ran in 16 bits
            S = self._S()
            d16 = [self._h16_bwd(self.op(name), ops.cast_to_h16(g, self.head_dtype, multiplier=S), tape[name], S)
                   for name, g in (("fpn_p5", dP5), ("fpn_p4", dP4), ("fpn_p3", dP3), ("fpn_p2", dP2))]
            d5s, d4s, d3s, d2s = [ops.cast_from_h16(t, 1.0 / S) for t in d16]
        else:
            for name, g in (("fpn_p5", dP5), ("fpn_p4", dP4), ("fpn_p3", dP3), ("fpn_p2", dP2)):
                op, c = self.op(name), tape[name]
                dz, _ = op.epilogue_bwd(g, c)
                layers.append(op); dzs.append(dz); cs.append(c)
            if any(c.V is not None for c in cs):
                d5s, d4s, d3s, d2s = self._bwd_group(layers, dzs, cs)
            else:
                self.wgrad_group([op.wgrad_item(dz, c) for op, dz, c in zip(layers, dzs, cs)])
                d5s, d4s, d3s, d2s = self._dgrad_multi(layers, dzs, cs)    # four independent 3x3 data gradients: one launch
        ops.upsample2_bwd(d2s, d3s, True)
        ops.upsample2_bwd(d3s, d4s, True)
        ops.upsample2_bwd(d4s, d5s, True)
        layers, dzs, cs = [], [], []
        for name, g in (("fpn_c2p2", d2s), ("fpn_c3p3", d3s), ("fpn_c4p4", d4s), ("fpn_c5p5", d5s)):
            op, c = self.op(name), tape[name]
            dz, _ = op.epilogue_bwd(g, c)
            layers.append(op); dzs.append(dz); cs.append(c)
        self.wgrad_group([op.wgrad_item(dz, c) for op, dz, c in zip(layers, dzs, cs)])
        dC = self._dgrad_multi(layers, dzs, cs)                         # and the four lateral 1x1 ones
        if self.grad_ready:
            self.join_wgrad()
            self.grad_ready(*self.grad_ranges["tail"])
        d_out = dC[3]                                   # gradient w.r.t. C5
        d16 = None                                      # the running gradient in 16 bits (times S), between 16-bit blocks
        S = self._S()
        for si in (3, 2, 1, 0):
            stage = self.stages[si]
            for bi in range(len(stage) - 1, -1, -1):
                blk = stage[bi]
                if tape[id(blk)].h16:
                    if d16 is None:
                        d16 = ops.cast_to_h16(d_out, self.head_dtype, multiplier=S)
                    d16 = self._block_bwd_h16(blk, d16, tape[id(blk)], S)
                    d_out = None
                    if bi == 0 and si > 0:          # first block of a stage: its input C_(s-1) also feeds the FPN lateral
                        d_out, d16 = ops.axpy_from_h16(d16, dC[si - 1], 1.0 / S), None
                    continue
                if d_out is None:
                    d_out, d16 = ops.cast_from_h16(d16, 1.0 / S), None
                # the first block of stage s+1 consumes C_s, whose FPN gradient is already in dC[si-1]
                acc_buf = dC[si - 1] if (bi == 0 and si > 0) else None
                # the block before this one in the forward order: its output epilogue backward (ReLU mask, BN of its 2c
                # convolution) rides on this block's last data gradient when that is a split-K layer
                below = None
                if bi > 0:
                    below = stage[bi - 1]
                elif si > 0:
                    below = self.stages[si - 1][-1]
                if below is not None:                   # (a block below that ran in 16 bits differentiates its own output stage)
                    below = None if tape[id(below)].h16 else (below, tape[id(below)].c)
                d_out = self._block_bwd(blk, d_out, tape[id(blk)], acc_buf, below)
            if self.grad_ready:
                self.join_wgrad()
                self.grad_ready(*self.grad_ranges[si + 2])
        assert not isinstance(d_out, tuple)             # the first block of the network has no block below it
        if d_out is None:
            d_out = ops.cast_from_h16(d16, 1.0 / S)
        am, pre_shape = tape["pool"]
        d_relu = ops.maxpool3x3s2_bwd(d_out, am, pre_shape)
        c1 = self.op("conv1")
        dz, _ = c1.epilogue_bwd(d_relu, tape["conv1"])
        c1.wgrad(dz, tape["conv1"])
        self.join_wgrad()
        if self.grad_ready:
            self.grad_ready(*self.grad_ranges["head"])
            self.grad_ready(*self.grad_ranges["bn"])

    def _block_bwd(self, blk, d_out, ctxs, acc_buf, below=None):
        """Backward of one bottleneck block.  ``d_out``: gradient w.r.t. the block output, or the pair (dz of the 2c
        convolution, gradient after the output ReLU) when the block after it already applied this block's output
        epilogue backward (see ``below``).  Returns the gradient w.r.t. the block input, or such a pair for ``below``."""
        ca, cb, cc, c1c = ctxs.a, ctxs.b, ctxs.c, ctxs.shortcut
        if isinstance(d_out, tuple):
            dzc, dy = d_out
        else:
            dzc, dy = blk.c2c.epilogue_bwd(d_out, cc, want_dy=True)
        # 2c -> 2b -> 2a: each data-gradient convolution (or its split-K reduction) applies the epilogue backward of
        # the layer below (mrcnn_conv2d_dgrad_ep)
        dzb = self._dgrad_ep(dzc, blk.c2c.wt, "valid", blk.c2b, cb)
        dza = self._dgrad_ep(dzb, blk.c2b.wt, (1, 1), blk.c2a, ca)
        # the block's weight gradients travel together (they trail the data gradients on their stream anyway)
        items = [blk.c2c.wgrad_item(dzc, cc), blk.c2b.wgrad_item(dzb, cb), blk.c2a.wgrad_item(dza, ca)]
        if blk.c1 is None:
            self.wgrad_group(items)
            # identity shortcut: dx = dy + dgrad_2a
            fused = self._final_dgrad_fused(blk, dza, dy, below)
            return fused if fused is not None else blk.c2a.dgrad(dza, ca, out=dy, accumulate=True)   # in place on dy
        dz1, _ = blk.c1.epilogue_bwd(dy, c1c)
        self.wgrad_group(items + [blk.c1.wgrad_item(dz1, c1c)])
        if acc_buf is not None:
            dx = blk.c1.dgrad(dz1, c1c, out=acc_buf, accumulate=True)
        else:
            dx = blk.c1.dgrad(dz1, c1c)
        fused = self._final_dgrad_fused(blk, dza, dx, below)
        return fused if fused is not None else blk.c2a.dgrad(dza, ca, out=dx, accumulate=True)

    def _final_dgrad_fused(self, blk, dza, acc, below):
        """dx = dgrad_2a(dza) + acc with the output epilogue backward of the block below fused into the split-K reduction:
        returns (dz of below's 2c convolution, masked gradient for below's shortcut), or None when that data gradient is not
        a dense stride-1 split-K layer (the caller then takes the two-launch route)."""
        if below is None or not self.fused_dgrad_epilogue or blk.c2a.stride != 1:
            return None
        pblk, pcc = below
        op = pblk.c2c
        z, out, act = pcc.z, pcc.out, pcc.act
        if op.bn is None or act != ACT_RELU:
            return None
        dy_below = ops.empty_like(acc)
        got = ops.conv2d_dgrad_ep(dza, blk.c2a.wt, "valid", out, z, op.scale, op.mean, op.rstd, op.dgamma, op.dbeta, op.db, act,
                                  res=acc, dy_out=dy_below)
        return None if got is None else (got, dy_below)

    # =========================================================================================
    #  the whole training step as one HIP graph
    # =========================================================================================
    def _mode_key(self):
        """Every engine switch a captured graph / recorded launch tape bakes in besides the tensors: a replay is only valid for the
        mode it was made in (tests and tools flip these attributes between steps of one engine)."""
        # ... and what a launch bakes in by VALUE: the loss weights and the clip norm are scalar arguments of recorded calls
        # (cfg is mutable: run.py patches it in place).  The trainable mask / weight decay live in gran_coef, a buffer with a
        # stable address that set_trainable refreshes in place, so recordings survive a change of `layers`.  The class weights
        # are such a buffer too (set_class_weights); WHETHER the loss call reads one is baked in (another C-ABI entry).
        return _TRAIN_SWITCHES(self) + (float(self.loss_scale), self.forced_rpn_rois is not None, tuple(self.loss_weights()),
                                        float(self.cfg.GRADIENT_CLIP_NORM), self.class_weights is not None)

    @contextlib.contextmanager
    def _rolled_back(self):
        """Settle passes (they size every workspace, arena slot and weight image before a capture or recording) are no training
        steps: weights, momentum and the skipped-step counter (a float16 overflow there is no skipped step) are restored."""
        keep = (self.params.clone(), self.momentum.clone(), self.skipped_steps.clone())
        yield
        for t, k in zip((self.params, self.momentum, self.skipped_steps), keep):
            t.copy_(k)
        self.params_changed()

    @staticmethod
    def _static_inputs(dev_inputs, static=None):
        """The static input buffers of a captured / recorded step, holding `dev_inputs`: new ones, or `static` with the inputs
        copied in unless they already are these buffers."""
        if static is None:
            static = [torch.empty_like(t) for t in dev_inputs]
        for s_, t in zip(static, dev_inputs):
            if s_.data_ptr() != t.data_ptr():
                s_.copy_(t, non_blocking=True)
        return static

    def step_graphed(self, dev_inputs, learning_rate, momentum):
        """forward_backward + apply_gradients (single rank) replayed from a HIP graph: one capture per input signature,
        learning rate / momentum and engine mode.  A step is ~670 launches in float32 and ~930 with the 16-bit blocks; issued
        one by one they cost 15-21 ms of host time, more than the device needs in the 16-bit modes.  The three streams of the
        step (main, weight gradients, auxiliary) fork from and re-join the capturing stream, so the graph keeps their
        concurrency.  Inputs are copied into the graph's static buffers; the returned losses tensor is the graph's static
        output (valid until the next replay).  Nothing on this path may use memset / memcpy nodes."""
        key = (tuple((tuple(t.shape), t.dtype) for t in dev_inputs), float(learning_rate), float(momentum), id(self.cfg),
               self._mode_key())
        entry = self._train_graphs.get(key)
        if entry is None:
            assert self.grad_ready is None, "graph replay is single-rank: gradient hooks cannot be captured"
            static = self._static_inputs(dev_inputs)

            def settle():
                for _ in range(2):
                    self.forward_backward(*static)
                    self.apply_gradients(learning_rate, momentum, 1)
            with self._rolled_back():                       # two eager steps on a side stream
                self._settle(settle)
            graph = torch.cuda.CUDAGraph()
            with _capture(graph):
                losses = self.forward_backward(*static)
                self.apply_gradients(learning_rate, momentum, 1)
            entry = (graph, static, losses)
            self._train_graphs[key] = entry
        graph, static, losses = entry
        self._static_inputs(dev_inputs, static)
        graph.replay()
        self.params_changed(fold=False)                     # the captured step ends with the optimiser
        return losses

    def step_taped(self, dev_inputs, learning_rate, momentum, world_size=1, reducer=None):
        """forward_backward + apply_gradients (single rank) from a recorded launch tape (_hip.tape_*): the first call per
        input signature / rates / mode runs the step through the engine while every launch -- C-ABI calls with their
        descriptors and pointers, event records / waits between the three streams -- is written down; later calls copy the
        inputs into the recording's buffers and issue the same calls again.  Same launches on the same streams in the same
        order as the eager step (so, unlike the HIP-graph replay, the same overlap), without the engine's Python per launch.
        Valid because the step arena, the workspaces and the weight images have stable addresses.
        Data parallelism (`reducer`: parallel.GradReducer, self.grad_ready = reducer.ready): the gradient hooks are part of the
        recording -- event hand-offs to the exchange stream, the mrcnn_allreduce_grad calls and the final join -- so a
        data-parallel step is re-issued like a single-rank one.  The settle pass runs WITHOUT the hooks (local, rolled
        back): every call of this function then enters exactly one set of collectives whether it records or replays, so ranks
        that record in different steps cannot desynchronise."""
        key = (tuple((tuple(t.shape), t.dtype) for t in dev_inputs), float(learning_rate), float(momentum), id(self.cfg),
               torch.cuda.current_stream(self.dev).cuda_stream, self._mode_key(), int(world_size),
               None if reducer is None else id(reducer))
        entry = self._train_tapes.get(key)
        if entry is None:
            assert (self.grad_ready is None) == (reducer is None), "gradient hooks are recorded through their GradReducer"
            static = self._static_inputs(dev_inputs)
            with self._rolled_back():                       # one eager step
                hook, self.grad_ready = self.grad_ready, None
                try:
                    self.forward_backward(*static)
                finally:
                    self.grad_ready = hook
                self.apply_gradients(learning_rate, momentum, 1)
            _hip_mod.tape_begin()
            try:
                losses = self.forward_backward(*static)
                if reducer is not None:
                    reducer.finish()
                self.apply_gradients(learning_rate, momentum, world_size)
            finally:
                tape = _hip_mod.tape_end()
            # the recorded pointers are arena slots and workspaces: hold them, so a later step of another shape or mode
            # (which replaces slots) cannot hand their memory to someone else while this tape is alive
            self._train_tapes[key] = (tape, static, losses, list(self.arena.slots), list(ops._ws_cache.values()), reducer)
            return losses                                   # the recording pass was this step
        tape, static, losses = entry[:3]
        self._static_inputs(dev_inputs, static)
        _hip_mod.tape_replay(tape)
        self.params_changed(fold=False)                     # the recorded step ends with the optimiser
        return losses

    # =========================================================================================
    #  optimiser (MaskRCNN.compile, model.py:2255-2291)
    # =========================================================================================
    def skipped_step_count(self):
        """Steps whose float16 gradients were not finite (skipped on the device).  Synchronises: call it where the host
        reads the losses anyway."""
        return int(self.skipped_steps.item())

    def adapt_loss_scale(self, floor=1.0):
        """Dynamic part of the loss scaling, done wherever the host looks (MaskRCNN.train: once per epoch): halve the scale
        once for every step skipped since the last look.  Returns the number of newly skipped steps."""
        n = self.skipped_step_count()
        new = n - self._skipped_seen
        self._skipped_seen = n
        if new > 0:
            self.loss_scale = max(float(floor), self.loss_scale / (2.0 ** min(new, 8)))
        return new

    def apply_gradients(self, learning_rate, momentum, world_size=1):
        """grads (already summed over ranks) -> /world, + L2 term, global-norm clip, SGD-momentum."""
        cfg = self.cfg
        ops.grad_prepare(self.grads, self.params, 1.0 / world_size, self.gran_coef, self.sumsq)
        # float16 mode: a gradient that overflowed under the static loss scale must not reach the weights -- the guarded form
        # skips the update on the device and counts it (skipped_step_count / adapt_loss_scale); float32 and bfloat16 keep the
        # reference's plain Keras semantics
        guard = self.skipped_steps if self.head_dtype == torch.float16 else None
        ops.sgd_momentum(self.params, self.momentum, self.grads, self.sumsq, cfg.GRADIENT_CLIP_NORM, learning_rate,
                         momentum, self.gran_coef, skipped=guard)
        self.params_changed()
