"""The HBM-bound kernels every step passes through -- csrc/elementwise.hip, csrc/optim.hip, the casts, the 16-bit epilogue
backward and the weight images at the end of csrc/conv_h16.hip, the flip / transpose at the end of csrc/conv_wgrad.hip -- against
the exact or float64 references of tests/glue_cases.py (whose header says how exact each comparison is), at the smallest shapes
that reach each path: the vector and the scalar forms, misaligned pointers, a second trip of every grid-stride loop, every block
cap.  All comparisons go through the check_* helpers of glue_cases.py; tests/test_glue_cpu.py shows that those refuse wrong
results.  Every buffer a kernel writes by address carries guard values that are asserted afterwards."""
import numpy as np
import pytest
import torch

import glue_cases as gc

pytestmark = pytest.mark.gpu

NONE, RELU, SIGMOID = gc.ACT_NONE, gc.ACT_RELU, gc.ACT_SIGMOID


def _ops():
    from caesar_mrcnn_amd import ops
    return ops


def _hip():
    from caesar_mrcnn_amd import _hip
    return _hip


def _refused(fn, *a, **k):
    with pytest.raises(_hip().HipPathError):
        fn(*a, **k)
    torch.cuda.synchronize()


def _shifted(t, dev, elems=1):
    """A copy of t on the device that starts `elems` elements into a larger allocation (a misaligned pointer)."""
    buf = torch.zeros(t.numel() + elems + 8, dtype=t.dtype, device=dev)
    v = buf[elems:elems + t.numel()].view(t.shape)
    v.copy_(t)
    return v


# ---- float32 epilogue backward ---------------------------------------------------------------------------------------------
def _epi_inputs(d, dev, put):
    return {k: (None if d[k] is None else put(d[k])) for k in ("dout", "out", "z", "scale", "mean", "rstd")}


def _epi_run(d, t, dev, want, put=None):
    """One call producing the outputs named in `want`; returns them on the CPU."""
    ops = _ops()
    C, M = d["C"], d["M"]
    mk = (lambda shape: torch.zeros(shape, device=dev)) if put is None else (lambda shape: put(torch.zeros(shape)))
    o = {k: (mk((M, C)) if k in ("dy", "dz") else mk((C,))) for k in want}
    ops.epilogue_bwd(t["dout"], t["out"], t["z"] if "dgamma" in o else None, t["scale"], t["mean"] if "dgamma" in o else None,
                     t["rstd"] if "dgamma" in o else None, dy_out=o.get("dy"), dz_out=o.get("dz"), dgamma=o.get("dgamma"),
                     dbeta=o.get("dbeta"), dbias=o.get("dbias"), act=d["act"])
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in o.items()}


@pytest.mark.parametrize("act", [NONE, RELU, SIGMOID])
@pytest.mark.parametrize("name", sorted(gc.EPI_CASES))
def test_epilogue_bwd_against_float64(dev, name, act):
    """dz / dy exact under NONE and ReLU (bounded under sigmoid), dy_out asserted in every case, the channel sums inside
    (n + k) u sum|terms|; then each output alone."""
    C, M = gc.EPI_CASES[name]
    d = gc.epi_case(C, M, act)
    ref = gc.epi_ref(d)
    t = _epi_inputs(d, dev, lambda x: x.to(dev))
    tag = "%s act %d" % (name, act)
    got = _epi_run(d, t, dev, ("dy", "dz", "dgamma", "dbeta", "dbias"))
    gc.check_epilogue(tag, ref, got)
    for alone in (("dz",), ("dy",), ("dgamma",), ("dbias",)):
        gc.check_epilogue(tag + " only " + alone[0], ref, _epi_run(d, t, dev, alone))


@pytest.mark.parametrize("act", [NONE, RELU])
def test_epilogue_bwd_misaligned_power_of_two(dev, act):
    """C = 16, M = 65 with every tensor one float into its allocation: the scalar kernel on a power-of-two C gives the aligned
    (vector) run's dz and dy bit for bit, and sums inside the same bound."""
    d = gc.epi_case(16, 65, act)
    ref = gc.epi_ref(d)
    want = ("dy", "dz", "dgamma", "dbeta", "dbias")
    aligned = _epi_run(d, _epi_inputs(d, dev, lambda x: x.to(dev)), dev, want)
    put = lambda x: _shifted(x, dev)
    shifted = _epi_run(d, _epi_inputs(d, dev, put), dev, want, put=put)
    assert gc.same_bits(shifted["dz"], aligned["dz"]) and gc.same_bits(shifted["dy"], aligned["dy"])
    gc.check_epilogue("shifted act %d" % act, ref, shifted)


@pytest.mark.parametrize("name", ["vec_c16_m65", "sca_c48_m333"])
def test_epilogue_bwd_dz_may_alias_dout(dev, name):
    ops = _ops()
    C, M = gc.EPI_CASES[name]
    d = gc.epi_case(C, M, RELU)
    ref = gc.epi_ref(d)
    t = _epi_inputs(d, dev, lambda x: x.to(dev))
    plain = _epi_run(d, t, dev, ("dz", "dbeta"))
    both = t["dout"].clone()
    dbeta = torch.zeros(C, device=dev)
    ops.epilogue_bwd(both, t["out"], None, t["scale"], dz_out=both, dbeta=dbeta, act=RELU)
    assert gc.same_bits(both, plain["dz"])
    gc.check_epilogue(name + " aliased", ref, dict(dz=both, dbeta=dbeta))


def test_epilogue_bwd_refusals(dev):
    ops = _ops()
    x = torch.zeros(2, 4097, device=dev)
    _refused(ops.epilogue_bwd, x, dz_out=torch.zeros_like(x))
    y = torch.zeros(4, 16, device=dev)
    _refused(ops.epilogue_bwd, y, dz_out=torch.zeros_like(y), act=RELU)                       # act without out
    _refused(ops.epilogue_bwd, y, dgamma=torch.zeros(16, device=dev), mean=torch.zeros(16, device=dev),
             rstd=torch.zeros(16, device=dev))                                               # dgamma without z


# ---- 16-bit epilogue backward ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", gc.H16)
@pytest.mark.parametrize("act", [NONE, RELU])
@pytest.mark.parametrize("name", sorted(gc.EPI16_CASES))
def test_epilogue_bwd_h16_against_exact(dev, name, act, dtype):
    """dz = float32(g scale) rounded once, dy = g: bit for bit.  Sums against float64, with BN sums and with dbias only,
    grad_multiplier 1 and 1/1024 (powers of two: exact), with and without dy, and dz written over dout."""
    ops, hip = _ops(), _hip()
    C, M = gc.EPI16_CASES[name]
    d = gc.epi16_case(C, M, act, dtype)
    t = {k: (None if d[k] is None else d[k].to(dev)) for k in ("dout", "out", "z", "scale", "mean", "rstd")}
    for gmul in (1.0, 1.0 / 1024):
        for want_dy in (False, True):
            tag = "%s %s act %d gmul %g" % (name, str(dtype)[6:], act, gmul)
            ref = gc.epi16_ref(d, gmul, bn=True)
            dgamma, dbeta = torch.zeros(C, device=dev), torch.zeros(C, device=dev)
            r = ops.epilogue_bwd_h16(t["dout"], t["out"], t["z"], t["scale"], t["mean"], t["rstd"], dgamma=dgamma, dbeta=dbeta, act=act,
                                     grad_multiplier=gmul, want_dy=want_dy)
            dz, dy = r if want_dy else (r, None)
            gc.check_epilogue16(tag + " bn", ref, dict(dz=dz, dy=dy, dgamma=dgamma, dbeta=dbeta))
            ref = gc.epi16_ref(d, gmul, bn=False)
            dbias = torch.zeros(C, device=dev)
            r = ops.epilogue_bwd_h16(t["dout"], t["out"], dbias=dbias, act=act, grad_multiplier=gmul, want_dy=want_dy)
            dz, dy = r if want_dy else (r, None)
            gc.check_epilogue16(tag + " bias", ref, dict(dz=dz, dy=dy, dbias=dbias))
    # dz_out aliasing dout (the wrapper always allocates dz: through the C entry)
    ref = gc.epi16_ref(d, 1.0, bn=True)
    both, dbeta = t["dout"].clone(), torch.zeros(C, device=dev)
    p = hip.ptr
    hip.check(hip.lib().mrcnn_epilogue_bwd_h16_dy(gc.H16.index(dtype), p(both), p(t["out"]), None, p(t["scale"]), None, None, p(both), None,
                                                  None, p(dbeta), None, M, C, act, 1.0, hip.current_stream()), "aliased")
    gc.check_epilogue16(name + " aliased", ref, dict(dz=both, dbeta=dbeta))


@pytest.mark.parametrize("dtype", gc.H16)
def test_epilogue_bwd_h16_refusals(dev, dtype):
    ops = _ops()
    for C in (8, 48):
        _refused(ops.epilogue_bwd_h16, torch.zeros(4, C, dtype=dtype, device=dev))
    x = torch.zeros(4, 16, dtype=dtype, device=dev)
    _refused(ops.epilogue_bwd_h16, _shifted(x.cpu(), dev))                                    # 2 bytes off
    _refused(ops.epilogue_bwd_h16, x, out=x, act=SIGMOID)
    _refused(ops.epilogue_bwd_h16, x, act=RELU)                                               # ReLU without out


# ---- max pool --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", gc.POOL_SHAPES)
def test_maxpool_ties_go_to_the_first_maximum(dev, shape):
    """ReLU-like input (mostly zeros, tied positives): out, argmax (first maximum in row-major scan, as torch's autograd) and the
    gradient (multiples of 1/8: exact) all bit for bit; both parities of H and W, an all-negative window beside the padding."""
    ops = _ops()
    c = gc.pool_case(shape)
    x = c["x"].to(dev)
    out, am = ops.maxpool3x3s2(x, want_argmax=True)
    gc.check_pool(str(shape), c, out, am)
    gc.check_pool(str(shape) + " no argmax", c, ops.maxpool3x3s2(x))
    gc.check_pool(str(shape), c, dx=ops.maxpool3x3s2_bwd(c["dout"].to(dev), am, tuple(shape)))


# ---- resampling and the small kernels --------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", gc.SUBSAMPLE_SHAPES)
def test_subsample2_odd_extents(dev, shape):
    ops = _ops()
    x = gc.eighths(shape, 11)
    gc.assert_bits("subsample2", ops.subsample2(x.to(dev)), gc.subsample_ref(x))
    dout, dx0 = gc.eighths(gc.subsample_ref(x).shape, 12), gc.eighths(shape, 13)
    dx = dx0.to(dev)
    ops.subsample2_bwd_acc(dout.to(dev), dx)
    gc.assert_bits("subsample2_bwd_acc", dx, gc.subsample_bwd_ref(dout, dx0))


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("shape", gc.UPSAMPLE_SHAPES)
def test_upsample2_bwd_both_modes(dev, shape, accumulate):
    ops = _ops()
    N, H, W, C = shape
    dout, acc = gc.eighths((N, 2 * H, 2 * W, C), 14), gc.eighths(shape, 15)
    dsrc = acc.to(dev) if accumulate else torch.full(shape, float("nan"), device=dev)
    ops.upsample2_bwd(dout.to(dev), dsrc, accumulate)
    assert not bool(torch.isnan(dsrc).any())
    gc.assert_bits("upsample2_bwd", dsrc, gc.upsample_bwd_ref(dout, acc, accumulate))


@pytest.mark.parametrize("C", gc.UNSHUFFLE_C)
def test_pixel_unshuffle2(dev, C):
    ops = _ops()
    for H in (1, 2, 3):
        for W in (1, 2, 3):
            src = torch.randn(2, 2 * H, 2 * W, C, generator=torch.Generator().manual_seed(H * 10 + W))
            out = torch.full((2, H, W, 4 * C), float("nan"), device=dev)
            ops.pixel_unshuffle2(src.to(dev), out=out)
            gc.assert_bits("unshuffle %d %d %d" % (H, W, C), out, gc.unshuffle_ref(src))
    _refused(ops.pixel_unshuffle2, torch.zeros(1, 2, 2, 6, device=dev))


def test_add_inplace_second_trip(dev):
    """n = 1, 257 and 4096 * 256 + 4099 (the grid is capped at 4096 workgroups: a second trip with a ragged end); one float32
    addition per element: exact.  The large input is built, and compared, on the device."""
    ops = _ops()
    for n in (1, 257):
        a, b = gc.eighths((n,), 16), torch.randn(n, generator=torch.Generator().manual_seed(n))
        dst = a.to(dev)
        ops.add_inplace(dst, b.to(dev))
        gc.assert_bits("add_inplace %d" % n, dst, a + b)
    n = 4096 * 256 + 4099
    i = torch.arange(n, device=dev, dtype=torch.int32)
    a, b = (i % 1021).float() / 8 - 60, (i % 509).float() * 0.37 + 1e-3
    buf = torch.full((n + 64,), 7.0, device=dev)
    buf[:n] = a
    ops.add_inplace(buf[:n], b)
    assert torch.equal(buf[:n], a + b) and bool((buf[n:] == 7.0).all())


@pytest.mark.parametrize("n", [1, 257])
def test_bn_fold(dev, n):
    ops = _ops()
    d = gc.bn_case(n)
    ref = gc.bn_ref(d, ops.BN_EPS)
    t = {k: v.to(dev) for k, v in d.items()}
    for with_rstd in (False, True):
        scale, shift = torch.full((n + 1,), 9.0, device=dev), torch.full((n + 1,), 9.0, device=dev)
        rstd = torch.full((n + 1,), 9.0, device=dev) if with_rstd else None
        ops.bn_fold(t["gamma"], t["beta"], t["mean"], t["var"], scale[:n], shift[:n], None if rstd is None else rstd[:n])
        gc.check_bn_fold("bn_fold %d" % n, d, ref, scale[:n], shift[:n], None if rstd is None else rstd[:n])
        assert float(scale[n]) == 9.0 and float(shift[n]) == 9.0 and (rstd is None or float(rstd[n]) == 9.0)


# ---- copy2d / fill_zero ----------------------------------------------------------------------------------------------------
COPIES = [  # dst_pitch, src_pitch, row_bytes, rows, dst_shift, src_shift
    (8, 12, 4, 1, 0, 0), (8, 12, 4, 37, 0, 0), (32, 48, 16, 1, 0, 0), (32, 48, 16, 37, 0, 0), (1024, 1008, 1000, 1, 0, 0),
    (1024, 1008, 1000, 37, 0, 0), (16, 16, 16, 37, 0, 0),
    (12, 10, 6, 37, 0, 0), (32, 48, 16, 37, 2, 0), (32, 48, 16, 37, 0, 2),          # the unaligned fall-back (outside any capture)
    (4096 + 64, 4096 + 32, 4096, 16385, 0, 0),                                      # 65536 * 256 + 1024 words: a second trip
]


@pytest.mark.parametrize("case", COPIES, ids=lambda c: "-".join(map(str, c)))
def test_copy2d_guards_and_pitches(dev, case):
    ops = _ops()
    dp, sp, rb, rows, ds, ss = case
    dst0, do, src, so = gc.copy2d_buffers(dp, sp, rb, rows, ds, ss, device=dev)
    dst = dst0.clone()
    assert do + (rows - 1) * dp + rb + gc.GUARD == dst.numel() and so + (rows - 1) * sp + rb + gc.GUARD == src.numel()
    ops.copy2d(dst.data_ptr() + do, dp, src.data_ptr() + so, sp, rb, rows)
    torch.cuda.synchronize()
    assert torch.equal(dst, gc.copy2d_expected(dst0, do, dp, src, so, sp, rb, rows)), "a guard, a pitch gap or a row differs"


def test_copy2d_refusals(dev):
    ops = _ops()
    b = torch.zeros(256, dtype=torch.uint8, device=dev)
    _refused(ops.copy2d, b.data_ptr(), 8, b.data_ptr() + 128, 16, 16, 2)        # dst pitch below the row
    _refused(ops.copy2d, b.data_ptr(), 16, b.data_ptr() + 128, 16, 0, 2)


@pytest.mark.parametrize("nbytes,shift", [(16, 0), (16384 * 256 * 16 + 4096, 0), (1, 0), (15, 0), (4 * 2 ** 20 + 3, 0), (32, 4)])
def test_fill_zero_guards(dev, nbytes, shift):
    """16-byte stores (16 bytes; one workgroup past the 16384-workgroup grid) and the byte kernel (1, 15, 4 MiB + 3 bytes: past
    its grid too; an aligned size at a pointer 4 bytes off)."""
    ops = _ops()
    buf0 = gc.sentinel_bytes(2 * gc.GUARD + nbytes + shift, 5, device=dev)
    buf = buf0.clone()
    ops.fill_zero(buf[gc.GUARD + shift:gc.GUARD + shift + nbytes])
    torch.cuda.synchronize()
    assert torch.equal(buf, gc.fill_expected(buf0, gc.GUARD + shift, nbytes))


# ---- optimiser -------------------------------------------------------------------------------------------------------------
def _tables(n):
    t = [gc.gran_table(n)]
    if n == 64:
        t.append(torch.tensor([-1.0]))
    return t


@pytest.mark.parametrize("n", gc.OPT_SIZES)
def test_grad_prepare_elements_norm_and_determinism(dev, n):
    """Every element of the gradient output (frozen -> 0, coef == 0 -> one product, coef > 0 -> a + b c either way), the norm
    against float64 of those outputs inside depth u, and two runs equal bit for bit.  n = 2^21 + 64 * 37 is past the
    1024-workgroup cap and leaves the final kernel more than 256 partials."""
    ops = _ops()
    depth = gc.grad_prepare_depth(n)      # 4 squares per trip x trips, 6 wave levels, 2 for the 4-way LDS add, final trips, 8 tree levels, 1 for the square
    for coef in _tables(n):
        c = gc.opt_case(n)
        runs = []
        for _ in range(2):
            g, out = c["grads"].to(dev), torch.full((1,), -1.0, device=dev)
            ops.grad_prepare(g, c["params"].to(dev), 0.37, coef.to(dev), out)
            runs.append((g.cpu(), out.cpu()))
        assert gc.same_bits(runs[0][0], runs[1][0]) and gc.same_bits(runs[0][1], runs[1][1]), "two runs differ"
        g, out = runs[0]
        gc.grad_prepare_check("grad_prepare %d" % n, g, c["grads"], c["params"], 0.37, coef)
        if bool((coef >= 0).any()):
            gc.check_norm("grad_prepare %d" % n, out[0], g, depth)
        else:
            assert float(out[0]) == 0.0
    # exactly representable products and sums: one possible result
    coef = gc.gran_table(n)
    coef[coef == gc.COEFS[2]] = gc.COEFS[1]
    c = gc.opt_case(n, exact=True)
    g, out = c["grads"].to(dev), torch.zeros(1, device=dev)
    ops.grad_prepare(g, c["params"].to(dev), 0.25, coef.to(dev), out)
    cc = coef.repeat_interleave(64).double()
    want = torch.where(cc < 0, torch.zeros(n, dtype=torch.float64), c["grads"].double() * 0.25 + cc.clamp(min=0) * c["params"].double())
    gc.assert_bits("grad_prepare exact %d" % n, g, want.float())


@pytest.mark.parametrize("n", gc.OPT_SIZES)
def test_sumsq_norm_and_determinism(dev, n):
    """sumsq against float64 inside depth u, twice bit for bit.  On inputs whose squares sum exactly in float32 (multiples of
    1/2 in [-1, 1]) sumsq, grad_prepare's norm with all coefficients 0 and scale 1, and the float64 sum are one number.  (For
    general values the two kernels need not agree to the bit: sumsq gives a thread every 256th float, grad_prepare four
    neighbours, so their partial sums round differently -- only the fixed order WITHIN each kernel is promised.)"""
    ops = _ops()
    depth = gc.sumsq_depth(n)             # per-thread trips, 6 wave levels, 2 for the 4-way LDS add, final trips, 8 tree levels, 1 for the square
    g = gc.opt_case(n)["grads"]
    outs = []
    for _ in range(2):
        out = torch.full((1,), -1.0, device=dev)
        ops.sumsq(g.to(dev), out)
        outs.append(out.cpu())
    assert gc.same_bits(outs[0], outs[1])
    gc.check_norm("sumsq %d" % n, outs[0][0], g, depth)
    halves = torch.randint(-2, 3, (n,), generator=torch.Generator().manual_seed(n % 1000)).float() / 2
    a, b = torch.zeros(1, device=dev), torch.zeros(1, device=dev)
    ops.sumsq(halves.to(dev), a)
    hg = halves.to(dev)
    ops.grad_prepare(hg, torch.ones(n, device=dev), 1.0, torch.zeros(n // 64, device=dev), b)
    assert float(a) == float(b) == float((halves.double() ** 2).sum())
    gc.assert_bits("scale 1 keeps the gradient", hg, halves)


def _sgd(ops, dev, c, coef, ss, clipnorm, lr, mom, skipped=None):
    w, v = c["params"].to(dev), c["mom"].to(dev)
    ops.sgd_momentum(w, v, c["grads"].to(dev), ss, clipnorm, lr, mom, coef.to(dev), skipped)
    return w.cpu(), v.cpu()


@pytest.mark.parametrize("n", gc.OPT_SIZES + (gc.SGD_BIG,))
def test_sgd_update_frozen_granules_and_clip(dev, n):
    """Per element inside 4 u (|m v| + |lr g clip| + |w|) of the float64 update (the clip factor as the float32 scalar both sides
    derive from the same squared norm), frozen granules untouched bit for bit; a norm below clipnorm gives the clipnorm = 0
    result bit for bit.  n = 2^23 + 320 is past sgd_kernel's 4096-workgroup cap."""
    ops = _ops()
    lr, mom = 1e-3, 0.9
    for coef in _tables(n):
        c = gc.opt_case(n)
        ss32 = np.float32(float((c["grads"].double() ** 2).sum()))
        ss = torch.tensor([float(ss32)], device=dev)
        norm = float(np.sqrt(ss32))
        w1, v1 = _sgd(ops, dev, c, coef, ss, norm / 4, lr, mom)               # above: clipped
        gc.check_sgd("sgd %d clipped" % n, c, gc.sgd_ref(c, coef, gc.clip_factor(ss32, norm / 4), lr, mom), w1, v1)
        if n == gc.SGD_BIG:
            continue
        w0, v0 = _sgd(ops, dev, c, coef, ss, 0.0, lr, mom)
        gc.check_sgd("sgd %d unclipped" % n, c, gc.sgd_ref(c, coef, 1.0, lr, mom), w0, v0)
        w2, v2 = _sgd(ops, dev, c, coef, ss, norm * 2, lr, mom)               # below
        assert gc.same_bits(w2, w0) and gc.same_bits(v2, v0), "a norm below clipnorm changed the step"
        if bool((coef >= 0).any()):
            assert not gc.same_bits(w1, w0)


def test_sgd_norm_equal_to_clipnorm(dev):
    """One non-zero gradient entry of magnitude clipnorm: sumsq is exactly clipnorm^2, the kernel's `>=` takes the clipped branch
    and clipnorm / norm is exactly 1 -- the step equals the clipnorm = 0 step bit for bit (so `>` in its place could not be told
    apart by any output; what this pins is that nothing but 1.0 comes out of the boundary)."""
    ops = _ops()
    n = 64 * 4097
    coef = gc.gran_table(n)
    c = gc.opt_case(n)
    c["grads"] = torch.zeros(n)
    at = int((coef.repeat_interleave(64) >= 0).nonzero()[777])
    c["grads"][at] = -5.0
    ss = torch.zeros(1, device=dev)
    ops.sumsq(c["grads"].to(dev), ss)
    assert float(ss) == 25.0
    w1, v1 = _sgd(ops, dev, c, coef, ss, 5.0, 1e-3, 0.9)
    w0, v0 = _sgd(ops, dev, c, coef, ss, 0.0, 1e-3, 0.9)
    assert gc.same_bits(w1, w0) and gc.same_bits(v1, v0)
    gc.check_sgd("norm == clipnorm", c, gc.sgd_ref(c, coef, 1.0, 1e-3, 0.9), w1, v1)


def test_guarded_sgd_non_finite_in_the_last_float(dev):
    ops = _ops()
    n = gc.OPT_SIZES[-1]
    coef = gc.gran_table(n, last_trainable=True)
    c = gc.opt_case(n)
    c["grads"][-1] = float("inf")
    g, ss, skipped = c["grads"].to(dev), torch.zeros(1, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    ops.grad_prepare(g, c["params"].to(dev), 1.0, coef.to(dev), ss)
    assert not bool(torch.isfinite(ss).any()), "the last float did not reach the norm"
    w, v = c["params"].to(dev), c["mom"].to(dev)
    ops.sgd_momentum(w, v, g, ss, 5.0, 1e-3, 0.9, coef.to(dev), skipped)
    assert int(skipped) == 1 and gc.same_bits(w, c["params"]) and gc.same_bits(v, c["mom"])


# ---- casts -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", gc.H16)
def test_cast_to_h16_round_to_nearest_even(dev, dtype):
    """float32(x mul) rounded once to nearest-even, bit for bit: ties between 16-bit neighbours, the float16 overflow edge
    (65519.996 -> 65504, 65520 -> inf), float16 subnormal results, signed zeros, infinities, NaN; dst aligned and one element
    off (guards around it asserted); an unaligned src refused; n = 0 launches nothing."""
    ops = _ops()
    for n in gc.CAST_LENGTHS:
        for mul in gc.CAST_MULS:
            x = gc.cast_values(dtype, n, mul)
            want = gc.cast_to_ref(x, mul, dtype)
            xd = x.to(dev)
            gc.assert_bits("cast_to %d %g" % (n, mul), ops.cast_to_h16(xd, dtype, multiplier=mul), want)
            buf = torch.full((n + 9,), gc.W_SENTINEL, dtype=dtype, device=dev)
            ops.cast_to_h16(xd, dtype, out=buf[1:1 + n], multiplier=mul)
            gc.assert_bits("cast_to %d %g shifted" % (n, mul), buf[1:1 + n], want)
            assert float(buf[0]) == gc.W_SENTINEL and bool((buf[1 + n:] == gc.W_SENTINEL).all())
    _refused(ops.cast_to_h16, _shifted(torch.zeros(16), dev), dtype)
    hip, buf = _hip(), torch.full((8,), gc.W_SENTINEL, dtype=dtype, device=dev)          # (an empty tensor has no address: through the C entry)
    assert hip.lib().mrcnn_cast_to_h16(hip.ptr(torch.ones(8, device=dev)), hip.ptr(buf), 0, gc.H16.index(dtype), 1.0, hip.current_stream()) == 0
    assert bool((buf == gc.W_SENTINEL).all())


@pytest.mark.parametrize("dtype", gc.H16)
def test_cast_from_h16_and_axpy_both_paths(dev, dtype):
    """cast_from: float32(h) * mul, one rounding, bit for bit (-0 stays -0).  axpy: dst + h mul, fused or not, bit for bit; on
    small integers with a power-of-two multiplier exactly the one possible value.  8 elements per thread when n % 8 == 0 and
    both pointers are aligned, the scalar form otherwise (n % 8 != 0; src one element off; dst one float off)."""
    ops = _ops()
    for n in gc.CAST_LENGTHS:
        h = gc.h16_values(dtype, n)
        a = torch.randn(n, generator=torch.Generator().manual_seed(n % 977))
        small = torch.randint(-64, 65, (n,), generator=torch.Generator().manual_seed(n % 971)).to(dtype)
        a8 = gc.eighths((n,), n % 1000)
        for mul in gc.CAST_MULS:
            for src_off, dst_off in ((0, 0), (1, 0), (0, 1)):
                tag = "%d %g src+%d dst+%d" % (n, mul, src_off, dst_off)
                put_s = (lambda t: _shifted(t, dev)) if src_off else (lambda t: t.to(dev))
                put_d = (lambda t: _shifted(t, dev)) if dst_off else (lambda t: t.to(dev))
                out = put_d(torch.full((n,), gc.W_SENTINEL))
                ops.cast_from_h16(put_s(h), mul, out=out)
                gc.assert_bits("cast_from " + tag, out, gc.cast_from_ref(h, mul))
                dst = put_d(a)
                ops.axpy_from_h16(put_s(h), dst, mul)
                gc.check_fma("axpy " + tag, dst, a, h, mul)
                if mul != 3.7:
                    dst = put_d(a8)
                    ops.axpy_from_h16(put_s(small), dst, mul)
                    gc.assert_bits("axpy exact " + tag, dst, (a8.double() + small.double() * mul).float())
    hip, buf = _hip(), torch.full((8,), gc.W_SENTINEL, device=dev)                       # n = 0: no launch, nothing written
    src = torch.ones(8, dtype=dtype, device=dev)
    for fn in (hip.lib().mrcnn_cast_from_h16, hip.lib().mrcnn_axpy_from_h16):
        assert fn(hip.ptr(src), hip.ptr(buf), 0, gc.H16.index(dtype), 1.0, hip.current_stream()) == 0
    assert bool((buf == gc.W_SENTINEL).all())


# ---- weight images ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", gc.W_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_weight_images_single_layer(dev, shape):
    ops = _ops()
    KH, KW, Cin, Cout = shape
    w = gc.weight_values(shape)
    wd_ = w.to(dev)
    n = w.numel()
    buf = torch.full((n + 128,), gc.W_SENTINEL, device=dev)
    ops.weight_flip_transpose(wd_, out=buf[64:64 + n].view(KH, KW, Cout, Cin))
    gc.assert_bits("flip", buf[64:64 + n].view(KH, KW, Cout, Cin), gc.flip_ref(w))
    assert bool((buf[:64] == gc.W_SENTINEL).all()) and bool((buf[64 + n:] == gc.W_SENTINEL).all())
    for dtype in gc.H16:
        for want_dgrad in (True, False):
            pool = torch.full((2 * n + 192,), gc.W_SENTINEL, dtype=dtype, device=dev)
            wf = pool[64:64 + n].view(Cout, KH * KW * Cin)
            wdg = pool[128 + n:128 + 2 * n].view(Cin, KH * KW * Cout) if want_dgrad else None
            ops.weights_to_h16(wd_, dtype, out=(wf, wdg))
            want = torch.full((2 * n + 192,), gc.W_SENTINEL, dtype=dtype)
            want[64:64 + n] = gc.h16_fwd_ref(w, dtype).reshape(-1)
            if want_dgrad:
                want[128 + n:128 + 2 * n] = gc.h16_dgrad_ref(w, dtype).reshape(-1)
            gc.assert_bits("images %s dgrad %d" % (dtype, want_dgrad), pool, want)
        a, b = ops.weights_to_h16(wd_, dtype, want_dgrad=False)
        assert b is None and gc.same_bits(a, gc.h16_fwd_ref(w, dtype))


def test_weight_flip_transpose_batched(dev):
    """All layers of one flat buffer at non-contiguous offsets in one launch: every image equals the single-layer kernel's and the
    reference, every float between the layers keeps its sentinel; then a table with a single entry."""
    ops = _ops()
    flat, offs = gc.flat_params()
    fd = flat.to(dev)
    entries = [(o,) + tuple(s) for o, s in zip(offs, gc.W_BATCH)]
    out = torch.full_like(fd, gc.W_SENTINEL)
    ops.weight_flip_transpose_batched(fd, out, ops.flip_table(entries, dev))
    gc.check_flat_flip("batched", out, flat, offs)
    for o, s in zip(offs, gc.W_BATCH):
        n = int(np.prod(s))
        assert torch.equal(out[o:o + n], ops.weight_flip_transpose(fd[o:o + n].view(s)).reshape(-1))
    out = torch.full_like(fd, gc.W_SENTINEL)
    ops.weight_flip_transpose_batched(fd, out, ops.flip_table(entries[2:3], dev))
    gc.check_flat_flip("one entry", out, flat, offs, only={2})


@pytest.mark.parametrize("dtype", gc.H16)
def test_weights_to_h16_batched(dev, dtype):
    """The 16-bit images of all layers in one launch, images inside one sentinel-filled pool; entry 4 has no data-gradient image."""
    ops = _ops()
    flat, offs = gc.flat_params()
    fd = flat.to(dev)
    sizes = [int(np.prod(s)) for s in gc.W_BATCH]
    no_dgrad = 4
    at, where = 64, []
    for i, n in enumerate(sizes):
        f = at
        at += n + 64 + 8 * i
        d = None
        if i != no_dgrad:
            d = at
            at += n + 64
        where.append((f, d))
    pool = torch.full((at,), gc.W_SENTINEL, dtype=dtype, device=dev)
    want = torch.full((at,), gc.W_SENTINEL, dtype=dtype)
    entries = []
    for (f, d), o, s, n in zip(where, offs, gc.W_BATCH, sizes):
        KH, KW, Cin, Cout = s
        w = flat[o:o + n].view(s)
        want[f:f + n] = gc.h16_fwd_ref(w, dtype).reshape(-1)
        if d is not None:
            want[d:d + n] = gc.h16_dgrad_ref(w, dtype).reshape(-1)
        entries.append((fd[o:o + n].view(s), pool[f:f + n].view(Cout, KH * KW * Cin),
                        None if d is None else pool[d:d + n].view(Cin, KH * KW * Cout)))
    ops.weights_to_h16_batched(fd, ops.h16_image_table(fd, entries, dev), dtype)
    gc.assert_bits("batched images", pool, want)
    for w, wf, wd in entries:                                   # the single-layer kernel gives the same bits
        a, b = ops.weights_to_h16(w, dtype, want_dgrad=wd is not None)
        assert torch.equal(a, wf) and (wd is None or torch.equal(b, wd))
    one = torch.full((at,), gc.W_SENTINEL, dtype=dtype, device=dev)
    (f, d), s, n = where[0], gc.W_BATCH[0], sizes[0]
    e = [(entries[0][0], one[f:f + n].view(s[3], s[0] * s[1] * s[2]), one[d:d + n].view(s[2], s[0] * s[1] * s[3]))]
    ops.weights_to_h16_batched(fd, ops.h16_image_table(fd, e, dev), dtype)
    want1 = torch.full((at,), gc.W_SENTINEL, dtype=dtype)
    want1[f:f + n], want1[d:d + n] = want[f:f + n], want[d:d + n]
    gc.assert_bits("one entry", one, want1)
