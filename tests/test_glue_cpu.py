"""tests/glue_cases.py without a GPU: the properties its cases rely on (share of zeros and of tied windows, midpoints that are
midpoints, inputs whose sums are exact in float32), its references inside their own bounds when the same statements are evaluated
in float32 on the CPU, and -- so that tests/test_glue_gpu.py is not vacuous -- every check_* helper refusing a deliberately
wrong result computed from the same inputs."""
import numpy as np
import pytest
import torch

import glue_cases as gc


def _refused(fn, *a, **k):
    with pytest.raises(AssertionError):
        fn(*a, **k)


# ---- primitives ------------------------------------------------------------------------------------------------------------
def test_same_bits_sees_signed_zero_and_matches_nan():
    a = torch.tensor([0.0, 1.0, float("nan")])
    assert gc.same_bits(a, a.clone())
    assert not gc.same_bits(a, torch.tensor([-0.0, 1.0, float("nan")]))
    assert not gc.same_bits(a, torch.tensor([0.0, 1.0, 2.0]))
    assert not gc.same_bits(a, a.double())
    assert gc.worst_ratio([0.0, 1.0], [0.0, 2.0]) == 0.5 and gc.worst_ratio([1.0], [0.0]) == float("inf")


def test_check_fma_accepts_both_roundings_only():
    g = torch.Generator().manual_seed(1)
    a, b, c = torch.randn(4096, generator=g), torch.randn(4096, generator=g), torch.randn(4096, generator=g)
    fused = (a.double() + b.double() * c.double()).float()
    split = b * c + a
    assert gc.check_fma("fused", fused, a, b, c) > 0            # the two candidates do differ somewhere
    gc.check_fma("split", split, a, b, c)
    _refused(gc.check_fma, "overwrite", b * c, a, b, c)        # an axpy that overwrites instead of adding
    off = split.clone()
    off[17] = float(np.nextafter(np.float32(max(fused[17], split[17])), np.float32(np.inf)))
    _refused(gc.check_fma, "one ulp", off, a, b, c)


def test_eighths_sum_exactly():
    e = gc.eighths((5, 100000), 3)
    assert float(e.abs().max()) == 4.0 and bool((e * 8 == torch.round(e * 8)).all())
    s32 = ((e[0] + e[1]) + (e[2] + e[3])) + e[4]
    assert torch.equal(s32.double(), e.double().sum(0))


# ---- epilogue backward -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", [gc.ACT_NONE, gc.ACT_RELU, gc.ACT_SIGMOID])
def test_epilogue_statement_is_the_float64_autograd(act):
    """The closed form of epi_ref against torch's float64 autograd of act(bn(z)), everything in float64."""
    d = gc.epi_case(48, 33, act)
    z = d["z"].double().requires_grad_()
    gamma, beta = d["gamma"].double().requires_grad_(), d["beta"].double().requires_grad_()
    y = gamma * (z - d["mean"].double()) * d["rstd"].double() + beta
    out = torch.relu(y) if act == gc.ACT_RELU else torch.sigmoid(y) if act == gc.ACT_SIGMOID else y
    out.backward(d["dout"].double())
    d64 = dict(d, out=out.detach(), dout=d["dout"].double(), z=z.detach(), scale=(gamma * d["rstd"].double()).detach(),
               mean=d["mean"].double(), rstd=d["rstd"].double())
    r = gc.epi_ref(d64)
    tol = lambda t: 1e-12 * float(t.abs().max() + 1)
    assert float((r["dz"] - z.grad).abs().max()) <= tol(z.grad)
    assert float((r["dbeta"] - beta.grad).abs().max()) <= tol(beta.grad)
    assert float((r["dgamma"] - gamma.grad).abs().max()) <= tol(gamma.grad)


@pytest.mark.parametrize("name", sorted(gc.EPI_CASES))
@pytest.mark.parametrize("act", [gc.ACT_NONE, gc.ACT_RELU, gc.ACT_SIGMOID])
def test_epilogue_float32_inside_bounds_and_mutants_refused(name, act):
    C, M = gc.EPI_CASES[name]
    d = gc.epi_case(C, M, act)
    if act == gc.ACT_RELU:
        o = d["out"].view(-1)
        assert float((o == 0).float().mean()) >= 0.125
        assert bool((torch.signbit(o) & (o == 0)).any()) or o.numel() < 4
        assert bool((gc.epi_ref(d)["dy"][d["out"] == 0] == 0).all())
    if act == gc.ACT_SIGMOID and M * C >= 2:
        assert bool((d["out"] == 0).any()) and bool((d["out"] == 1).any())
    ref, f32 = gc.epi_ref(d), gc.epi_f32(d)
    ratios = gc.check_epilogue(name, ref, f32)
    assert all(r <= 1 for r in ratios.values())
    if M > 1:                                                   # a reduction that misses its last row
        d2 = dict(d, dout=d["dout"][:-1], z=d["z"][:-1], out=None if d["out"] is None else d["out"][:-1])
        short = gc.epi_f32(d2)
        for k in ("dbeta", "dgamma", "dbias"):
            _refused(gc.check_epilogue, name, ref, {k: short[k]})
    if C >= 16:                                                 # ... its last channel group
        for k in ("dbeta", "dgamma", "dbias"):
            cut = f32[k].clone()
            cut[-4:] = 0
            _refused(gc.check_epilogue, name, ref, {k: cut})
    if act == gc.ACT_SIGMOID:                                   # dz is bounded there, not pinned
        return
    wrong = f32["dz"].clone()
    wrong.view(-1)[-1] = float(np.nextafter(np.float32(wrong.view(-1)[-1]), np.float32(np.inf)))
    _refused(gc.check_epilogue, name, ref, {"dz": wrong})


@pytest.mark.parametrize("dtype", gc.H16)
def test_epilogue16_reference_and_mutants(dtype):
    d = gc.epi16_case(128, 70, gc.ACT_RELU, dtype)
    assert 0.4 < float((d["out"] == 0).float().mean()) < 0.6
    ref = gc.epi16_ref(d, 1.0 / 1024)
    g = torch.where(d["out"].float() > 0, d["dout"].float(), torch.zeros(()))
    dz32 = g * d["scale"]
    seq = lambda t: torch.from_numpy(np.add.accumulate(t.numpy(), axis=0, dtype=np.float32)[-1].copy()) * (1.0 / 1024)
    got = dict(dz=dz32.to(dtype), dy=g.to(dtype), dbeta=seq(g), dgamma=seq(g * (d["z"].float() - d["mean"]) * d["rstd"]), dbias=seq(dz32))
    assert all(r <= 1 for r in gc.check_epilogue16("f32", ref, got).values())
    _refused(gc.check_epilogue16, "trunc", ref, {"dz": gc.toward_zero(dz32, dtype)})
    _refused(gc.check_epilogue16, "row", ref, {"dbias": seq(dz32[:-1])})
    cut = got["dbeta"].clone()
    cut[-8:] = 0
    _refused(gc.check_epilogue16, "group", ref, {"dbeta": cut})
    _refused(gc.check_epilogue16, "unscaled", ref, {"dgamma": got["dgamma"] * 1024})


# ---- max pool --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", gc.POOL_SHAPES)
def test_pool_reference_is_torch_autograd_and_mutants_refused(shape):
    c = gc.pool_case(shape)
    x = c["x"]
    N, H, W, C = shape
    (OH, pt), (OW, pl) = gc.same_pad(H), gc.same_pad(W)
    assert pt == (0 if H % 2 == 0 else 1) and pl == (0 if W % 2 == 0 else 1)      # TF SAME: (0, 1) on even, (1, 1) on odd extents
    x64 = x.double().permute(0, 3, 1, 2).contiguous().requires_grad_()
    pb, pr = (OH - 1) * 2 + 3 - H - pt, (OW - 1) * 2 + 3 - W - pl
    y = torch.nn.functional.max_pool2d(torch.nn.functional.pad(x64, (pl, pr, pt, pb), value=float("-inf")), 3, 2)
    y.backward(c["dout"].double().permute(0, 3, 1, 2))
    assert torch.equal(y.detach().permute(0, 2, 3, 1).float(), c["out"])
    assert torch.equal(x64.grad.permute(0, 2, 3, 1).float(), c["dx"]), "torch does not send the gradient to the first maximum"
    assert torch.equal(c["dx"].double().sum((1, 2)), c["dout"].double().sum((1, 2)))      # exact: multiples of 1/8
    gc.check_pool("ref", c, c["out"], c["argmax"], c["dx"])
    if H * W >= 63:
        zeros, tied = gc.pool_stats(x)
        assert zeros >= 0.5 and tied >= 0.05, (zeros, tied)
        out_l, am_l = gc.pool_ref(x, last=True)                 # the last maximum instead of the first
        assert torch.equal(out_l, c["out"])
        _refused(gc.check_pool, "last", c, argmax=am_l)
        _refused(gc.check_pool, "last", c, dx=gc.pool_bwd_ref(c["dout"], am_l, shape))
    if tuple(shape) == gc.POOL_NEG_SHAPE:                       # padding taken as 0 on the all-negative window
        assert float(c["out"][0, -1, -1, 0]) == -0.5
        out_z, _ = gc.pool_ref(x, pad_zero=True)
        assert float(out_z[0, -1, -1, 0]) == 0.0
        _refused(gc.check_pool, "pad", c, out=out_z)


# ---- resampling, small kernels ---------------------------------------------------------------------------------------------
def test_resample_references():
    for shape in gc.SUBSAMPLE_SHAPES:
        N, H, W, C = shape
        x = gc.eighths(shape, 1).double().requires_grad_()
        y = x[:, ::2, ::2, :]
        assert tuple(y.shape) == (N, (H + 1) // 2, (W + 1) // 2, C)
        dout, dx0 = gc.eighths(y.shape, 2), gc.eighths(shape, 3)
        y.backward(dout.double())
        assert torch.equal(gc.subsample_bwd_ref(dout, dx0).double(), x.grad + dx0.double())
    for shape in gc.UPSAMPLE_SHAPES:
        N, H, W, C = shape
        s = gc.eighths(shape, 4).double().requires_grad_()
        up = s.repeat_interleave(2, 1).repeat_interleave(2, 2)
        dout, acc = gc.eighths(up.shape, 5), gc.eighths(shape, 6)
        up.backward(dout.double())
        assert torch.equal(gc.upsample_bwd_ref(dout, acc, True).double(), s.grad + acc.double())     # five eighths: exact
        assert torch.equal(gc.upsample_bwd_ref(dout, acc, False).double(), s.grad)
    src = torch.arange(2 * 4 * 6 * 4, dtype=torch.float32).view(2, 4, 6, 4)
    r = gc.unshuffle_ref(src)
    for a in range(2):
        for b in range(2):
            assert torch.equal(r[..., (a * 2 + b) * 4:(a * 2 + b + 1) * 4], src[:, a::2, b::2, :])


def test_bn_fold_float32_inside_bounds():
    d = gc.bn_case(257)
    ref = gc.bn_ref(d, 1e-3)
    r = 1.0 / torch.sqrt(d["var"] + float(np.float32(1e-3)))
    s = d["gamma"] * r
    out = gc.check_bn_fold("f32", d, ref, s, d["beta"] - d["mean"] * s, r)
    assert all(v <= 1 for v in out.values())
    _refused(gc.check_bn_fold, "eps", d, ref, d["gamma"] / torch.sqrt(d["var"]), d["beta"], None)


# ---- copies ----------------------------------------------------------------------------------------------------------------
def test_copy2d_expected_and_pitch_mutant():
    dst0, do, src, so = gc.copy2d_buffers(48, 32, 16, 37)
    want = gc.copy2d_expected(dst0, do, 48, src, so, 32, 16, 37)
    assert torch.equal(want[:do], dst0[:do]) and torch.equal(want[-gc.GUARD:], dst0[-gc.GUARD:])
    for r in (0, 17, 36):
        assert torch.equal(want[do + r * 48:do + r * 48 + 16], src[so + r * 32:so + r * 32 + 16])
        if r < 36:
            assert torch.equal(want[do + r * 48 + 16:do + (r + 1) * 48], dst0[do + r * 48 + 16:do + (r + 1) * 48])   # the pitch gap
    assert bool((dst0 != 0).all())
    wrong = gc.copy2d_expected(dst0, do, 48, src, so, 32, 16, 37, ignore_dst_pitch=True)
    assert not torch.equal(wrong, want)
    z = gc.fill_expected(dst0, do + 4, 15)
    assert int((z == 0).sum()) == 15 and bool((z[do + 4:do + 19] == 0).all())


# ---- optimiser -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", gc.OPT_SIZES)
def test_granule_table(n):
    coef = gc.gran_table(n)
    ng = n // 64
    assert coef.numel() == ng
    if ng == 1:
        return
    c = coef.numpy()
    assert (c[:2] < 0).all() and (c[-2:] < 0).all()
    for k in range(16, ng - 1, 16):
        assert c[k - 1] < 0 and c[k] < 0                        # straddles every workgroup boundary
    m = c[ng // 2:ng // 2 + 40]
    assert ((m[:-1] < 0) != (m[1:] < 0)).sum() >= 30            # alternating
    adj = ((c[:-1] == 0) & (c[1:] > 0)) | ((c[:-1] > 0) & (c[1:] == 0))
    assert adj.any() and (c >= 0).mean() > 0.5
    assert gc.gran_table(n, last_trainable=True)[-1] >= 0


def test_grad_prepare_reference_exact_inputs_and_mutants():
    n = 64 * 40
    coef = gc.gran_table(n)
    coef[coef == gc.COEFS[2]] = gc.COEFS[1]                     # power-of-two coefficients only
    c = gc.opt_case(n, exact=True)
    scale = 0.25
    cc = coef.repeat_interleave(64)
    want = torch.where(cc < 0, torch.zeros(n), c["grads"] * scale + torch.where(cc > 0, cc, torch.zeros(n)) * c["params"])
    exact64 = torch.where(cc < 0, torch.zeros(n, dtype=torch.float64),
                          c["grads"].double() * scale + cc.clamp(min=0).double() * c["params"].double())
    assert torch.equal(want.double(), exact64)                  # every product and sum is exact in float32
    assert gc.grad_prepare_check("exact", want, c["grads"], c["params"], scale, coef) == 0
    thawed = c["grads"] * scale + cc.abs() * c["params"]         # a frozen granule updated
    _refused(gc.grad_prepare_check, "frozen", thawed, c["grads"], c["params"], scale, coef)
    _refused(gc.grad_prepare_check, "no decay", c["grads"] * scale * (cc >= 0), c["grads"], c["params"], scale, coef)


@pytest.mark.parametrize("n", gc.OPT_SIZES)
def test_norm_depth_and_bound(n):
    c = gc.opt_case(n)
    g = c["grads"]
    d = gc.sumsq_depth(n)
    assert d == {64: 19, 64 * 4097: 26, 2 ** 21 + 64 * 37: 30}[n]
    assert gc.grad_prepare_depth(n) == {64: 22, 64 * 4097: 26, 2 ** 21 + 64 * 37: 33}[n]
    pair = float((g * g).sum())                                 # torch's float32 pairwise sum
    assert gc.check_norm("pairwise", pair, g, d) <= 1
    tail = max(n // 1024, 1)                                    # a final pass that misses its last partial
    _refused(gc.check_norm, "short", float((g[:-tail].double() ** 2).sum()), g, d)
    halves = torch.randint(-2, 3, (n,), generator=torch.Generator().manual_seed(n % 1000)).float() / 2
    assert float((halves * halves).sum()) == float((halves.double() ** 2).sum()) < 2 ** 22      # exact in float32 in any order


def test_clip_factor_and_sgd_reference():
    n = 64 * 40
    coef = gc.gran_table(n)
    c = gc.opt_case(n)
    lr, mom = 1e-3, 0.9
    ss = np.float32(float((c["grads"].double() ** 2).sum()))
    norm = float(np.sqrt(ss))
    assert gc.clip_factor(ss, 0.0) == 1 and gc.clip_factor(ss, 2 * norm) == 1
    assert gc.clip_factor(ss, norm / 4) == np.float32(np.float32(norm / 4) / np.sqrt(ss))
    # norm == clipnorm: `>=` divides, `>` does not -- and both give exactly 1.0, so no output can tell them apart; what the
    # boundary pins is that the step equals the unclipped one bit for bit.  One float above the boundary `>=` and `>` agree again.
    assert gc.clip_factor(np.float32(25.0), 5.0) == 1 == gc.clip_factor(np.float32(25.0), 5.0, strict=True)
    clip = gc.clip_factor(ss, norm / 4)
    ref = gc.sgd_ref(c, coef, clip, lr, mom)
    w, v = gc.sgd_f32(c, coef, clip, lr, mom)
    assert max(gc.check_sgd("f32", c, ref, w, v)) <= 1
    w2, v2 = gc.sgd_f32(c, coef, clip, lr, mom, touch_frozen=True)          # a frozen granule updated
    _refused(gc.check_sgd, "frozen", c, ref, w2, v2)
    w3, v3 = gc.sgd_f32(c, coef, 1.0, lr, mom)                              # the clip not applied above the norm
    _refused(gc.check_sgd, "unclipped", c, ref, w3, v3)


# ---- casts -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", gc.H16)
def test_midpoints_are_midpoints_and_round_to_even(dtype):
    m = gc.midpoints(dtype)
    fin = m[m.abs() != 65520.0] if dtype == torch.float16 else m
    h = fin.to(dtype)
    b = h.view(torch.int16)
    assert bool((b & 1 == 0).all()), "torch's own cast is not to-nearest-even"
    other = torch.where(h.float().abs() < fin.abs(), b + 1, b - 1).view(dtype)
    assert torch.equal((h.double() + other.double()) / 2, fin.double())
    assert bool((h.float() != fin).all())
    lower = torch.minimum(b & 0x7FFF, other.view(torch.int16) & 0x7FFF)
    assert bool((lower & 1 == 0).any()) and bool((lower & 1 == 1).any())      # even and odd lower neighbours
    if dtype == torch.float16:
        assert torch.isinf(torch.tensor([65520.0]).to(dtype)).all() and float(torch.tensor([65519.996]).to(dtype)) == 65504.0
        blk = gc.cast_block(dtype).to(dtype)
        sub = (blk.float().abs() > 0) & (blk.float().abs() < 2.0 ** -14)
        assert int(sub.sum()) >= 6


@pytest.mark.parametrize("dtype", gc.H16)
@pytest.mark.parametrize("mul", gc.CAST_MULS)
def test_cast_reference_and_mutants(dtype, mul):
    x = gc.cast_values(dtype, 1027, mul)
    want = gc.cast_to_ref(x, mul, dtype)
    assert gc.same_bits(want, want.clone())
    prod = x * float(np.float32(mul))
    _refused(gc.assert_bits, "trunc", gc.toward_zero(prod, dtype), want)
    if mul != 3.7:                                              # the block's products are the midpoints
        blk, nm = gc.cast_block(dtype), gc.midpoints(dtype).numel()
        hit = gc._ibits(prod[5:5 + nm]) == gc._ibits(blk[:nm])
        assert int(hit.sum()) >= nm // 2 and (mul != 1.0 or gc.same_bits(prod[5:5 + blk.numel()], blk))
        _refused(gc.assert_bits, "away", gc.ties_away(prod, dtype), want)
        assert bool(torch.isnan(want).any()) and bool(torch.isinf(want).any())
        assert bool((torch.signbit(want) & (want == 0)).any())
    h = gc.h16_values(dtype, 1027)
    back = gc.cast_from_ref(h, mul)
    _refused(gc.assert_bits, "+0", torch.where(back == 0, torch.zeros(()), back), back)          # -0 turned into +0
    dst = gc.eighths((1027,), 9)
    gc.check_fma("axpy", dst + h.float() * float(np.float32(mul)), dst, h, mul)
    _refused(gc.check_fma, "overwrite", back, dst, h, mul)


# ---- weight images ---------------------------------------------------------------------------------------------------------
def test_weight_image_references_and_mutants():
    for s in gc.W_SHAPES:
        KH, KW, Cin, Cout = s
        w = gc.weight_values(s)
        f = gc.flip_ref(w)
        a, b, ci, co = KH - 1, 0, Cin - 1, Cout // 2
        assert f[KH - 1 - a, KW - 1 - b, co, ci] == w[a, b, ci, co]
        for dtype in gc.H16:
            wf, wd = gc.h16_fwd_ref(w, dtype), gc.h16_dgrad_ref(w, dtype)
            assert wf[co, (a * KW + b) * Cin + ci] == w[a, b, ci, co].to(dtype)
            assert wd[ci, ((KH - 1 - a) * KW + (KW - 1 - b)) * Cout + co] == w[a, b, ci, co].to(dtype)
            # the data-gradient image is the forward image of the flipped, transposed kernel
            assert torch.equal(wd, gc.h16_fwd_ref(f, dtype))
    w = gc.weight_values((3, 3, 40, 33))
    assert not torch.equal(gc.flip_ref(w, rotate=False), gc.flip_ref(w))                 # a tap index that is not rotated
    assert not torch.equal(gc.flip_ref(w, swap=True), gc.flip_ref(w))                    # Cin and Cout swapped in the stride
    assert not torch.equal(gc.h16_dgrad_ref(w, torch.float16, rotate=False), gc.h16_dgrad_ref(w, torch.float16))
    flat, offs = gc.flat_params()
    assert all(o % 64 == 0 for o in offs) and offs[0] >= 64
    ends = [o + int(np.prod(s)) for o, s in zip(offs, gc.W_BATCH)]
    assert all(offs[i + 1] - ends[i] >= 64 for i in range(len(offs) - 1)) and flat.numel() - ends[-1] >= 64
    tiles = [gc.n_tiles(s) for s in gc.W_BATCH]
    assert tiles[0] > 1 and tiles[1] == 1 and tiles[2] > 1 and tiles[-1] == 1 and tiles[-2] == 1
    good = torch.full_like(flat, gc.W_SENTINEL)
    for s, o in zip(gc.W_BATCH, offs):
        n = int(np.prod(s))
        good[o:o + n] = gc.flip_ref(flat[o:o + n].view(s)).reshape(-1)
    gc.check_flat_flip("good", good, flat, offs)
    for kw in (dict(rotate=False), dict(swap=True)):
        bad = good.clone()
        s, o = gc.W_BATCH[3], offs[3]
        n = int(np.prod(s))
        bad[o:o + n] = gc.flip_ref(flat[o:o + n].view(s), **kw).reshape(-1)
        _refused(gc.check_flat_flip, "bad", bad, flat, offs)
    spill = good.clone()
    spill[ends[1]] = 0.0                                        # one float past a layer
    _refused(gc.check_flat_flip, "spill", spill, flat, offs)
