"""Seeded inputs, float64 / exact references and comparison helpers for the HBM-bound glue kernels (csrc/elementwise.hip), the
optimiser (csrc/optim.hip), the 16-bit casts, epilogue backward and weight images (end of csrc/conv_h16.hip) and the float32
flip / transpose (end of csrc/conv_wgrad.hip).  numpy and CPU torch only: nothing here imports the package or touches a GPU.
tests/test_glue_gpu.py feeds the kernels' results to the check_* helpers below; tests/test_glue_cpu.py feeds the same helpers
deliberately wrong results and asserts that they are refused.

How exact (u = 2^-24, the unit roundoff of float32):
  * data movement, and one float32 operation followed by one round-to-nearest-even conversion: equal bit for bit (same_bits:
    +0 and -0 differ, NaN matches NaN);
  * a + b * c: either float32(float64(a + b c)) (fused) or float32(float32(b c) + a), bit for bit (check_fma);
  * sums of at most four multiples of 1/8 in [-4, 4]: exact in float32, so equal to the float64 sum cast down;
  * channel sums: (n + k) u sum|terms| around the float64 sum of the same float32 inputs, n addends, k roundings in a term;
  * squared norms: relative d u, d the depth of the summation read from optim.hip (sumsq_depth / grad_prepare_depth);
  * the SGD update: 4 u (|m v| + |lr g clip| + |w|) per element around the float64 update.
"""
import math

import numpy as np
import torch

U = 2.0 ** -24
ACT_NONE, ACT_RELU, ACT_SIGMOID = 0, 1, 2          # include/mrcnn_hip.h
H16 = (torch.float16, torch.bfloat16)


# ---------------------------------------------------------------------------------------------------------------------------
# comparison primitives
def _ibits(t):
    t = t.detach().cpu().contiguous()
    return t.view({4: torch.int32, 2: torch.int16, 8: torch.int64, 1: torch.uint8}[t.element_size()]) if t.is_floating_point() else t


def same_bits(got, want):
    """Equal bit for bit (so +0 != -0); a NaN matches any NaN."""
    got, want = got.detach().cpu(), want.detach().cpu()
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    if not got.is_floating_point():
        return torch.equal(got, want)
    nan = torch.isnan(want)
    if not torch.equal(torch.isnan(got), nan):
        return False
    return bool(((_ibits(got) == _ibits(want)) | nan).all())


def assert_bits(tag, got, want):
    assert same_bits(got, want), "%s: differs from the exact reference" % tag


def worst_ratio(err, bound):
    """max err / bound; 0 / 0 counts as 0, a positive error over a zero bound as inf."""
    err = np.asarray(err, dtype=np.float64)
    bound = np.broadcast_to(np.asarray(bound, dtype=np.float64), err.shape)
    if err.size == 0:
        return 0.0
    if np.isnan(err).any():
        return float("inf")
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    return float(r.max())


def check_bound(tag, got, ref64, bound, what):
    r = worst_ratio(np.abs(np.asarray(got.detach().cpu(), dtype=np.float64) - np.asarray(ref64, dtype=np.float64)), bound)
    print("[%s] max |err| / (%s) = %.3f" % (tag, what, r))
    assert r <= 1.0, "%s: %.3f x the bound %s" % (tag, r, what)
    return r


def check_fma(tag, got, a, b, c):
    """got = a + b * c elementwise in float32, contracted or not.  a, b float32 tensors (b may be 16 bit: converted exactly), c a
    float32 scalar or tensor."""
    a = a.detach().cpu().float()
    b = b.detach().cpu().float()
    c = c.detach().cpu().float() if torch.is_tensor(c) else torch.tensor(float(np.float32(c)), dtype=torch.float32)
    fused = (a.double() + b.double() * c.double()).float()
    split = (b * c) + a
    got = got.detach().cpu()
    nan = torch.isnan(split)
    assert torch.equal(torch.isnan(got), nan), "%s: NaNs differ" % tag
    ok = (_ibits(got) == _ibits(fused)) | (_ibits(got) == _ibits(split)) | nan
    assert bool(ok.all()), "%s: %d elements are neither the fused nor the two-step result" % (tag, int((~ok).sum()))
    return int((_ibits(fused) != _ibits(split)).sum())


def eighths(shape, seed):
    """Multiples of 1/8 in [-4, 4]: any four of them (plus a fifth) sum exactly in float32."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-32, 33, tuple(shape), generator=g).float() / 8


def sentinel_bytes(n, phase=0, device=None):
    """1 .. 251, never 0, period 251 (a prime: no pitch lines up with it)."""
    return ((torch.arange(n, dtype=torch.int32, device=device) + phase) % 251 + 1).to(torch.uint8)


# ---------------------------------------------------------------------------------------------------------------------------
# float32 epilogue backward: out = act(scale * z' + shift) with scale = gamma * rstd, z' = z - mean
EPI_CASES = {           # name: (C, M); the kernel the aligned call takes is in the name
    "vec_c16_m1": (16, 1), "vec_c16_m65": (16, 65), "vec_c4096_m9": (4096, 9),
    "sca_c48_m333": (48, 333), "sca_c3_m1": (3, 1),
}


def epi_case(C, M, act, seed=0):
    """float32 inputs of one call.  out = float32(act(bn(z))) evaluated in float64; under ReLU a few of its zeros become -0.0 and
    one eighth of all entries is forced to exactly 0.0, under sigmoid z is pushed far enough out for exact 0 and 1."""
    g = torch.Generator().manual_seed(1000 + seed + 7 * C + M)
    d = dict(C=C, M=M, act=act)
    d["dout"] = torch.randn(M, C, generator=g)
    d["z"] = torch.randn(M, C, generator=g) * 2 + 0.5
    d["gamma"] = torch.rand(C, generator=g) + 0.5
    d["beta"] = torch.randn(C, generator=g) * 0.3
    d["mean"] = torch.randn(C, generator=g) * 0.5 + 0.5
    d["rstd"] = 1.0 / torch.sqrt(torch.rand(C, generator=g) + 0.25)
    d["scale"] = d["gamma"] * d["rstd"]
    if act == ACT_SIGMOID and M * C >= 2:
        flat = d["z"].view(-1)
        flat[0::11] = 4000.0
        flat[1::11] = -4000.0
    y = d["gamma"].double() * (d["z"].double() - d["mean"].double()) * d["rstd"].double() + d["beta"].double()
    if act == ACT_RELU:
        out = torch.relu(y).float()
        flat = out.view(-1)
        flat[3::8] = 0.0                                       # one eighth exactly 0.0 whatever z says there
        zero = (flat == 0).nonzero().view(-1)
        flat[zero[::5]] = -0.0
        d["out"] = out
    elif act == ACT_SIGMOID:
        d["out"] = torch.sigmoid(y).float()
    else:
        d["out"] = None
    return d


def epi_ref(d):
    """float64 statement on the float32 inputs: g = dout act'(out), dz = g scale, the three channel sums, the sums of the terms'
    magnitudes and the number of float32 roundings inside one term (k)."""
    g = d["dout"].double()
    kact = 0
    if d["act"] == ACT_RELU:
        g = torch.where(d["out"] > 0, g, torch.zeros_like(g))
    elif d["act"] == ACT_SIGMOID:
        o = d["out"].double()
        g = g * o * (1 - o)
        kact = 3                                                # g o, 1 - o, their product
    dz = g * d["scale"].double()
    tg = g * (d["z"].double() - d["mean"].double()) * d["rstd"].double()
    r = dict(dy=g, dz=dz, dbeta=g.sum(0), dgamma=tg.sum(0), dbias=dz.sum(0),
             abs=dict(dbeta=g.abs().sum(0), dgamma=tg.abs().sum(0), dbias=dz.abs().sum(0)),
             k=dict(dbeta=max(kact, 1), dgamma=3 + kact, dbias=1 + kact), n=d["M"], kact=kact)
    if kact == 0:                                               # no rounding in g, one in dz: the float32 values are pinned
        g32 = g.float()
        r["dy32"], r["dz32"] = g32, g32 * d["scale"]
    return r


def epi_f32(d):
    """The same statement evaluated in float32 on the CPU (what a correct kernel may return); rows summed in order."""
    g = d["dout"].clone()
    if d["act"] == ACT_RELU:
        g = torch.where(d["out"] > 0, g, torch.zeros_like(g))
    elif d["act"] == ACT_SIGMOID:
        g = g * d["out"] * (1 - d["out"])
    dz = g * d["scale"]
    tg = g * (d["z"] - d["mean"]) * d["rstd"]
    seq = lambda t: torch.from_numpy(np.add.accumulate(t.numpy(), axis=0, dtype=np.float32)[-1].copy())
    return dict(dy=g, dz=dz, dbeta=seq(g), dgamma=seq(tg), dbias=seq(dz))


def check_epilogue(tag, ref, got):
    """got: any subset of dy, dz, dbeta, dgamma, dbias (float32 tensors).  Returns the error / bound ratios of the sums."""
    ratios = {}
    for name in ("dy", "dz"):
        if got.get(name) is None:
            continue
        if ref["kact"] == 0:
            assert_bits("%s %s" % (tag, name), got[name], ref[name + "32"])
        else:                                                   # sigmoid: kact (+1 for dz) roundings of a product
            k = ref["kact"] + (name == "dz")
            check_bound("%s %s" % (tag, name), got[name], ref[name], k * U * ref[name].abs().numpy() + 2.0 ** -149, "%d u |ref|" % k)
    for name in ("dbeta", "dgamma", "dbias"):
        if got.get(name) is None:
            continue
        n, k = ref["n"], ref["k"][name]
        ratios[name] = check_bound("%s %s" % (tag, name), got[name], ref[name], (n + k) * U * ref["abs"][name].numpy(),
                                   "(%d + %d) u sum|terms|" % (n, k))
    return ratios


# ---------------------------------------------------------------------------------------------------------------------------
# 16-bit epilogue backward
EPI16_CASES = {"c16_m1": (16, 1), "c16_m129": (16, 129), "c128_m70": (128, 70), "c4096_m5": (4096, 5), "c256_m2049": (256, 2049)}


def epi16_case(C, M, act, dtype, seed=0):
    g = torch.Generator().manual_seed(2000 + seed + 7 * C + M)
    d = dict(C=C, M=M, act=act, dtype=dtype)
    d["dout"] = (torch.randn(M, C, generator=g) * 4).to(dtype)
    d["z"] = (torch.randn(M, C, generator=g) * 2 + 0.5).to(dtype)
    d["out"] = torch.relu(torch.randn(M, C, generator=g)).to(dtype) if act == ACT_RELU else None   # half of it exactly 0
    d["mean"] = torch.randn(C, generator=g) * 0.5 + 0.5
    d["rstd"] = 1.0 / torch.sqrt(torch.rand(C, generator=g) + 0.25)
    d["scale"] = (torch.rand(C, generator=g) + 0.5) * d["rstd"]
    return d


def epi16_ref(d, gmul, bn=True):
    """dy = g and dz = float32(g scale) rounded once to the 16-bit type: exact.  Sums in float64 of the float32 terms (dbias sums
    the unrounded float32 dz, as the kernel does), times gmul (a power of two here: exact)."""
    g = d["dout"].float()
    if d["act"] == ACT_RELU:
        g = torch.where(d["out"].float() > 0, g, torch.zeros_like(g))
    scale = d["scale"] if bn else None
    dz32 = g * scale if scale is not None else g
    g64 = g.double()
    tg = g64 * (d["z"].double() - d["mean"].double()) * d["rstd"].double()
    return dict(dy16=g.to(d["dtype"]), dz16=dz32.to(d["dtype"]), n=d["M"], gmul=gmul,
                dbeta=g64.sum(0) * gmul, dgamma=tg.sum(0) * gmul, dbias=dz32.double().sum(0) * gmul,
                abs=dict(dbeta=g64.abs().sum(0) * gmul, dgamma=tg.abs().sum(0) * gmul, dbias=dz32.double().abs().sum(0) * gmul),
                k=dict(dbeta=1, dgamma=3, dbias=1))


def check_epilogue16(tag, ref, got):
    ratios = {}
    if got.get("dz") is not None:
        assert_bits(tag + " dz", got["dz"], ref["dz16"])
    if got.get("dy") is not None:
        assert_bits(tag + " dy", got["dy"], ref["dy16"])
    for name in ("dbeta", "dgamma", "dbias"):
        if got.get(name) is None:
            continue
        n, k = ref["n"], ref["k"][name]
        ratios[name] = check_bound("%s %s" % (tag, name), got[name], ref[name], (n + k) * U * ref["abs"][name].numpy(),
                                   "(%d + %d) u sum|terms|" % (n, k))
    return ratios


# ---------------------------------------------------------------------------------------------------------------------------
# 3x3 / stride 2 max pool, TF SAME
POOL_SHAPES = [(1, 1, 1, 3), (1, 2, 2, 5), (2, 7, 9, 3), (1, 8, 6, 4), (1, 17, 23, 8)]
POOL_NEG_SHAPE = (1, 8, 6, 4)            # carries an all-negative window that also touches the padding


def same_pad(size):
    out = -(-size // 2)
    return out, max((out - 1) * 2 + 3 - size, 0) // 2


def pool_input(shape, seed=0):
    """relu of normals with the positives rounded to multiples of 1/2: mostly zeros, ties among the positives."""
    g = torch.Generator().manual_seed(3000 + seed + sum(shape))
    x = torch.round(torch.relu(torch.randn(shape, generator=g)) * 2) / 2
    if tuple(shape) == POOL_NEG_SHAPE:   # rows 6, 7 x columns 4, 5 of channel 0: the last window (rows 6..8, columns 4..6) sees only these
        x[0, 6:8, 4:6, 0] = torch.tensor([[-1.0, -2.0], [-0.5, -3.0]])
    return x


def pool_ref(x, last=False, pad_zero=False):
    """Explicit scan of the window in row-major order; the FIRST maximum wins (v > best).  argmax = ih * W + iw.
    last / pad_zero: the two wrong pools of test_glue_cpu.py (last maximum wins; the padding counts as 0)."""
    x = x.numpy()
    N, H, W, C = x.shape
    (OH, pt), (OW, pl) = same_pad(H), same_pad(W)
    best = np.full((N, OH, OW, C), -np.inf, dtype=np.float32)
    bi = np.full((N, OH, OW, C), -1, dtype=np.int32)
    touches = np.zeros((OH, OW), dtype=bool)
    for oh in range(OH):
        for ow in range(OW):
            for a in range(3):
                for b in range(3):
                    ih, iw = oh * 2 - pt + a, ow * 2 - pl + b
                    if not (0 <= ih < H and 0 <= iw < W):
                        touches[oh, ow] = True
                        continue
                    v = x[:, ih, iw]
                    cur, idx = best[:, oh, ow], bi[:, oh, ow]
                    up = (idx < 0) | ((v >= cur) if last else (v > cur))
                    cur[up] = v[up]
                    idx[up] = ih * W + iw
    if pad_zero:
        best = np.where(touches[None, :, :, None], np.maximum(best, np.float32(0)), best)
    return torch.from_numpy(best), torch.from_numpy(bi)


def pool_bwd_ref(dout, argmax, shape):
    N, H, W, C = shape
    dx = np.zeros((N, H * W, C), dtype=np.float64)
    am = argmax.numpy().reshape(N, -1, C)
    do = dout.double().numpy().reshape(N, -1, C)
    n, _, c = np.meshgrid(np.arange(N), np.arange(am.shape[1]), np.arange(C), indexing="ij")
    ok = am >= 0
    np.add.at(dx, (n[ok], am[ok], c[ok]), do[ok])
    return torch.from_numpy(dx.reshape(N, H, W, C)).float()


def pool_case(shape):
    x = pool_input(shape)
    out, am = pool_ref(x)
    dout = eighths(out.shape, 3100 + sum(shape))
    return dict(x=x, out=out, argmax=am, dout=dout, dx=pool_bwd_ref(dout, am, shape))


def check_pool(tag, case, out=None, argmax=None, dx=None):
    if out is not None:
        assert_bits(tag + " out", out, case["out"])
    if argmax is not None:
        assert torch.equal(argmax.cpu(), case["argmax"]), tag + ": argmax is not the first maximum of the window"
    if dx is not None:
        assert_bits(tag + " dx", dx, case["dx"])


def pool_stats(x):
    """(share of zeros, share of windows whose positive maximum occurs more than once)."""
    N, H, W, C = x.shape
    (OH, pt), (OW, pl) = same_pad(H), same_pad(W)
    tied = total = 0
    xn = x.numpy()
    for oh in range(OH):
        for ow in range(OW):
            r0, c0 = max(oh * 2 - pt, 0), max(ow * 2 - pl, 0)
            win = xn[:, r0:min(oh * 2 - pt + 3, H), c0:min(ow * 2 - pl + 3, W)].reshape(N, -1, C)
            m = win.max(1, keepdims=True)
            tied += int((((win == m).sum(1) > 1) & (m[:, 0] > 0)).sum())
            total += N * C
    return float((x == 0).float().mean()), tied / total


# ---------------------------------------------------------------------------------------------------------------------------
# resampling and the small kernels
SUBSAMPLE_SHAPES = [(2, 7, 5, 3), (1, 1, 1, 1), (2, 8, 8, 256)]
UPSAMPLE_SHAPES = [(2, 3, 5, 3), (1, 1, 1, 1)]                   # of dsrc; dout is [N, 2H, 2W, C]
UNSHUFFLE_C = (4, 12, 256)


def subsample_ref(x):
    return x[:, ::2, ::2, :].contiguous()


def subsample_bwd_ref(dout, dx0):
    dx = dx0.double().clone()
    dx[:, ::2, ::2, :] += dout.double()
    return dx.float()


def upsample_bwd_ref(dout, dsrc0, accumulate):
    N, H2, W2, C = dout.shape
    s = dout.double().view(N, H2 // 2, 2, W2 // 2, 2, C).sum((2, 4))
    return (s + dsrc0.double() if accumulate else s).float()


def unshuffle_ref(src):
    N, H2, W2, C = src.shape
    return src.view(N, H2 // 2, 2, W2 // 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(N, H2 // 2, W2 // 2, 4 * C).contiguous()


def bn_case(n, seed=0):
    g = torch.Generator().manual_seed(3500 + seed + n)
    return dict(gamma=torch.rand(n, generator=g) + 0.5, beta=torch.randn(n, generator=g), mean=torch.randn(n, generator=g),
                var=torch.rand(n, generator=g) * 4 + 1e-3)


def bn_ref(d, eps):
    eps = float(np.float32(eps))
    r = 1.0 / torch.sqrt(d["var"].double() + eps)
    s = d["gamma"].double() * r
    return dict(rstd=r, scale=s, shift=d["beta"].double() - d["mean"].double() * s, mean_scale=(d["mean"].double() * s).abs())


def check_bn_fold(tag, d, ref, scale, shift, rstd=None):
    """rstd: var + eps, sqrt, divide -- each correctly rounded, the square root halving the first: 3 u.  scale one more.
    shift = beta - mean * scale: the 4 u of scale on the product, the product's own rounding and the difference's."""
    out = {}
    if rstd is not None:
        out["rstd"] = check_bound(tag + " rstd", rstd, ref["rstd"], 3 * U * ref["rstd"].numpy(), "3 u |rstd|")
    out["scale"] = check_bound(tag + " scale", scale, ref["scale"], 4 * U * ref["scale"].abs().numpy(), "4 u |scale|")
    b = 6 * U * ref["mean_scale"].numpy() + U * ref["shift"].abs().numpy()
    out["shift"] = check_bound(tag + " shift", shift, ref["shift"], b, "6 u |mean scale| + u |shift|")
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# copy2d / fill_zero on byte buffers with guard bytes (device-agnostic: the large cases are built and compared on the device)
GUARD = 64


def copy2d_expected(dst0, dst_off, dst_pitch, src, src_off, src_pitch, row_bytes, rows, ignore_dst_pitch=False):
    """dst0 / src: uint8 buffers; returns what dst must hold afterwards (every other byte unchanged)."""
    out = dst0.clone()
    dp = row_bytes if ignore_dst_pitch else dst_pitch
    out.as_strided((rows, row_bytes), (dp, 1), dst_off).copy_(src.as_strided((rows, row_bytes), (src_pitch, 1), src_off))
    return out


def copy2d_buffers(dst_pitch, src_pitch, row_bytes, rows, dst_shift=0, src_shift=0, device=None):
    """Two sentinel-filled byte buffers: GUARD bytes, the addressed range (the last row ends after row_bytes), GUARD bytes.
    Returns (dst0, dst_off, src, src_off); the shifts move the addressed range (an unaligned pointer)."""
    span = lambda pitch: (rows - 1) * pitch + row_bytes
    dst0 = sentinel_bytes(2 * GUARD + span(dst_pitch) + dst_shift, 0, device)
    src = sentinel_bytes(2 * GUARD + span(src_pitch) + src_shift, 97, device)
    return dst0, GUARD + dst_shift, src, GUARD + src_shift


def fill_expected(buf0, off, nbytes):
    out = buf0.clone()
    out[off:off + nbytes] = 0
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# optimiser
OPT_SIZES = (64, 64 * 4097, 2 ** 21 + 64 * 37)
SGD_BIG = 2 ** 23 + 64 * 5
COEFS = (0.0, 2.0 ** -9, 3e-4)


def gran_table(n, last_trainable=False):
    """Coefficient per 64-float granule: trainable granules cycle through 0 / 2^-9 / 3e-4 (coef == 0 beside coef > 0); frozen
    (-1) are the first and last two granules, the last granule of every workgroup's 16 with the first of the next (both the
    vector kernels walk 256 x 4 floats = 16 granules per workgroup and trip), and every other granule of a stretch in the middle."""
    ng = n // 64
    idx = np.arange(ng)
    coef = np.asarray(COEFS, dtype=np.float32)[idx % 3]
    if ng == 1:
        return torch.from_numpy(coef.copy())
    frozen = (idx < 2) | (idx >= ng - 2) if ng >= 8 else (idx == 0)
    frozen |= ((idx % 16 == 15) | (idx % 16 == 0)) & (idx > 0) & (ng > 16)
    mid = (idx >= ng // 2) & (idx < ng // 2 + 40)
    frozen |= mid & (idx % 2 == 1)
    frozen &= ~(mid & (idx % 2 == 0) & (idx % 16 != 15) & (idx % 16 != 0))
    if last_trainable:
        frozen[-1] = False
    coef = coef.copy()
    coef[frozen] = -1.0
    return torch.from_numpy(coef)


def opt_case(n, seed=0, exact=False):
    """grads / params / momentum.  exact: small integers over 8 (with the power-of-two coefficient and scale every product and
    sum of grad_prepare is then exact)."""
    g = torch.Generator().manual_seed(4000 + seed + n % 9973)
    if exact:
        mk = lambda: torch.randint(-16, 17, (n,), generator=g).float() / 8
    else:
        mk = lambda: torch.randn(n, generator=g)
    return dict(grads=mk() * (1 if exact else 0.1), params=mk(), mom=mk() * (1 if exact else 0.01))


def grad_prepare_check(tag, got_g, grads, params, scale, coef):
    """Per element: frozen -> exactly 0; coef == 0 -> float32(g scale); else float32(g scale) + coef w, fused or not."""
    c = coef.repeat_interleave(64)
    gs = grads * float(np.float32(scale))
    got_g = got_g.cpu()
    fr = c < 0
    assert bool((got_g[fr] == 0).all()), tag + ": a frozen granule's gradient is not 0"
    z = c == 0
    assert_bits(tag + " coef == 0", got_g[z], gs[z])
    p = c > 0
    return check_fma(tag + " coef > 0", got_g[p], gs[p], params[p], c[p])


def sumsq_depth(n):
    """Depth of mrcnn_sumsq's summation: blocks = min(ceil(n / 2048), 1024) of 256 threads; a thread adds ceil(n / (256 blocks))
    squares, then 6 wave levels, 2 levels of the 4-way LDS add; the final kernel adds ceil(blocks / 256) partials per thread and
    folds 256 threads in 8 levels; + 1 for the rounding of the square."""
    blocks = min(-(-n // 2048), 1024)
    return -(-n // (256 * blocks)) + 6 + 2 + -(-blocks // 256) + 8 + 1


def grad_prepare_depth(n):
    """As sumsq_depth with 4 squares per trip: blocks = min(ceil(n / 4 / 512), 1024), ceil(n / 4 / (256 blocks)) trips of 4."""
    blocks = min(-(-(n // 4) // 512), 1024)
    return 4 * -(-(n // 4) // (256 * blocks)) + 6 + 2 + -(-blocks // 256) + 8 + 1


def check_norm(tag, got, values, depth):
    """got: the kernel's scalar; values: the float32 numbers whose squares it summed."""
    ref = float((values.double() ** 2).sum())
    got = float(got)
    r = worst_ratio([abs(got - ref)], [depth * U * ref])
    print("[%s] |sumsq - ref| / (%d u ref) = %.3f" % (tag, depth, r))
    assert r <= 1.0, "%s: %.3f x the bound of depth %d" % (tag, r, depth)
    return r


def clip_factor(sumsq32, clipnorm, strict=False):
    """The float32 scalar the kernel derives: clipnorm / sqrt(sumsq) when the norm is >= clipnorm (K.clip_norm), else 1; both
    operations are correctly rounded on either side.  strict: `>` in place of `>=`."""
    clipnorm = np.float32(clipnorm)
    if not clipnorm > 0:
        return np.float32(1.0)
    norm = np.sqrt(np.float32(sumsq32))
    hit = norm > clipnorm if strict else norm >= clipnorm
    return np.float32(clipnorm / norm) if hit else np.float32(1.0)


def sgd_ref(c, coef, clip, lr, momentum):
    """float64 update with the float32 scalars as the kernel holds them: v = m v - lr (g clip), w += v on trainable granules."""
    lr, momentum, clip = float(np.float32(lr)), float(np.float32(momentum)), float(clip)
    tr = (coef.repeat_interleave(64) >= 0)
    g, v0, w0 = c["grads"].double(), c["mom"].double(), c["params"].double()
    mv, lg = momentum * v0, lr * g * clip
    v = torch.where(tr, mv - lg, v0)
    w = torch.where(tr, w0 + v, w0)
    return dict(v=v, w=w, tr=tr, bound_v=4 * U * (mv.abs() + lg.abs()), bound_w=4 * U * (mv.abs() + lg.abs() + w0.abs()))


def check_sgd(tag, c, ref, got_w, got_v):
    """Frozen granules keep parameter and momentum bit for bit.  Trainable: momentum m v (1 rounding), lr (g clip) (2), the
    difference (1): 2 u |m v| + 3 u |lr g clip| <= the bound; the parameter adds one rounding of w + v:
    3 u |m v| + 4 u |lr g clip| + u |w| <= 4 u (|m v| + |lr g clip| + |w|)."""
    got_w, got_v, fr = got_w.cpu(), got_v.cpu(), ~ref["tr"]
    assert same_bits(got_w[fr], c["params"][fr]) and same_bits(got_v[fr], c["mom"][fr]), tag + ": a frozen granule was updated"
    tr = ref["tr"]
    rv = check_bound(tag + " momentum", got_v[tr], ref["v"][tr], ref["bound_v"][tr].numpy(), "4 u (|m v| + |lr g clip|)")
    rw = check_bound(tag + " params", got_w[tr], ref["w"][tr], ref["bound_w"][tr].numpy(), "4 u (|m v| + |lr g clip| + |w|)")
    return rv, rw


def sgd_f32(c, coef, clip, lr, momentum, touch_frozen=False):
    """The update in float32 on the CPU, as the kernel writes it.  touch_frozen: the wrong optimiser of test_glue_cpu.py."""
    tr = (coef.repeat_interleave(64) >= 0) | touch_frozen
    lr, momentum, clip = np.float32(lr), np.float32(momentum), np.float32(clip)
    v = torch.where(tr, float(momentum) * c["mom"] - float(lr) * (c["grads"] * float(clip)), c["mom"])
    w = torch.where(tr, c["params"] + v, c["params"])
    return w, v


# ---------------------------------------------------------------------------------------------------------------------------
# casts
CAST_LENGTHS = (1, 2, 3, 5, 8, 1027, 1032, 2 ** 20 + 13, 2 ** 20 + 16)
CAST_MULS = (1.0, 1.0 / 1024, 3.7, 1024.0)


def _next_up_bits(dtype, bits):
    return torch.tensor(bits, dtype=torch.int16).view(dtype), torch.tensor([b + 1 for b in bits], dtype=torch.int16).view(dtype)


def midpoints(dtype):
    """float32 values exactly half way between two adjacent 16-bit values, lower neighbour with an even and with an odd last bit,
    both signs; float16 also between subnormals and between the largest finite value and 2^16 (65520: rounds to inf)."""
    if dtype == torch.float16:
        bits = [0x3C00, 0x3C01, 0x3C02, 0x3C03, 0x4BFE, 0x4BFF, 0x0400, 0x0401, 0x0001, 0x0002, 0x03FE, 0x03FF, 0x7BFD, 0x7BFE]
    else:
        bits = [0x3F80, 0x3F81, 0x3F82, 0x3F83, 0x40FE, 0x40FF, 0x0080, 0x0081, 0x7F00, 0x7F01, 0x1234, 0x1235]
    lo, hi = _next_up_bits(dtype, bits)
    mid = ((lo.double() + hi.double()) / 2).float()
    if dtype == torch.float16:
        mid = torch.cat([mid, torch.tensor([65520.0])])          # half way between 65504 and 2^16
    return torch.cat([mid, -mid])


def cast_block(dtype):
    """The fixed block: midpoints, the edges of the finite range, values that become subnormal, zeros, infinities, NaN."""
    parts = [midpoints(dtype)]
    if dtype == torch.float16:
        parts.append(torch.tensor([65504.0, 65519.996, 65520.0, -65504.0, -65519.996, -65520.0, 65536.0, 1e6]))
        parts.append(torch.tensor([2.0 ** -14, 2.0 ** -15, 3 * 2.0 ** -24, 2.0 ** -24, 2.0 ** -25, 1.5 * 2.0 ** -25, 2.0 ** -26, 5.1e-6,
                                   -2.0 ** -15, -2.0 ** -25, -4.3e-7]))
    else:
        parts.append(torch.tensor([3.3895314e38, 3.4e38, -3.4e38, 2.0 ** -126, 2.0 ** -127, 3 * 2.0 ** -133, 2.0 ** -134, -2.0 ** -130]))
    parts.append(torch.tensor([0.0, -0.0, float("inf"), float("-inf"), float("nan"), 1.0, -1.0]))
    return torch.cat(parts)


def cast_values(dtype, n, mul=1.0, seed=0):
    """n float32 values: seeded normals; from n = 1027 on the fixed block sits at offset 5, divided by `mul` when that is a power
    of two (exact), so that the PRODUCT is the midpoint / edge."""
    g = torch.Generator().manual_seed(5000 + seed + n % 9973)
    x = torch.randn(n, generator=g) * 3
    blk = cast_block(dtype)
    if n >= blk.numel() + 5:
        if math.frexp(mul)[0] == 0.5:                             # where the division neither overflows nor loses bits
            pre = blk / mul
            blk = torch.where(_ibits(pre * mul) == _ibits(blk), pre, blk)
        x[5:5 + blk.numel()] = blk
    return x


def cast_to_ref(x, mul, dtype):
    return (x * float(np.float32(mul))).to(dtype)


def cast_from_ref(h, mul):
    return h.float() * float(np.float32(mul))


def h16_values(dtype, n, seed=0):
    """16-bit inputs of cast_from / axpy: the rounded cast_values (so subnormals, zeros, infinities and NaN included)."""
    return cast_values(dtype, n, 1.0, seed).to(dtype)


def toward_zero(x, dtype):
    """x * 1 truncated to the 16-bit type (a wrong cast)."""
    h = x.to(dtype)
    b = h.view(torch.int16).clone()
    over = (h.float().abs() > x.abs()) & torch.isfinite(x)
    b[over] -= 1                                                # sign-magnitude: one step towards zero
    return b.view(dtype)


def ties_away(x, dtype):
    """Round to nearest with ties away from zero (a wrong cast)."""
    h = x.to(dtype)
    b = h.view(torch.int16).clone()
    up = (b + 1).view(dtype)
    fin = torch.isfinite(x) & torch.isfinite(h)
    tie = fin & (h.float().abs() < x.abs()) & ((h.double() + torch.where(fin, up, h).double()) / 2 == x.double())
    tie |= fin & (h.float().abs() < x.abs()) & torch.isinf(up) & (x.abs() == 65520.0) & (dtype == torch.float16)
    b[tie] += 1
    return b.view(dtype)


# ---------------------------------------------------------------------------------------------------------------------------
# weight images
W_SHAPES = [(1, 1, 1, 1), (7, 7, 3, 64), (3, 3, 40, 33), (1, 1, 256, 1024), (2, 2, 64, 32)]
# the batched table: many tiles, one tile, many, many, many, one tile twice in a row (a second and third 1 x 1 x 1 x 1 layer) --
# every kind of boundary the tile -> layer binary search has to place
W_BATCH = [(1, 1, 256, 1024), (1, 1, 1, 1), (7, 7, 3, 64), (3, 3, 40, 33), (2, 2, 64, 32), (1, 1, 1, 1), (1, 1, 1, 1)]
W_SENTINEL = -7.75


def n_tiles(shape):
    kh, kw, cin, cout = shape
    return kh * kw * ((cin + 31) // 32) * ((cout + 31) // 32)


def weight_values(shape, seed=0):
    g = torch.Generator().manual_seed(6000 + seed + sum(shape))
    return torch.randn(shape, generator=g)


def flat_layout(shapes=W_BATCH):
    """Offsets (floats, multiples of 64) of the layers in one flat buffer with at least 64 sentinel floats before, between and
    after them; returns (offsets, total)."""
    offs, at = [], 64
    for s in shapes:
        offs.append(at)
        at += -(-int(np.prod(s)) // 64) * 64 + 64 * (1 + len(offs) % 3)
    return offs, at


def flat_params(shapes=W_BATCH):
    offs, total = flat_layout(shapes)
    flat = torch.full((total,), W_SENTINEL)
    for i, (s, o) in enumerate(zip(shapes, offs)):
        flat[o:o + int(np.prod(s))] = weight_values(s, i).reshape(-1)
    return flat, offs


def flip_ref(w, rotate=True, swap=False):
    """[KH, KW, Cout, Cin] with the taps rotated by 180 degrees.  rotate=False / swap=True: the two wrong images."""
    KH, KW, Cin, Cout = w.shape
    r = (w.flip(0, 1) if rotate else w).permute(0, 1, 3, 2).contiguous()
    if swap:                                                    # rows written Cout apart where they are Cin long
        r = r.view(KH * KW, Cout, Cin).transpose(1, 2).contiguous().view(KH, KW, Cout, Cin)
    return r


def h16_fwd_ref(w, dtype):
    KH, KW, Cin, Cout = w.shape
    return w.permute(3, 0, 1, 2).reshape(Cout, KH * KW * Cin).to(dtype)


def h16_dgrad_ref(w, dtype, rotate=True):
    KH, KW, Cin, Cout = w.shape
    return (w.flip(0, 1) if rotate else w).permute(2, 0, 1, 3).reshape(Cin, KH * KW * Cout).to(dtype)


def check_flat_flip(tag, got_flat, flat, offs, shapes=W_BATCH, only=None):
    """got_flat: the transposed flat buffer, pre-filled with the sentinel.  Layers in `only` (default all) hold their image,
    every other float still the sentinel."""
    want = torch.full_like(flat, W_SENTINEL)
    for i, (s, o) in enumerate(zip(shapes, offs)):
        if only is None or i in only:
            n = int(np.prod(s))
            want[o:o + n] = flip_ref(flat[o:o + n].view(s)).reshape(-1)
    assert_bits(tag, got_flat, want)
