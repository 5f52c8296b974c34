"""BatchNorm HIP kernels (csrc/batchnorm.hip) and the conv-epilogue
statistics path against a float64 reference written out below.

Error measure: PER ELEMENT, never per tensor.  For an fp32 output
    |got - want| <= TOL32 * (|want| + s_c)
where s_c is the per-channel scale of the quantity (|gamma_c| + |beta_c| for
y, the per-channel max |want| for an activation gradient, the sum of the
absolute summands for a per-channel sum).  A bf16 output adds its own
half-ulp rounding.  Half an ulp of a bf16 number v (8 significant bits) is
2^(floor(log2 |v|) - 8): that is 2^-9 * |v| only at the top of a binade and
2^-8 * |v| at its bottom, so the flat term 2^-9 * |want| is missed by a
correctly rounded store (measured: 1.99x, profiles/bn_numerics.md) and the
exact half-ulp is used instead; a truncating store (a whole ulp) still fails.
The reference is computed from the exact values the kernel reads (bf16 inputs
are upcast), so input quantisation never enters the tolerance.
"""

import functools
import itertools

import pytest
import torch
import torch.nn.functional as F

from conv_menus import BN_CONV_CASES

pytestmark = pytest.mark.gpu

EPS = 1e-5
U32 = 2.0 ** -24          # fp32 unit roundoff
# 4x the worst normalised error of stock fp32 torch batch_norm (forward and
# autograd) against the float64 reference over every case of this file,
# 3.480e-07 (y of (2,128,7,4) f32 with residual + ELU); measured values per
# case and quantity are in profiles/bn_numerics.md.
TOL32 = 4 * 3.480e-07

F32, BF16 = torch.float32, torch.bfloat16


def _ext():
    import fedkit.ops
    assert fedkit.ops.has_ext(), "fedkit._C must be built on a GPU box"
    return fedkit.ops.ext()


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def _pc(v):
    """[C] -> broadcastable over (N, C, H, W)."""
    return v.view(1, -1, 1, 1)


def half_ulp_bf16(v):
    """Half the spacing of bf16 numbers at magnitude v (float64 tensor):
    v = m * 2^e with m in [0.5, 1) has floor(log2 v) = e - 1."""
    _, e = torch.frexp(v.abs().clamp_min(2.0 ** -126))
    return torch.exp2(e.double() - 9)


def nerr(got, want, scale, out_bf16=False):
    """Worst per-element error in units of the allowed error:
    max |got - want| / (TOL32*(|want| + scale) [+ half_ulp_bf16]).  <= 1
    passes.  The half ulp is taken at max(|want|, |got|): the fp32 value that
    was rounded may sit just across a binade boundary from want.
    Returned together with the error normalised by (|want| + scale) alone,
    which is the figure profiles/bn_numerics.md records."""
    got = got.double()
    want = want.double()
    assert got.shape == want.shape, (got.shape, want.shape)
    diff = (got - want).abs()
    base = want.abs() + scale
    allowed = TOL32 * base
    if out_bf16:
        allowed = allowed + half_ulp_bf16(torch.maximum(want.abs(),
                                                        got.abs()))
    # a NaN anywhere must fail: nan_to_num maps it to +inf
    ratio = torch.nan_to_num(diff / allowed.clamp_min(1e-300), nan=float("inf"))
    raw = torch.nan_to_num(diff / base.clamp_min(1e-300), nan=float("inf"))
    return ratio.max().item(), raw.max().item()


def check(name, got, want, scale, out_bf16=False):
    ratio, raw = nerr(got, want, scale, out_bf16)
    print(f"  {name}: err/(|want|+s_c) = {raw:.3e}  (allowed units {ratio:.3f})")
    assert ratio <= 1.0, f"{name}: {ratio:.3f}x the allowed per-element error"


# ------------------------------------------------------------- f64 reference

def ref_stats(x):
    """mean, biased var, unbiased var (count == 1 keeps var) in float64."""
    xd = x.double()
    count = xd.numel() // xd.shape[1]
    mean = xd.sum((0, 2, 3)) / count
    var = ((xd - _pc(mean)) ** 2).sum((0, 2, 3)) / count
    unb = var * count / (count - 1) if count > 1 else var
    return mean, var, unb


def ref_fwd(x, gamma, beta, mean, var, elu=False, res=None, pad_out=0):
    """y (float64) from given statistics; res is the UNPADDED residual."""
    invstd = 1.0 / torch.sqrt(var + EPS)
    xhat = (x.double() - _pc(mean)) * _pc(invstd)
    z = xhat * _pc(gamma.double()) + _pc(beta.double())
    if res is not None:
        z = z + res.double()
    y = torch.where(z > 0, z, torch.expm1(z)) if elu else z
    if pad_out:
        y = F.pad(y, (pad_out,) * 4)
    return y, xhat, invstd


def ref_bwd(dy, xhat, invstd, gamma, y_saved=None):
    """g, dx, dgamma, dbeta in float64.  With a fused ELU the derivative is
    taken from the kernel's own saved y (what the kernel defines; keeps the
    comparison off the y ~ 0 discontinuity)."""
    g = dy.double()
    if y_saved is not None:
        ys = y_saved.double()
        g = g * torch.where(ys > 0, torch.ones_like(ys), ys + 1.0)
    count = g.numel() // g.shape[1]
    sg = g.sum((0, 2, 3))
    sgx = (g * xhat).sum((0, 2, 3))
    dx = _pc(gamma.double() * invstd) * (g - _pc(sg / count)
                                         - xhat * _pc(sgx / count))
    abs_g = g.abs().sum((0, 2, 3))
    abs_gx = (g * xhat).abs().sum((0, 2, 3))
    return g, dx, sgx, sg, abs_gx, abs_g


def chan_max(t):
    return _pc(t.abs().amax((0, 2, 3)))


# ----------------------------------------------------------------- the menu

# (shape, dtype): which loop of the reduction kernels each one reaches is in
# profiles/bn_numerics.md.  VEC = 4 (f32) / 8 (bf16) channels per lane.
LOOP_CASES = [
    ((1, 64, 1, 1), F32), ((1, 64, 1, 1), BF16),       # count == 1
    ((2, 8, 3, 5), F32), ((2, 8, 3, 5), BF16),         # less than one block
    ((9, 64, 61, 61), F32),     # 535824 vec > 4*512*256: cap, 4x loop, tail
    ((5, 64, 61, 67), BF16),    # 163480 vec in (1x, 2x) capped grid: bwd 2x
    ((3, 1024, 5, 7), F32), ((3, 2048, 5, 7), BF16),   # Cv = 256, members = 1
    ((4, 4, 9, 7), F32), ((4, 8, 9, 7), BF16),         # Cv = 1
]
EPI_SHAPES = [(3, 64, 5, 9), (2, 128, 7, 4)]
EVAL_SHAPES = [(3, 64, 5, 9), (3, 1024, 5, 7)]


def _id(v):
    if isinstance(v, torch.dtype):
        return "f32" if v == F32 else "bf16"
    if isinstance(v, tuple):
        return "x".join(str(i) for i in v)
    return str(v)


@functools.lru_cache(maxsize=None)
def make_case(shape, dtype, seed=11):
    """Inputs drawn once per (shape, dtype) and the float64 statistics of the
    exact values the kernel sees.  x = randn * sigma_c + mu_c with per-channel
    mu in [-1, 1] and sigma in [0.5, 1.5] (|mean|/std <= 2, the range of a
    conv output; conditioning beyond it is test_variance_conditioning's
    job), so mixing two channels up changes the answer."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    N, C, H, W = shape

    def rnd(*s):
        return torch.randn(*s, device="cuda", generator=g)

    def uni(*s):
        return torch.rand(*s, device="cuda", generator=g)

    mu = uni(C) * 2 - 1
    sigma = uni(C) + 0.5
    x = _cl((rnd(N, C, H, W) * _pc(sigma) + _pc(mu)).to(dtype))
    case = {
        "x": x,
        "dy": _cl(rnd(N, C, H, W).to(dtype)),
        "gamma": uni(C) + 0.5,
        "beta": rnd(C),
        "rm0": rnd(C),
        "rv0": uni(C) + 0.5,
    }
    case["mean"], case["var"], case["unb"] = ref_stats(x)
    # scale of the statistics themselves: a mean is a sum of |x| / count
    case["absmean"] = x.double().abs().sum((0, 2, 3)) / (N * H * W)
    return case


def check_stats(case, sm, siv, rm, rv, momentum):
    mean, var, unb = case["mean"], case["var"], case["unb"]
    invstd = 1.0 / torch.sqrt(var + EPS)
    check("save_mean", sm, mean, case["absmean"])
    check("save_invstd", siv, invstd, invstd)
    rm_want = (1 - momentum) * case["rm0"].double() + momentum * mean
    rv_want = (1 - momentum) * case["rv0"].double() + momentum * unb
    check("running_mean", rm, rm_want,
          (1 - momentum) * case["rm0"].double().abs()
          + momentum * case["absmean"])
    check("running_var", rv, rv_want, rv_want)


# ------------------------------------------------- 1. loop coverage, plain BN

@pytest.mark.parametrize("momentum", [0.1, 0.37])
@pytest.mark.parametrize("shape,dtype", LOOP_CASES, ids=_id)
def test_plain_bn_loops(shape, dtype, momentum):
    ext = _ext()
    c = make_case(shape, dtype)
    bf = dtype == BF16
    rm, rv = c["rm0"].clone(), c["rv0"].clone()
    y, sm, siv = ext.bn_fwd(c["x"], c["gamma"], c["beta"], rm, rv, True,
                            momentum, EPS)
    assert y.dtype == dtype and y.is_contiguous(
        memory_format=torch.channels_last)
    check_stats(c, sm, siv, rm, rv, momentum)
    yref, xhat, invstd = ref_fwd(c["x"], c["gamma"], c["beta"], c["mean"],
                                 c["var"])
    s_y = _pc(c["gamma"].double().abs() + c["beta"].double().abs())
    check("y", y, yref, s_y, bf)

    gx, gw, gb = ext.bn_bwd(c["dy"], c["x"], c["gamma"], sm, siv)
    _, dx, dgam, dbeta, abs_gx, abs_g = ref_bwd(c["dy"], xhat, invstd,
                                                c["gamma"])
    check("dx", gx, dx, chan_max(dx), bf)
    check("dgamma", gw, dgam, abs_gx)
    check("dbeta", gb, dbeta, abs_g)


# ---------------------------------------------------------- 2. rejected calls

def _plain(C, dtype, shape=None):
    shape = shape or (2, C, 3, 3)
    x = _cl(torch.randn(*shape, device="cuda").to(dtype))
    return (x, torch.ones(C, device="cuda"), torch.zeros(C, device="cuda"),
            torch.full((C,), 0.25, device="cuda"),
            torch.full((C,), 1.5, device="cuda"))


def _rejects_fwd(x, gamma, beta, rm, rv, **kw):
    """bn_fwd must raise and must not have touched the running statistics
    (the first kernel of every statistics path updates them)."""
    rm0, rv0 = rm.clone(), rv.clone()
    with pytest.raises(RuntimeError):
        _ext().bn_fwd(x, gamma, beta, rm, rv, True, 0.1, EPS, **kw)
    torch.cuda.synchronize()
    assert torch.equal(rm, rm0) and torch.equal(rv, rv0)


@pytest.mark.parametrize("C,dtype", [(2048, F32), (24, F32), (96, F32),
                                     (12, BF16), (24, BF16)], ids=_id)
def test_rejected_channel_counts(C, dtype):
    x, gamma, beta, rm, rv = _plain(C, dtype, (1, C, 2, 2))
    _rejects_fwd(x, gamma, beta, rm, rv)
    with pytest.raises(RuntimeError):
        _ext().bn_bwd(torch.ones_like(x), x, gamma, rm, rv)
    torch.cuda.synchronize()


def test_rejected_arguments():
    ext = _ext()
    C = 64
    x, gamma, beta, rm, rv = _plain(C, F32)
    # NCHW-contiguous input
    xn = torch.randn(2, C, 3, 3, device="cuda")
    assert not xn.is_contiguous(memory_format=torch.channels_last)
    _rejects_fwd(xn, gamma, beta, rm, rv)
    # residual of the other dtype, and of the wrong geometry
    _rejects_fwd(x, gamma, beta, rm, rv, residual=x.to(BF16), elu=True)
    _rejects_fwd(x, gamma, beta, rm, rv, residual=x, elu=True, res_pad=1)
    # backward: pad_in / want_g without the saved fused-ELU output
    gy = torch.ones_like(x)
    with pytest.raises(RuntimeError):
        ext.bn_bwd(gy, x, gamma, rm, rv, pad_in=1)
    with pytest.raises(RuntimeError):
        ext.bn_bwd(gy, x, gamma, rm, rv, want_g=True)
    with pytest.raises(RuntimeError):
        ext.bn_bwd(xn, x, gamma, rm, rv)
    torch.cuda.synchronize()


def test_rejected_conv_part():
    C, M = 128, 2 * 3 * 3
    x, gamma, beta, rm, rv = _plain(C, BF16)
    ok_tiles = (M + 63) // 64

    def part(*shape):
        return torch.zeros(*shape, device="cuda")

    # channel blocks do not match C
    _rejects_fwd(x, gamma, beta, rm, rv, conv_part=part(1, ok_tiles, 2, 64))
    _rejects_fwd(x, gamma, beta, rm, rv, conv_part=part(2, ok_tiles, 2, 32))
    # a tile-row count no launch of the conv can produce for this M
    _rejects_fwd(x, gamma, beta, rm, rv,
                 conv_part=part(2, ok_tiles + 1, 2, 64))
    _rejects_fwd(x, gamma, beta, rm, rv, conv_part=part(2, 0, 2, 64))
    # right shape, not contiguous / not on the device / not fp32
    _rejects_fwd(x, gamma, beta, rm, rv,
                 conv_part=part(2, ok_tiles, 2, 128)[..., ::2])
    _rejects_fwd(x, gamma, beta, rm, rv,
                 conv_part=torch.zeros(2, ok_tiles, 2, 64))
    _rejects_fwd(x, gamma, beta, rm, rv,
                 conv_part=part(2, ok_tiles, 2, 64).double())


# ------------------------------------- 3. epilogue variants, non-square shapes

SENTINEL = 1e4


def epilogue_combos():
    """(elu, res_pad or None for no residual, pad_out)."""
    return list(itertools.product([False, True], [None, 0, 1, 2], [0, 1, 2]))


def run_epilogue_combo(c, dtype, elu, rpad, pad_out, report=check):
    ext = _ext()
    bf = dtype == BF16
    x, gamma, beta = c["x"], c["gamma"], c["beta"]
    N, C, H, W = x.shape
    tag = f"elu={int(elu)} res={rpad} pad_out={pad_out}"
    res = res_buf = None
    if rpad is not None:
        res = _cl(c["dy"].flip(0))         # any tensor unrelated to x
        res_buf = res
        if rpad:
            # the border holds a sentinel: a kernel that reads the border
            # instead of the interior is off by 1e4
            res_buf = _cl(torch.full((N, C, H + 2 * rpad, W + 2 * rpad),
                                     SENTINEL, device="cuda", dtype=dtype))
            res_buf[:, :, rpad:-rpad, rpad:-rpad] = res
    rm, rv = c["rm0"].clone(), c["rv0"].clone()
    y, sm, siv = ext.bn_fwd(x, gamma, beta, rm, rv, True, 0.1, EPS,
                            residual=res_buf, elu=elu, pad_out=pad_out,
                            res_pad=rpad or 0)
    assert tuple(y.shape) == (N, C, H + 2 * pad_out, W + 2 * pad_out)
    yref, xhat, invstd = ref_fwd(x, gamma, beta, c["mean"], c["var"], elu,
                                 res, pad_out)
    s_y = _pc(gamma.double().abs() + beta.double().abs())
    # the WHOLE padded buffer: interior against the reference ...
    report(f"y[{tag}]", y, yref, s_y, bf)
    if pad_out:
        # ... and every border element exactly zero
        border = torch.ones(H + 2 * pad_out, W + 2 * pad_out, device="cuda",
                            dtype=torch.float64)
        border[pad_out:-pad_out, pad_out:-pad_out] = 0
        leak = torch.nan_to_num(y.double() * border, nan=1.0).abs().max()
        assert leak.item() == 0.0, f"{tag}: border not exactly zero"
    if not elu:
        if rpad is None and pad_out == 0:
            gx, gw, gb = ext.bn_bwd(c["dy"], x, gamma, sm, siv)
            _, dx, dgam, dbeta, agx, ag = ref_bwd(c["dy"], xhat, invstd, gamma)
            report(f"dx[{tag}]", gx, dx, chan_max(dx), bf)
            report(f"dgamma[{tag}]", gw, dgam, agx)
            report(f"dbeta[{tag}]", gb, dbeta, ag)
        return
    y_int = y[:, :, pad_out:-pad_out, pad_out:-pad_out] if pad_out else y
    g, dx, dgam, dbeta, agx, ag = ref_bwd(c["dy"], xhat, invstd, gamma, y_int)
    for want_g in (False, True):
        out = ext.bn_bwd(c["dy"], x, gamma, sm, siv, elu_y=y, want_g=want_g,
                         pad_in=pad_out)
        assert len(out) == (4 if want_g else 3)
        t = f"{tag} want_g={int(want_g)}"
        report(f"dx[{t}]", out[0], dx, chan_max(dx), bf)
        report(f"dgamma[{t}]", out[1], dgam, agx)
        report(f"dbeta[{t}]", out[2], dbeta, ag)
        if want_g:
            assert tuple(out[3].shape) == (N, C, H, W)
            report(f"g[{t}]", out[3], g, chan_max(g), bf)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=_id)
@pytest.mark.parametrize("shape", EPI_SHAPES, ids=_id)
def test_epilogue_variants(shape, dtype):
    c = make_case(shape, dtype)
    for elu, rpad, pad_out in epilogue_combos():
        run_epilogue_combo(c, dtype, elu, rpad, pad_out)


# ------------------------------------------------------------- 4. eval mode

@pytest.mark.parametrize("dtype", [F32, BF16], ids=_id)
@pytest.mark.parametrize("shape", EVAL_SHAPES, ids=_id)
def test_eval_mode_random_running_stats(shape, dtype):
    ext = _ext()
    c = make_case(shape, dtype)
    rm, rv = c["rm0"].clone(), c["rv0"].clone()
    y, sm, siv = ext.bn_fwd(c["x"], c["gamma"], c["beta"], rm, rv, False,
                            0.1, EPS)
    torch.cuda.synchronize()
    assert torch.equal(rm, c["rm0"]) and torch.equal(rv, c["rv0"])
    assert torch.equal(sm, c["rm0"])
    rvd = c["rv0"].double()
    check("save_invstd", siv, 1.0 / torch.sqrt(rvd + EPS),
          1.0 / torch.sqrt(rvd + EPS))
    yref, _, _ = ref_fwd(c["x"], c["gamma"], c["beta"], c["rm0"].double(), rvd)
    # s_c carries the size of the normalised value, which in eval mode is
    # not O(1): |x - rm| * invstd can be several units
    s_y = _pc(c["gamma"].double().abs() + c["beta"].double().abs())
    check("y", y, yref, s_y, dtype == BF16)


# --------------------------------- 5. conditioning of the one-pass variance

COND_SHAPE = (8, 64, 16, 16)


def cond_depth():
    """Longest chain of fp32 additions a value passes through in
    bn_partials_kernel + bn_colsum_finalize_kernel at COND_SHAPE in fp32:
    32768 vectors on 128 blocks of 256 threads -> 1 add into the thread's
    accumulator, 256 / Cv = 16 adds in the block's LDS reduction, 128 / 64 =
    2 adds per lane in the column sum, 6 shuffle-tree adds."""
    N, C, H, W = COND_SHAPE
    nvec = N * H * W * C // 4
    nb = min((nvec + 255) // 256, 512)
    per_thread = -(-nvec // (nb * 256))
    return per_thread + 256 // (C // 4) + -(-nb // 64) + 6


def cond_errors(mu):
    g = torch.Generator(device="cuda").manual_seed(23)
    x = _cl(torch.randn(*COND_SHAPE, device="cuda", generator=g) * 0.25 + mu)
    C = COND_SHAPE[1]
    one = torch.ones(C, device="cuda")
    _, _, siv = _ext().bn_fwd(x, one, one * 0, one * 0, one.clone(), True,
                              0.1, EPS)
    mean, var, _ = ref_stats(x)
    want = 1.0 / torch.sqrt(var + EPS)
    r = mean.abs() / torch.sqrt(var)
    rel = (siv.double() - want).abs() / want
    return rel, r


@pytest.mark.parametrize("mu", [0.0, 2.0, 8.0])
def test_variance_conditioning(mu):
    """var = E[x^2] - mean^2 in fp32 loses about (1 + r^2) units of roundoff
    for r = |mean| / std: each of the two sums carries at most d * 2^-24
    relative error, d = cond_depth() = 25, and their difference is divided
    by a variance (1 + r^2) times smaller than E[x^2].  Bound, per channel:
    relerr(save_invstd) <= d * 2^-24 * (1 + r_c^2)."""
    d = cond_depth()
    assert d == 25
    rel, r = cond_errors(mu)
    bound = d * U32 * (1 + r * r)
    worst = (rel / bound).max().item()
    print(f"  mu={mu}: r up to {r.max().item():.2f}, max relerr "
          f"{rel.max().item():.3e}, bound {bound.max().item():.3e}, "
          f"worst err/bound {worst:.3f}")
    assert worst <= 1.0


# ------------------------------------------- 6. conv-epilogue BN statistics

# (xp shape, Kout, R, stride): the menu lives in tests/conv_menus.py, shared
# with the CPU planner test.
CONV_CASES = BN_CONV_CASES
WINDOW = {CONV_CASES[3], CONV_CASES[4]}


def conv_inputs(xshape, Kout, R):
    """Small-integer bf16 operands: every product and every fp32 partial sum
    of the convolution is then exact, so y does not depend on the order of
    accumulation and 'bit for bit' is a well-defined demand whichever tile
    size or split the plain forward picks.  Each output channel gets its
    own power-of-two gain so that channels differ in scale."""
    g = torch.Generator(device="cuda").manual_seed(31)
    xp = torch.randint(-3, 4, xshape, device="cuda", generator=g)
    w = torch.randint(-1, 2, (Kout, xshape[1], R, R), device="cuda",
                      generator=g)
    gain = 2.0 ** (torch.arange(Kout, device="cuda") % 4).float()
    w = w.float() * gain.view(-1, 1, 1, 1) / 8
    return _cl(xp.to(BF16)), _cl(w.to(BF16))


def conv_part_depth(M, tiles):
    """fp32 additions per value in the MODE-1 epilogue: (BM/2/16)*4 rows into
    the lane's accumulator, 2 xor-shuffle adds across the 4 lane groups, 1
    add joining the two waves of a column -> 19 at BM = 128, 11 at BM = 64.
    (The test itself sums the tile rows in float64.)"""
    bm = 64 if tiles == -(-M // 64) else 128
    return (bm // 2 // 16) * 4 + 2 + 1


def bn_own_depth(M, C, vec):
    """bn_partials_kernel + bn_colsum_finalize_kernel, as in cond_depth()."""
    nvec = M * C // vec
    nb = min(-(-nvec // 256), 512)
    return -(-nvec // (nb * 256)) + max(256 // (C // vec), 1) \
        + -(-nb // 64) + 6


@pytest.mark.parametrize("xshape,Kout,R,stride", CONV_CASES, ids=_id)
def test_conv_epilogue_stats(xshape, Kout, R, stride):
    ext = _ext()
    xp, w = conv_inputs(xshape, Kout, R)
    N = xshape[0]
    P = (xshape[2] - R) // stride + 1
    Q = (xshape[3] - R) // stride + 1
    M = N * P * Q
    is_window = (xshape, Kout, R, stride) in WINDOW
    if is_window:
        before = torch.full((Kout * 64 * 64,), 7.0, device="cuda")
    y, part = ext.conv2d_fwd_prepadded_bnstats(xp, w, stride)
    if is_window:
        # (d) canaries: weak alone, they back up check (a)
        after = torch.full((Kout * 64 * 64,), 9.0, device="cuda")
        torch.cuda.synchronize()
        assert (before == 7.0).all() and (after == 9.0).all()
    # (b) same y as the plain forward, bit for bit
    y_plain = ext.conv2d_fwd_prepadded(xp, w, stride)
    assert tuple(y.shape) == (N, Kout, P, Q)
    assert torch.equal(y, y_plain)
    assert torch.equal(xp, conv_inputs(xshape, Kout, R)[0])

    # (a) slab geometry and contents
    tiles = part.shape[1]
    assert tuple(part.shape) == (Kout // 64, tiles, 2, 64)
    assert tiles in (-(-M // 64), -(-M // 128)), (tiles, M)
    assert part.is_contiguous() and part.dtype == F32
    yd = y.double()
    s_want = yd.sum((0, 2, 3))
    q_want = (yd * yd).sum((0, 2, 3))
    s_abs = yd.abs().sum((0, 2, 3))
    tot = part.double().sum(1)                       # [Kout/64][2][64]
    s_got = tot[:, 0, :].reshape(-1)
    q_got = tot[:, 1, :].reshape(-1)
    d = conv_part_depth(M, tiles)
    assert d in (11, 19)
    es = ((s_got - s_want).abs() / (d * U32 * s_abs).clamp_min(1e-300)).max()
    eq = ((q_got - q_want).abs() / (d * U32 * q_want).clamp_min(1e-300)).max()
    print(f"  M={M} tiles={tiles} d={d}: sum err/bound {es.item():.3f}, "
          f"sumsq err/bound {eq.item():.3f}")
    assert es.item() <= 1.0 and eq.item() <= 1.0

    # (c) BN from the slab and BN's own reduction, against float64 statistics
    mean = s_want / M
    var = ((yd - _pc(mean)) ** 2).sum((0, 2, 3)) / M
    unb = var * M / (M - 1)
    invstd = 1.0 / torch.sqrt(var + EPS)
    r2 = mean * mean / var.clamp_min(1e-300)
    g = torch.Generator(device="cuda").manual_seed(37)
    gamma = torch.rand(Kout, device="cuda", generator=g) + 0.5
    beta = torch.randn(Kout, device="cuda", generator=g)
    rm0 = torch.randn(Kout, device="cuda", generator=g)
    rv0 = torch.rand(Kout, device="cuda", generator=g) + 0.5
    mom = 0.37
    # finalize from the slab adds ceil(tiles/64) + 6 more additions
    depths = {"conv_part": d + -(-tiles // 64) + 6,
              "own": bn_own_depth(M, Kout, 8)}
    for name, kw in (("conv_part", {"conv_part": part}), ("own", {})):
        rm, rv = rm0.clone(), rv0.clone()
        yb, sm, siv = ext.bn_fwd(y, gamma, beta, rm, rv, True, mom, EPS, **kw)
        dd = depths[name]
        e_mean = ((sm.double() - mean).abs()
                  / (dd * U32 * s_abs / M).clamp_min(1e-300)).max().item()
        # one-pass variance: (1 + r^2) units of roundoff, as in
        # test_variance_conditioning; eps only shrinks the relative error
        e_inv = ((siv.double() - invstd).abs() / invstd
                 / (dd * U32 * (1 + r2))).max().item()
        rm_want = (1 - mom) * rm0.double() + mom * mean
        rv_want = (1 - mom) * rv0.double() + mom * unb
        e_rm = ((rm.double() - rm_want).abs()
                / (U32 * rm_want.abs() + mom * dd * U32 * s_abs / M
                   + 2 * U32 * ((1 - mom) * rm0.double().abs()
                                + mom * mean.abs()))).max().item()
        e_rv = ((rv.double() - rv_want).abs()
                / (2 * mom * dd * U32 * (1 + r2) * unb
                   + 3 * U32 * rv_want)).max().item()
        print(f"  {name}: d={dd} mean {e_mean:.3f} invstd {e_inv:.3f} "
              f"running_mean {e_rm:.3f} running_var {e_rv:.3f} (err/bound)")
        assert max(e_mean, e_inv, e_rm, e_rv) <= 1.0, name
        yref, _, _ = ref_fwd(y, gamma, beta, mean, var)
        s_y = _pc(gamma.double().abs() + beta.double().abs())
        check(f"bn y [{name}]", yb, yref, s_y, True)


# -------------------------------------- 7. FEDKIT_CONV_BNSTATS end to end

def test_conv_bnstats_switch_end_to_end(monkeypatch):
    import copy

    import fedkit.ops.norm as norm
    from fedkit.ops import FedBatchNorm2d, FedConv2d

    torch.manual_seed(41)
    conv0 = FedConv2d(64, 64, 3, padding=1, bias=False).cuda().train()
    bn0 = FedBatchNorm2d(64).cuda().train()
    with torch.no_grad():
        bn0.weight.uniform_(0.5, 1.5)
        bn0.bias.normal_()
    x0 = _cl(torch.randn(32, 64, 32, 32, device="cuda"))
    gy = _cl(torch.randn(32, 64, 32, 32, device="cuda").to(BF16))

    real_ext = norm._ext()
    seen = []

    class Spy:
        def __getattr__(self, name):
            return getattr(real_ext, name)

        def bn_fwd(self, *a, **kw):
            seen.append(kw.get("conv_part"))
            return real_ext.bn_fwd(*a, **kw)

    monkeypatch.setattr(norm, "_ext", lambda: Spy())

    def run(flag):
        if flag:
            monkeypatch.setenv("FEDKIT_CONV_BNSTATS", "1")
        else:
            monkeypatch.delenv("FEDKIT_CONV_BNSTATS", raising=False)
        conv, bn = copy.deepcopy(conv0), copy.deepcopy(bn0)
        x = x0.clone().requires_grad_(True)
        with torch.autocast(device_type="cuda", dtype=BF16):
            h = conv(x)
            stats = getattr(h, "_fedkit_bn_stats", None)
            y = norm.bn_elu(bn, h)
        y.backward(gy)
        return dict(y=y.detach(), dx=x.grad, dw=conv.weight.grad,
                    dgamma=bn.weight.grad, dbeta=bn.bias.grad,
                    rm=bn.running_mean, rv=bn.running_var), stats

    off, stats_off = run(False)
    assert stats_off is None and seen == [None]
    on, stats_on = run(True)
    # the conv attached its partials and bn_fwd consumed exactly those
    assert stats_on is not None and stats_on.shape[0] == 1 \
        and tuple(stats_on.shape[2:]) == (2, 64)
    assert len(seen) == 2 and seen[1] is not None \
        and seen[1].data_ptr() == stats_on.data_ptr()

    # Both runs are within the bf16 tolerance of the exact result, so they
    # are within twice that of each other.
    def close(name, a, b, scale, bf):
        got, want = a.double(), b.double()
        allowed = 2 * (TOL32 * (want.abs() + scale)
                       + (half_ulp_bf16(torch.maximum(want.abs(), got.abs()))
                          if bf else 0))
        ratio = torch.nan_to_num((got - want).abs() / allowed.clamp_min(1e-300),
                                 nan=float("inf")).max().item()
        print(f"  {name}: {ratio:.3f} of the allowed difference")
        assert ratio <= 1.0, name

    s_y = _pc(bn0.weight.double().abs() + bn0.bias.double().abs())
    close("y", on["y"], off["y"], s_y, True)
    close("running_mean", on["rm"], off["rm"], off["rm"].double().abs(), False)
    close("running_var", on["rv"], off["rv"], off["rv"].double().abs(), False)
    # gradients: sums of bf16-rounded terms, the rounding term takes the
    # scale of the sum's terms (per-channel / per-tensor max), not of the sum
    for k in ("dx", "dw", "dgamma", "dbeta"):
        want = off[k].double()
        scale = chan_max(want) if want.dim() == 4 else want.abs().max()
        got = on[k].double()
        allowed = 2 * (TOL32 * (want.abs() + scale)
                       + half_ulp_bf16(want.abs() + scale))
        ratio = torch.nan_to_num((got - want).abs() / allowed,
                                 nan=float("inf")).max().item()
        print(f"  {k}: {ratio:.3f} of the allowed difference")
        assert ratio <= 1.0, k
