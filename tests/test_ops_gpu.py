"""GPU numerics tests: every HIP kernel vs a plain torch fp32 reference of
the same op (SURVEY.md §4 test plan).  All marked @pytest.mark.gpu."""

import pytest
import torch
import torch.nn.functional as F

from conv_menus import BANK_CASES, GEN_N, RESNET_SHAPES, VAE_CPC_CONVS

pytestmark = pytest.mark.gpu


def _ext():
    import fedkit.ops
    assert fedkit.ops.has_ext(), "fedkit._C must be built on a GPU box"
    return fedkit.ops.ext()


def rel_err(got, want):
    got = got.float()
    want = want.float()
    denom = want.abs().max().clamp_min(1e-6)
    return (got - want).abs().max().item() / denom.item()


def frob_err(got, want):
    got = got.float()
    want = want.float()
    return ((got - want).norm() / want.norm().clamp_min(1e-12)).item()


# ----------------------------------------------------------------- elementwise

@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_elu_fwd_bwd(dtype):
    ext = _ext()
    torch.manual_seed(0)
    x = torch.randn(3, 64, 17, 31, device="cuda", dtype=dtype)
    y = ext.elu_fwd(x)
    want = F.elu(x.float())
    tol = 1e-6 if dtype == torch.float32 else 1e-2
    assert rel_err(y, want) < tol
    gy = torch.randn_like(x)
    gx = ext.elu_bwd(gy, y)
    xref = x.float().detach().requires_grad_(True)
    F.elu(xref).backward(gy.float())
    assert rel_err(gx, xref.grad) < (1e-5 if dtype == torch.float32 else 2e-2)


def test_elu_channels_last_no_copy():
    ext = _ext()
    x = torch.randn(2, 64, 8, 8, device="cuda").contiguous(
        memory_format=torch.channels_last)
    y = ext.elu_fwd(x)
    assert y.is_contiguous(memory_format=torch.channels_last)
    assert rel_err(y, F.elu(x)) < 1e-6


# -------------------------------------------------------------------- flat ops

def test_pack_unpack_axpy_gpu():
    ext = _ext()
    torch.manual_seed(1)
    ts = [torch.randn(s, device="cuda") for s in
          [(64, 3, 3, 3), (64,), (11,), (512, 256), (1,)]]
    n = sum(t.numel() for t in ts)
    flat = torch.empty(n, device="cuda")
    ext.pack_params(ts, flat)
    want = torch.cat([t.reshape(-1) for t in ts])
    assert torch.equal(flat, want)
    outs = [torch.zeros_like(t) for t in ts]
    ext.unpack_params(flat, outs)
    for a, b in zip(ts, outs):
        assert torch.equal(a, b)
    upd = torch.randn(n, device="cuda")
    ref = [t.clone() for t in ts]
    ext.add_flat_params(ts, upd, 0.3)
    off = 0
    for t, r in zip(ts, ref):
        k = r.numel()
        assert torch.allclose(t, r + 0.3 * upd[off:off + k].view_as(r),
                              atol=1e-6)
        off += k


def test_pack_many_tensors_chunking():
    """More than one 48-tensor descriptor chunk (ResNet18 has 62 tensors)."""
    ext = _ext()
    ts = [torch.randn(7, device="cuda") for _ in range(130)]
    flat = torch.empty(7 * 130, device="cuda")
    ext.pack_params(ts, flat)
    assert torch.equal(flat, torch.cat(ts))


def _cast_sources():
    """Numels around the 8-wide cast unit — units start in one tensor and
    end in another, the last unit is a tail — plus a channels_last 4-D."""
    torch.manual_seed(5)
    ts = [torch.randn(n, device="cuda") for n in (0, 1, 7, 8, 9, 15, 16, 17)]
    ts.append(torch.randn(8, 3, 3, 3, device="cuda").contiguous(
        memory_format=torch.channels_last))
    return ts


def _check_cast_roundtrip(ext, srcs):
    lo = [torch.zeros_like(s, dtype=torch.bfloat16) for s in srcs]
    ext.cast_f32_to_bf16(srcs, lo)
    for s, d in zip(srcs, lo):
        assert d.stride() == s.stride()
        assert torch.equal(d, s.to(torch.bfloat16))
    hi = [torch.zeros_like(d, dtype=torch.float32) for d in lo]
    ext.cast_bf16_to_f32(lo, hi)
    for d, h in zip(lo, hi):
        assert h.stride() == d.stride()
        assert torch.equal(h, d.float())


def test_batched_casts_direct():
    _check_cast_roundtrip(_ext(), _cast_sources())


def test_batched_casts_past_one_table():
    """50 tensors: two 48-tensor tables, one launch each."""
    torch.manual_seed(6)
    _check_cast_roundtrip(
        _ext(), [torch.randn(7, device="cuda") for _ in range(50)])


def _assert_rejected_untouched(fn, outputs):
    """fn must raise before any launch: outputs stay bit-unchanged."""
    before = [t.clone() for t in outputs]
    with pytest.raises(RuntimeError):
        fn()
    torch.cuda.synchronize()
    for t, b in zip(outputs, before):
        assert t.dtype == b.dtype and torch.equal(t, b)


@pytest.mark.parametrize("flat_kind", ["short", "cpu"])
@pytest.mark.parametrize("op", ["pack", "unpack", "axpy"])
def test_flat_ops_reject_bad_flat_before_launch(op, flat_kind):
    ext = _ext()
    torch.manual_seed(7)
    ts = [torch.randn(n, device="cuda") for n in (5, 8, 3)]
    flat = torch.randn(15 if flat_kind == "short" else 16,
                       device="cuda" if flat_kind == "short" else "cpu")
    call = {"pack": lambda: ext.pack_params(ts, flat),
            "unpack": lambda: ext.unpack_params(flat, ts),
            "axpy": lambda: ext.add_flat_params(ts, flat, 0.5)}[op]
    _assert_rejected_untouched(call, ts + [flat])


def test_add_flat_rejects_late_bad_dtype_before_launch():
    """The bad tensor sits in the second table; the first 48 stay put."""
    ext = _ext()
    torch.manual_seed(8)
    ts = [torch.randn(7, device="cuda") for _ in range(49)]
    ts.append(torch.randn(7, device="cuda").half())
    flat = torch.randn(7 * 50, device="cuda")
    _assert_rejected_untouched(
        lambda: ext.add_flat_params(ts, flat, 0.5), ts)


@pytest.mark.parametrize("case", ["src_dtype", "numel", "layout"])
def test_cast_rejects_mismatch_before_launch(case):
    ext = _ext()
    torch.manual_seed(9)
    src = torch.randn(8, 3, 3, 3, device="cuda")
    if case == "src_dtype":
        src = src.to(torch.bfloat16)
        dst = torch.zeros_like(src)
    elif case == "numel":
        dst = torch.zeros(8, 3, 3, 2, device="cuda", dtype=torch.bfloat16)
    else:
        src = src.contiguous(memory_format=torch.channels_last)
        dst = torch.zeros(8, 3, 3, 3, device="cuda", dtype=torch.bfloat16)
        assert dst.stride() != src.stride()
    good = torch.randn(9, device="cuda")
    good_dst = torch.zeros(9, device="cuda", dtype=torch.bfloat16)
    _assert_rejected_untouched(
        lambda: ext.cast_f32_to_bf16([good, src], [good_dst, dst]),
        [good_dst, dst])


# ----------------------------------------------------------------------- loss

@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_cross_entropy(dtype):
    ext = _ext()
    torch.manual_seed(2)
    logits = torch.randn(128, 10, device="cuda", dtype=dtype)
    labels = torch.randint(0, 10, (128,), device="cuda")
    loss, lse = ext.cross_entropy_fwd(logits, labels)
    want = F.cross_entropy(logits.float(), labels)
    assert abs(loss.item() - want.item()) < (1e-5 if dtype == torch.float32 else 5e-3)
    g = torch.ones((), device="cuda")
    gx = ext.cross_entropy_bwd(logits, labels, lse, g)
    ref = logits.float().detach().requires_grad_(True)
    F.cross_entropy(ref, labels).backward()
    assert rel_err(gx, ref.grad) < (1e-4 if dtype == torch.float32 else 2e-2)


# ------------------------------------------------------------------ batchnorm

@pytest.mark.parametrize("C", [64, 128, 256, 512])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_bn_fwd_bwd_vs_torch(C, dtype):
    ext = _ext()
    torch.manual_seed(3)
    N, H, W = 8, 9, 9
    x = (torch.randn(N, C, H, W, device="cuda") * 2 + 0.5).to(dtype)
    x = x.contiguous(memory_format=torch.channels_last)
    gamma = torch.rand(C, device="cuda") + 0.5
    beta = torch.randn(C, device="cuda")
    rm = torch.zeros(C, device="cuda")
    rv = torch.ones(C, device="cuda")
    y, sm, siv = ext.bn_fwd(x, gamma, beta, rm, rv, True, 0.1, 1e-5)

    xf = x.float().detach().requires_grad_(True)
    rm_ref = torch.zeros(C, device="cuda")
    rv_ref = torch.ones(C, device="cuda")
    gref = gamma.detach().requires_grad_(True)
    bref = beta.detach().requires_grad_(True)
    yref = F.batch_norm(xf, rm_ref, rv_ref, gref, bref, True, 0.1, 1e-5)
    tol = 1e-4 if dtype == torch.float32 else 3e-2
    assert rel_err(y, yref) < tol
    assert rel_err(rm, rm_ref) < 1e-3
    assert rel_err(rv, rv_ref) < 1e-3

    gy = torch.randn_like(x)
    gx, gw, gb = ext.bn_bwd(gy, x, gamma, sm, siv)
    yref.backward(gy.float())
    assert rel_err(gb, bref.grad) < (1e-3 if dtype == torch.float32 else 3e-2)
    assert rel_err(gw, gref.grad) < (1e-3 if dtype == torch.float32 else 3e-2)
    assert rel_err(gx, xf.grad) < (1e-3 if dtype == torch.float32 else 5e-2)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("with_res", [False, True])
def test_bn_fused_elu_residual(dtype, with_res):
    """bn_fwd(residual=..., elu=True) == elu(batch_norm(x) + residual)."""
    ext = _ext()
    torch.manual_seed(5)
    C = 128
    x = (torch.randn(8, C, 9, 9, device="cuda")).to(dtype)
    x = x.contiguous(memory_format=torch.channels_last)
    res = torch.randn_like(x) if with_res else None
    gamma = torch.rand(C, device="cuda") + 0.5
    beta = torch.randn(C, device="cuda")
    rm = torch.zeros(C, device="cuda")
    rv = torch.ones(C, device="cuda")
    y, _, _ = ext.bn_fwd(x, gamma, beta, rm, rv, True, 0.1, 1e-5,
                         residual=res, elu=True)
    yref = F.batch_norm(x.float(), torch.zeros(C, device="cuda"),
                        torch.ones(C, device="cuda"), gamma, beta,
                        True, 0.1, 1e-5)
    if with_res:
        yref = yref + res.float()
    yref = F.elu(yref)
    assert rel_err(y, yref) < (1e-4 if dtype == torch.float32 else 3e-2)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_bn_elu_autograd_vs_composed(dtype):
    """fedkit.ops.norm.bn_elu fwd+bwd == composed BN/add/ELU autograd."""
    from fedkit.ops.norm import FedBatchNorm2d, bn_elu
    torch.manual_seed(6)
    C = 64
    bn = FedBatchNorm2d(C).cuda().train()
    x = torch.randn(8, C, 9, 9, device="cuda", dtype=dtype,
                    requires_grad=True)
    res = torch.randn_like(x, requires_grad=True)
    xcl = x.detach().clone().requires_grad_(True)
    rescl = res.detach().clone().requires_grad_(True)
    y = bn_elu(bn, x.contiguous(memory_format=torch.channels_last),
               residual=res)
    gy = torch.randn_like(y)
    y.backward(gy)

    bn2 = FedBatchNorm2d(C).cuda().train()
    yref = F.elu(F.batch_norm(xcl.float(), bn2.running_mean, bn2.running_var,
                              bn2.weight, bn2.bias, True, 0.1, 1e-5)
                 + rescl.float())
    yref.backward(gy.float())
    tol = 1e-3 if dtype == torch.float32 else 5e-2
    assert rel_err(y, yref) < tol
    assert rel_err(x.grad, xcl.grad) < tol
    assert rel_err(res.grad, rescl.grad) < tol
    assert rel_err(bn.weight.grad, bn2.weight.grad) < tol


def test_bn_eval_mode():
    ext = _ext()
    C = 64
    x = torch.randn(4, C, 8, 8, device="cuda").contiguous(
        memory_format=torch.channels_last)
    gamma = torch.rand(C, device="cuda") + 0.5
    beta = torch.randn(C, device="cuda")
    rm = torch.randn(C, device="cuda")
    rv = torch.rand(C, device="cuda") + 0.5
    y, _, _ = ext.bn_fwd(x, gamma, beta, rm.clone(), rv.clone(), False, 0.1, 1e-5)
    yref = F.batch_norm(x, rm, rv, gamma, beta, False, 0.1, 1e-5)
    assert rel_err(y, yref) < 1e-4


# ----------------------------------------------------------------------- conv

# shape menus: tests/conv_menus.py (shared with the CPU planner test, which
# checks that they reach every instantiated conv kernel)

@pytest.mark.parametrize("N,C,H,K,R,stride", RESNET_SHAPES)
def test_conv_fwd_vs_torch(N, C, H, K, R, stride):
    ext = _ext()
    torch.manual_seed(4)
    pad = 1 if R == 3 else 0
    x = torch.randn(N, C, H, H, device="cuda", dtype=torch.bfloat16)
    w = torch.randn(K, C, R, R, device="cuda", dtype=torch.bfloat16) * 0.05
    xc = x.contiguous(memory_format=torch.channels_last)
    wc = w.contiguous(memory_format=torch.channels_last)
    y = ext.conv2d_fwd(xc, wc, stride, pad)
    want = F.conv2d(x.float(), w.float(), None, stride, pad)
    assert y.shape == want.shape
    assert frob_err(y, want) < 1.5e-2, f"fwd mismatch {frob_err(y, want)}"


@pytest.mark.parametrize("N,C,H,K,R,stride", RESNET_SHAPES)
def test_conv_bwd_data_vs_torch(N, C, H, K, R, stride):
    ext = _ext()
    torch.manual_seed(5)
    pad = 1 if R == 3 else 0
    P = (H + 2 * pad - R) // stride + 1
    gy = torch.randn(N, K, P, P, device="cuda", dtype=torch.bfloat16)
    w = torch.randn(K, C, R, R, device="cuda", dtype=torch.bfloat16) * 0.05
    gyc = gy.contiguous(memory_format=torch.channels_last)
    wc = w.contiguous(memory_format=torch.channels_last)
    gx = ext.conv2d_bwd_data(gyc, wc, stride, pad, H, H)
    xref = torch.zeros(N, C, H, H, device="cuda", requires_grad=True)
    F.conv2d(xref, w.float(), None, stride, pad).backward(gy.float())
    assert gx.shape == xref.grad.shape
    assert frob_err(gx, xref.grad) < 1.5e-2


@pytest.mark.parametrize("N,C,H,K,R,stride", RESNET_SHAPES)
def test_conv_bwd_weight_vs_torch(N, C, H, K, R, stride):
    ext = _ext()
    torch.manual_seed(6)
    pad = 1 if R == 3 else 0
    P = (H + 2 * pad - R) // stride + 1
    x = torch.randn(N, C, H, H, device="cuda", dtype=torch.bfloat16)
    gy = torch.randn(N, K, P, P, device="cuda", dtype=torch.bfloat16)
    xc = x.contiguous(memory_format=torch.channels_last)
    gyc = gy.contiguous(memory_format=torch.channels_last)
    gw = ext.conv2d_bwd_weight(gyc, xc, stride, pad, R, R)
    wref = torch.zeros(K, C, R, R, device="cuda", requires_grad=True)
    F.conv2d(x.float(), wref, None, stride, pad).backward(gy.float())
    assert gw.shape == wref.grad.shape
    assert frob_err(gw, wref.grad) < 1.5e-2


def test_conv_small_c3():
    """ResNet conv1: C=3 direct kernel."""
    ext = _ext()
    torch.manual_seed(7)
    x = torch.randn(8, 3, 32, 32, device="cuda", dtype=torch.bfloat16)
    w = torch.randn(64, 3, 3, 3, device="cuda", dtype=torch.bfloat16) * 0.2
    y = ext.conv2d_fwd(x.contiguous(memory_format=torch.channels_last),
                       w.contiguous(memory_format=torch.channels_last), 1, 1)
    want = F.conv2d(x.float(), w.float(), None, 1, 1)
    assert frob_err(y, want) < 1.5e-2


def test_conv_identity_transpose_detecting():
    """Asymmetric-B check (guide G9): catches swapped MFMA operand layouts."""
    ext = _ext()
    C, K = 64, 64
    x = torch.zeros(2, C, 8, 8, device="cuda", dtype=torch.bfloat16)
    # delta input at a single (pixel, channel)
    x[0, 5, 3, 4] = 1.0
    w = torch.arange(K * C, device="cuda", dtype=torch.float32).reshape(K, C, 1, 1)
    w = (w / (K * C)).to(torch.bfloat16)
    y = ext.conv2d_fwd(x.contiguous(memory_format=torch.channels_last),
                       w.contiguous(memory_format=torch.channels_last), 1, 0)
    want = F.conv2d(x.float(), w.float(), None, 1, 0)
    assert frob_err(y, want) < 1e-2


# ----------------------------------------------------------- module-level path

def test_fedconv_module_autograd():
    from fedkit.ops import FedConv2d
    torch.manual_seed(8)
    m = FedConv2d(64, 128, 3, stride=2, padding=1, bias=False).cuda()
    m = m.to(memory_format=torch.channels_last)
    x = torch.randn(4, 64, 16, 16, device="cuda", dtype=torch.bfloat16)
    x = x.contiguous(memory_format=torch.channels_last).requires_grad_(True)
    y = m(x)
    loss = y.float().square().mean()
    loss.backward()
    assert m.weight.grad is not None
    assert x.grad is not None
    # fp32 reference
    xr = x.detach().float().requires_grad_(True)
    yr = F.conv2d(xr, m.weight.detach().float(), None, 2, 1)
    yr.square().mean().backward()
    assert frob_err(y, yr) < 2e-2
    assert frob_err(x.grad, xr.grad) < 5e-2


def test_resnet18_training_step_bf16():
    """Whole-model smoke: one fwd+bwd+Adam step through the HIP kernels."""
    from fedkit.models import ResNet18
    from fedkit.ops import losses as L
    torch.manual_seed(9)
    net = ResNet18().cuda().to(memory_format=torch.channels_last)
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    x = torch.randn(32, 3, 32, 32, device="cuda").contiguous(
        memory_format=torch.channels_last)
    y = torch.randint(0, 10, (32,), device="cuda")
    with torch.autocast(device_type="cuda", dtype=torch.bfloat16):
        loss = L.cross_entropy(net(x), y)
    opt.zero_grad()
    loss.backward()
    opt.step()
    torch.cuda.synchronize()
    assert torch.isfinite(loss)
    for p in net.parameters():
        assert torch.isfinite(p).all()


# ------------------------------------------------------- generic conv (VAE/CPC)

@pytest.mark.parametrize("Cin,Kout,H,ks,stride,pad,dil", VAE_CPC_CONVS)
def test_gen_conv_fwd_bwd_vs_torch(Cin, Kout, H, ks, stride, pad, dil):
    from fedkit.ops.conv import _gen_conv
    torch.manual_seed(11)
    N = GEN_N
    x = (torch.randn(N, Cin, H, H, device="cuda") * 0.5).requires_grad_(True)
    w = (torch.randn(Kout, Cin, ks, ks, device="cuda") * 0.1).requires_grad_(True)
    b = torch.randn(Kout, device="cuda", requires_grad=True)
    y = _gen_conv(x.to(torch.bfloat16).contiguous(
        memory_format=torch.channels_last), w, b, stride, pad, dil)
    want = F.conv2d(x, w, b, stride, pad, dil)
    assert y.shape == want.shape, (y.shape, want.shape)
    assert frob_err(y.float(), want) < 2e-2
    gy = torch.randn_like(want)
    y.backward(gy.to(y.dtype))
    gxr, gwr, gbr = torch.autograd.grad(want, [x, w, b], gy)
    assert frob_err(w.grad.float(), gwr) < 2e-2
    assert frob_err(b.grad.float(), gbr) < 2e-2
    assert frob_err(x.grad.float(), gxr) < 2e-2


@pytest.mark.parametrize("Cin,Kout,H", [(96, 48, 2), (48, 24, 4),
                                        (24, 12, 8), (12, 3, 16)])
def test_conv_transpose_vs_torch(Cin, Kout, H):
    """FedConvTranspose2d (VAE decoder 4x4-s2, simple_models.py:262-265)."""
    from fedkit.ops.conv import FedConvTranspose2d
    torch.manual_seed(12)
    mod = FedConvTranspose2d(Cin, Kout, 4, stride=2, padding=1).cuda()
    x = (torch.randn(16, Cin, H, H, device="cuda") * 0.5).requires_grad_(True)
    y = mod(x.to(torch.bfloat16).contiguous(
        memory_format=torch.channels_last))
    want = F.conv_transpose2d(x, mod.weight, mod.bias, 2, 1)
    assert y.shape == want.shape
    assert frob_err(y.float(), want) < 2e-2
    gy = torch.randn_like(want)
    y.backward(gy.to(y.dtype))
    gxr, gwr = torch.autograd.grad(want, [x, mod.weight], gy,
                                   retain_graph=False)
    assert frob_err(x.grad.float(), gxr) < 2e-2
    assert frob_err(mod.weight.grad.float(), gwr) < 2e-2


def test_vae_model_gpu_step():
    """AutoEncoderCNN forward+backward end-to-end on the generic conv path."""
    from fedkit.models import AutoEncoderCNN
    from fedkit.ops.losses import vae_loss
    torch.manual_seed(13)
    net = AutoEncoderCNN().cuda()
    x = torch.rand(32, 3, 32, 32, device="cuda")
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out, mu, logvar = net(x)
        loss = vae_loss(out.float(), x, mu.float(), logvar.float())
    loss.backward()
    assert torch.isfinite(loss)
    for p in net.parameters():
        assert p.grad is None or torch.isfinite(p.grad).all()


# ---------------------------------------------------------- fused L-BFGS ops

def test_multi_dot_lincomb_vs_torch():
    from fedkit.ops import flat as flat_ops
    torch.manual_seed(20)
    N = 1000003
    x = torch.randn(N, device="cuda")
    vecs = [torch.randn(N, device="cuda") for _ in range(9)]
    got = flat_ops.multi_dot(vecs, x).cpu()
    want = torch.stack([torch.dot(v, x) for v in vecs]).cpu()
    assert torch.allclose(got, want, rtol=1e-4, atol=1e-2), (got, want)
    coeffs = [0.1 * (i - 4) for i in range(9)]
    lc = flat_ops.lincomb(x, -0.5, vecs, coeffs)
    ref = -0.5 * x + sum(c * v for c, v in zip(coeffs, vecs))
    assert frob_err(lc, ref) < 1e-6


def test_lbfgs_two_loop_fused_matches_reference():
    """Gram-matrix two-loop == the reference serial two-loop."""
    from fedkit.optim.lbfgsnew import LBFGSNew
    torch.manual_seed(21)
    N = 100003
    p = torch.nn.Parameter(torch.zeros(N, device="cuda"))
    opt = LBFGSNew([p], history_size=7)
    g = torch.randn(N, device="cuda")
    hist_s = [torch.randn(N, device="cuda") for _ in range(5)]
    # make curvature pairs positive-definite-ish: y = 2s + noise
    hist_y = [2.0 * s_ + 0.1 * torch.randn(N, device="cuda") for s_ in hist_s]
    SY = [[float(s_.dot(y_)) for y_ in hist_y] for s_ in hist_s]
    YY = [[float(a.dot(b)) for b in hist_y] for a in hist_y]
    H = 0.37
    d_ref = opt._two_loop(g, list(hist_y), list(hist_s), H,
                          [None] * 7, [None] * 7)
    d_fused = opt._two_loop_fused(g, hist_y, hist_s, H, SY, YY)
    assert frob_err(d_fused, d_ref) < 1e-4


def test_lbfgs_gpu_quadratic_converges():
    """LBFGSNew full path (fused dots + cubic Wolfe) on a convex quadratic."""
    from fedkit.optim.lbfgsnew import LBFGSNew
    torch.manual_seed(22)
    n = 2000
    A = torch.randn(n, n, device="cuda") / n ** 0.5
    Q = A @ A.t() + 0.1 * torch.eye(n, device="cuda")
    b = torch.randn(n, device="cuda")
    x = torch.nn.Parameter(torch.zeros(n, device="cuda"))
    opt = LBFGSNew([x], history_size=10, max_iter=10, line_search_fn=True)

    def closure():
        opt.zero_grad()
        loss = 0.5 * x @ Q @ x - b @ x
        if torch.is_grad_enabled():
            loss.backward()
        return loss

    for _ in range(15):
        opt.step(closure)
    xstar = torch.linalg.solve(Q, b)
    rel = (x.detach() - xstar).norm() / xstar.norm()
    assert rel < 1e-2, float(rel)


# ------------------------------------------------------------------- pooling

@pytest.mark.parametrize("C,H,k", [(64, 32, 2), (16, 8, 2), (512, 4, 4),
                                   (96, 16, 2)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_pool_fwd_bwd_vs_torch(C, H, k, dtype):
    from fedkit.ops.pool import max_pool2d, avg_pool2d
    torch.manual_seed(31)
    x = torch.randn(8, C, H, H, device="cuda", dtype=dtype,
                    requires_grad=True)
    for fed, ref in ((max_pool2d, F.max_pool2d), (avg_pool2d, F.avg_pool2d)):
        y = fed(x, k)
        want = ref(x.float(), k)
        assert y.shape == want.shape
        assert frob_err(y.float(), want) < 1e-2
        gy = torch.randn_like(want)
        gx, = torch.autograd.grad(y, x, gy.to(y.dtype), retain_graph=False)
        gxr, = torch.autograd.grad(want, x, gy, retain_graph=False)
        assert frob_err(gx.float(), gxr.float()) < 1e-2


# ------------------------------------------------- driver-level GPU smokes

def _smoke_cfg(**kw):
    from fedkit.parallel import FedConfig
    return FedConfig(K=2, default_batch=32, Nloop=1, Nepoch=1, Nadmm=1,
                     check_results=False, save_model=False, use_cuda=True,
                     max_steps_per_epoch=2, be_verbose=False, **kw)


def test_vae_job_gpu_smoke():
    """federated_vae path: AutoEncoderCNN + vae_loss on the generic convs."""
    from fedkit.parallel import FederatedJob
    from fedkit.ops.losses import vae_loss

    def loss_fn(net, images, _labels):
        out, mu, logvar = net(images)
        return vae_loss(out.float(), images.float(), mu.float(),
                        logvar.float())

    job = FederatedJob(_smoke_cfg(model="AutoEncoderCNN", strategy="fedavg",
                                  per_layer=True), loss_fn=loss_fn)
    job.run()
    for ck in job.comm.my_clients:
        for p in job.nets[ck].parameters():
            assert torch.isfinite(p).all()


def test_vae_cl_job_gpu_smoke():
    """federated_vae_cl path: clustering VAE with the 4-term ELBO."""
    from fedkit.parallel import FederatedJob
    from fedkit.ops.losses import vaecl_loss

    def loss_fn(net, images, _labels):
        ekhat, mu_xi, sig2_xi, mu_b, sig2_b, mu_th, sig2_th = net(images)
        return vaecl_loss(ekhat, mu_xi, sig2_xi, mu_b, sig2_b, mu_th,
                          sig2_th, images)

    job = FederatedJob(_smoke_cfg(model="AutoEncoderCNNCL",
                                  strategy="fedavg"), loss_fn=loss_fn)
    job.run()
    for ck in job.comm.my_clients:
        for p in job.nets[ck].parameters():
            assert torch.isfinite(p).all()


def test_cpc_models_gpu_smoke():
    """CPC encoder/contextgen/predictor + InfoNCE end-to-end on GPU."""
    from fedkit.models import EncoderCNN, ContextgenCNN, PredictorCNN
    from fedkit.ops.losses import info_nce
    torch.manual_seed(33)
    enc = EncoderCNN().cuda()
    ctx = ContextgenCNN().cuda()
    prd = PredictorCNN().cuda()
    ybatch = torch.randn(9, 8, 32, 32, device="cuda")
    with torch.autocast("cuda", dtype=torch.bfloat16):
        lat = enc(ybatch)                      # [9, latent]
        grid = lat.t().reshape(1, -1, 3, 3)    # [1, latent, px, py]
        c = ctx(grid)
        zhat, z = prd(grid, c)
        loss = info_nce(z.float(), zhat.float())
    loss.backward()
    assert torch.isfinite(loss)


# ---------------------------------------- full-model composition numerics

def test_resnet18_gpu_end_to_end_vs_eager():
    """Whole ResNet18 fwd+bwd on the native kernels vs the same weights on
    stock fp32 torch ops — catches composition bugs the per-op tests miss
    (layout handoffs, fused BN/ELU boundaries, pooling, weight pre-cast)."""
    import fedkit.ops as ops
    from fedkit.models import ResNet18
    torch.manual_seed(41)
    net = ResNet18().cuda().to(memory_format=torch.channels_last)
    x = torch.randn(16, 3, 32, 32, device="cuda").contiguous(
        memory_format=torch.channels_last)
    yt = torch.randint(0, 10, (16,), device="cuda")

    with torch.autocast("cuda", dtype=torch.bfloat16):
        logits = net(x)
        loss = F.cross_entropy(logits.float(), yt)
    loss.backward()
    nat_logits = logits.float().detach().clone()
    nat_grads = torch.cat([p.grad.detach().float().reshape(-1)
                           for p in net.parameters() if p.grad is not None])
    net.zero_grad(set_to_none=True)

    old = ops._NATIVE_ENV
    ops._NATIVE_ENV = False
    try:
        logits2 = net(x)                   # stock fp32 ops, same weights
        loss2 = F.cross_entropy(logits2, yt)
        loss2.backward()
    finally:
        ops._NATIVE_ENV = old
    ref_logits = logits2.float().detach()
    ref_grads = torch.cat([p.grad.detach().float().reshape(-1)
                           for p in net.parameters() if p.grad is not None])

    assert frob_err(nat_logits, ref_logits) < 3e-2, \
        frob_err(nat_logits, ref_logits)
    assert frob_err(nat_grads, ref_grads) < 6e-2, \
        frob_err(nat_grads, ref_grads)


@pytest.mark.parametrize("name", ["Net", "Net1", "Net2"])
def test_classifier_models_gpu_vs_eager(name):
    """Net/Net1/Net2 fwd+bwd numerics on the native kernels vs the same
    weights on stock fp32 ops.  The 5x5 / valid-3x3 convs run the MFMA
    generic path via the Kg-tail zero fill (Kg = 200 / 72 / 288), so this
    is a real numerics check of the comparison.png model family
    (VERDICT r1 #3, weak #5)."""
    import fedkit.ops as ops
    import fedkit.models as M
    torch.manual_seed(51)
    net = getattr(M, name)().cuda()
    x = torch.randn(32, 3, 32, 32, device="cuda")
    yt = torch.randint(0, 10, (32,), device="cuda")
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out = net(x)
        loss = F.cross_entropy(out.float(), yt)
    loss.backward()
    nat_logits = out.float().detach().clone()
    nat_grads = torch.cat([p.grad.detach().float().reshape(-1)
                           for p in net.parameters() if p.grad is not None])
    net.zero_grad(set_to_none=True)
    old = ops._NATIVE_ENV
    ops._NATIVE_ENV = False
    try:
        out2 = net(x)
        loss2 = F.cross_entropy(out2, yt)
        loss2.backward()
    finally:
        ops._NATIVE_ENV = old
    ref_logits = out2.float().detach()
    ref_grads = torch.cat([p.grad.detach().float().reshape(-1)
                           for p in net.parameters() if p.grad is not None])
    assert frob_err(nat_logits, ref_logits) < 3e-2, \
        frob_err(nat_logits, ref_logits)
    assert frob_err(nat_grads, ref_grads) < 6e-2, \
        frob_err(nat_grads, ref_grads)


@pytest.mark.parametrize("shape", [
    # (C, K, R, pad, H): Kg = R*R*pad8(C) % 64 != 0 tail cases
    (3, 6, 5, 0, 32),     # Net conv1, Kg=200
    (6, 16, 5, 0, 14),    # Net conv2, Kg=200
    (3, 32, 3, 0, 32),    # Net1 conv1, Kg=72
    (32, 32, 3, 0, 30),   # Net1 conv2, Kg=288
    (32, 64, 3, 0, 14),   # Net1 conv3, Kg=288
])
def test_gen_conv_kg_tail_numerics(shape):
    """Generic MFMA conv with Kg % 64 != 0 (zero-page tail tile) vs fp32
    torch conv: fwd, bwd-data, bwd-weight, bias grad."""
    from fedkit.ops.conv import FedConvGeneric
    C, K, R, pad, H = shape
    torch.manual_seed(C * 100 + K)
    m = FedConvGeneric(C, K, R, padding=pad).cuda()
    x = torch.randn(16, C, H, H, device="cuda", dtype=torch.bfloat16,
                    requires_grad=True)
    y = m(x)
    gy = torch.randn_like(y)
    y.backward(gy)
    gx, gw, gb = x.grad.clone(), m.weight.grad.clone(), m.bias.grad.clone()

    xr = x.detach().float().requires_grad_(True)
    mr = torch.nn.Conv2d(C, K, R, padding=pad).cuda()
    with torch.no_grad():
        mr.weight.copy_(m.weight)
        mr.bias.copy_(m.bias)
    yr = mr(xr)
    yr.backward(gy.float())
    assert frob_err(y, yr) < 2e-2, frob_err(y, yr)
    assert frob_err(gx, xr.grad) < 3e-2, frob_err(gx, xr.grad)
    assert frob_err(gw, mr.weight.grad) < 3e-2, frob_err(gw, mr.weight.grad)
    assert frob_err(gb, mr.bias.grad) < 3e-2, frob_err(gb, mr.bias.grad)


def test_flat_order_consistency_channels_last():
    """The penalty-side flat vector (flat_trainable) and the LBFGS flat
    grad must traverse elements in the SAME physical order the fused
    pack/unpack/axpy kernels use — channels_last weights made the old
    reshape(-1)/contiguous() forms silently permute (x - z) pairs."""
    from fedkit.models import ResNet18
    from fedkit.utils import (flat_trainable, get_trainable_values,
                              unfreeze_one_block)
    from fedkit.optim.lbfgsnew import LBFGSNew
    torch.manual_seed(61)
    net = ResNet18().cuda().to(memory_format=torch.channels_last)
    unfreeze_one_block(net, 3)
    v_pack = get_trainable_values(net, torch.device("cuda"))
    v_cat = flat_trainable(net).detach()
    assert torch.equal(v_pack, v_cat)

    # grad order: set grad = value, flat grad must equal packed values
    params = [p for p in net.parameters() if p.requires_grad]
    for p in params:
        p.grad = p.data.clone()
    opt = LBFGSNew(params)
    g = opt._flat_grad()
    assert torch.equal(g, v_pack)


def test_frozen_weight_cache_invalidation():
    """The per-module bf16 weight cache keys on the parameter's in-place
    version counter: put_trainable_values / optimizer writes must be
    picked up on the next forward."""
    from fedkit.ops.conv import FedConv2d
    torch.manual_seed(71)
    m = FedConv2d(64, 64, 3, padding=1, bias=False).cuda().to(
        memory_format=torch.channels_last)
    m.weight.requires_grad_(False)
    x = torch.randn(8, 64, 16, 16, device="cuda", dtype=torch.bfloat16
                    ).contiguous(memory_format=torch.channels_last)
    y1 = m(x)
    y2 = m(x)                               # served from cache
    assert torch.equal(y1, y2)
    with torch.no_grad():
        m.weight.mul_(2.0)                  # in-place: version bump
    y3 = m(x)
    assert frob_err(y3.float(), 2.0 * y1.float()) < 1e-2


def test_frozen_cache_invalidation_native_unpack():
    """The hazard ADVICE r1 flagged: put_trainable_values writes through the
    native unpack kernel (raw data_ptr, no dispatcher version bump) — the
    frozen bf16 weight cache must still see the new values on the next
    forward (fedkit.ops.flat bumps the version explicitly)."""
    from fedkit.ops.conv import FedConv2d
    from fedkit.utils.paramvec import (get_trainable_values,
                                       put_trainable_values)
    torch.manual_seed(73)
    m = FedConv2d(64, 64, 3, padding=1, bias=False).cuda().to(
        memory_format=torch.channels_last)
    m.weight.requires_grad_(False)
    x = torch.randn(8, 64, 16, 16, device="cuda", dtype=torch.bfloat16
                    ).contiguous(memory_format=torch.channels_last)
    y1 = m(x)
    _ = m(x)                                # cache now populated
    m.weight.requires_grad_(True)           # "unfreeze block"
    vec = get_trainable_values(m)
    put_trainable_values(m, 2.0 * vec)      # native unpack write
    m.weight.requires_grad_(False)          # "re-freeze"
    y3 = m(x)
    assert frob_err(y3.float(), 2.0 * y1.float()) < 1e-2


def test_lbfgs_history_past_fused_limit_falls_back():
    """history_size > (kMaxVecs-2)//2 must run via the unfused two-loop
    instead of aborting mid-training."""
    from fedkit.optim import LBFGSNew
    torch.manual_seed(3)
    A = torch.randn(40, 40, device="cuda")
    A = A @ A.t() / 40 + torch.eye(40, device="cuda")
    b = torch.randn(40, device="cuda")
    x = torch.zeros(40, device="cuda", requires_grad=True)
    opt = LBFGSNew([x], history_size=14, max_iter=6,
                   line_search_fn=True, batch_mode=False)

    def closure():
        if torch.is_grad_enabled():
            opt.zero_grad()
        f = 0.5 * x @ A @ x - b @ x
        if f.requires_grad:
            f.backward()
        return f

    f0 = float(closure().detach())
    for _ in range(12):
        opt.step(closure)
    f1 = float(closure().detach())
    assert f1 < f0 - 1.0  # made real progress, no abort


def test_vae_elbo_fused_vs_torch():
    """Fused MSE(sum)+KLD kernel vs the fp32 torch composition."""
    from fedkit.ops.losses import vae_loss
    import fedkit.ops as ops
    torch.manual_seed(7)
    recon = torch.rand(64, 3, 32, 32, device="cuda", requires_grad=True)
    x = torch.rand(64, 3, 32, 32, device="cuda")
    mu = torch.randn(64, 10, device="cuda", requires_grad=True)
    logvar = torch.randn(64, 10, device="cuda", requires_grad=True)

    loss = vae_loss(recon, x, mu, logvar)
    loss.backward()
    g = [recon.grad.clone(), mu.grad.clone(), logvar.grad.clone()]
    for t in (recon, mu, logvar):
        t.grad = None

    old = ops._NATIVE_ENV
    ops._NATIVE_ENV = False
    try:
        loss2 = vae_loss(recon, x, mu, logvar)
        loss2.backward()
    finally:
        ops._NATIVE_ENV = old
    assert abs(float(loss) - float(loss2)) / abs(float(loss2)) < 1e-5
    for got, p in zip(g, (recon, mu, logvar)):
        assert frob_err(got, p.grad) < 1e-5


def test_vaecl_terms_fused_vs_torch():
    """Fused cost1/cost3 reduction kernel (whole vaecl_loss) vs the torch
    per-cluster composition — values and all input grads."""
    from fedkit.ops.losses import vaecl_loss
    import fedkit.ops as ops
    torch.manual_seed(11)
    Kc, B, L = 10, 16, 32
    ekhat = torch.softmax(torch.randn(B, Kc, device="cuda"), 1).requires_grad_(True)
    x = torch.rand(B, 3, 32, 32, device="cuda")

    def mk(shape):
        return {ci: torch.rand(*shape, device="cuda").add_(0.1)
                .requires_grad_(True) for ci in range(Kc)}
    mu_xi, sig2_xi = mk((B, L)), mk((B, L))
    mu_b, sig2_b = mk((B, L)), mk((B, L))
    mu_th, sig2_th = mk((B, 3, 32, 32)), mk((B, 3, 32, 32))

    loss = vaecl_loss(ekhat, mu_xi, sig2_xi, mu_b, sig2_b, mu_th, sig2_th, x)
    loss.backward()
    grads = {}
    leaves = [("ekhat", [ekhat])] + [
        (nm, list(d.values())) for nm, d in
        [("mu_xi", mu_xi), ("sig2_xi", sig2_xi), ("mu_b", mu_b),
         ("sig2_b", sig2_b), ("mu_th", mu_th), ("sig2_th", sig2_th)]]
    for nm, ts in leaves:
        grads[nm] = [t.grad.clone() for t in ts]
        for t in ts:
            t.grad = None

    old = ops._NATIVE_ENV
    ops._NATIVE_ENV = False
    try:
        loss2 = vaecl_loss(ekhat, mu_xi, sig2_xi, mu_b, sig2_b,
                           mu_th, sig2_th, x)
        loss2.backward()
    finally:
        ops._NATIVE_ENV = old
    assert abs(float(loss) - float(loss2)) / abs(float(loss2)) < 1e-4, \
        (float(loss), float(loss2))
    for nm, ts in leaves:
        for got, t in zip(grads[nm], ts):
            assert frob_err(got, t.grad) < 1e-4, nm


def test_info_nce_fused_vs_torch():
    """Fused InfoNCE kernel vs the GEMM+softmax torch form."""
    from fedkit.ops.losses import info_nce
    import fedkit.ops as ops
    torch.manual_seed(13)
    z = torch.randn(4, 64, 3, 3, device="cuda", requires_grad=True)
    zhat = torch.randn(4, 64, 3, 3, device="cuda", requires_grad=True)

    loss = info_nce(z, zhat)
    loss.backward()
    gz, gzh = z.grad.clone(), zhat.grad.clone()
    z.grad = zhat.grad = None

    old = ops._NATIVE_ENV
    ops._NATIVE_ENV = False
    try:
        loss2 = info_nce(z, zhat)
        loss2.backward()
    finally:
        ops._NATIVE_ENV = old
    assert abs(float(loss) - float(loss2)) / abs(float(loss2)) < 1e-5
    assert frob_err(gz, z.grad) < 1e-4
    assert frob_err(gzh, zhat.grad) < 1e-4


def test_dilated_bank_fused_vs_per_conv():
    """Fused 5-tap dilated bank (one MFMA launch) vs the per-conv torch
    composition: forward values + input/weight/bias grads."""
    from fedkit.models import EncoderCNN
    import fedkit.ops as ops
    torch.manual_seed(17)
    enc = EncoderCNN().cuda()
    mods = [enc.conv1_1, enc.conv1_2, enc.conv1_4, enc.conv1_8, enc.conv1_16]
    x = torch.randn(9, 8, 32, 32, device="cuda", dtype=torch.bfloat16,
                    requires_grad=True)
    from fedkit.ops.conv import dilated_bank
    y = dilated_bank(x, mods)
    gy = torch.randn_like(y)
    y.backward(gy)
    gx = x.grad.clone()
    gws = [m.weight.grad.clone() for m in mods]
    gbs = [m.bias.grad.clone() for m in mods]
    x.grad = None
    for m in mods:
        m.weight.grad = m.bias.grad = None

    yr = torch.cat([torch.nn.functional.conv2d(
        x.float(), m.weight, m.bias, m.stride, m.padding, m.dilation)
        for m in mods], dim=1)
    yr.backward(gy.float())
    assert frob_err(y, yr) < 2e-2, frob_err(y, yr)
    assert frob_err(gx, x.grad) < 3e-2
    for t, m in enumerate(mods):
        assert frob_err(gws[t], m.weight.grad) < 3e-2, t
        assert frob_err(gbs[t], m.bias.grad) < 3e-2, t


@pytest.mark.parametrize("N,C,H,R,stride,kt,dils,pads", BANK_CASES)
def test_dilated_bank_kernel_variants(N, C, H, R, stride, kt, dils, pads):
    """conv2d_dilated_bank called directly at shapes that reach each of its
    four kernels (64/128-row tile x stride 1/2) vs the per-tap fp32 convs;
    same bound as the fused-bank forward check above."""
    ext = _ext()
    torch.manual_seed(18)
    x = torch.randn(N, C, H, H, device="cuda", dtype=torch.bfloat16)
    ws = [torch.randn(kt, C, R, R, device="cuda", dtype=torch.bfloat16) * 0.1
          for _ in dils]
    kg = R * R * C
    w2d = torch.zeros(64, kg * len(dils), device="cuda", dtype=torch.bfloat16)
    for t, w in enumerate(ws):
        w2d[t * kt:(t + 1) * kt, t * kg:(t + 1) * kg] = \
            w.permute(0, 2, 3, 1).reshape(kt, kg)
    y = ext.conv2d_dilated_bank(
        x.contiguous(memory_format=torch.channels_last), w2d, list(dils),
        list(pads), stride, R, kt * len(dils))
    want = torch.cat([F.conv2d(x.float(), w.float(), None, stride, p, d)
                      for w, d, p in zip(ws, dils, pads)], dim=1)
    assert y.shape == want.shape
    assert frob_err(y, want) < 2e-2, frob_err(y, want)


def test_encoder_bank_path_uses_fusion():
    """EncoderCNN forward goes through the fused bank under bf16 and
    matches the eager fp32 composition."""
    from fedkit.models import EncoderCNN
    import fedkit.ops as ops
    torch.manual_seed(19)
    enc = EncoderCNN().cuda()
    x = torch.randn(9, 8, 32, 32, device="cuda")
    with torch.autocast("cuda", dtype=torch.bfloat16):
        lat = enc(x)
    old = ops._NATIVE_ENV
    ops._NATIVE_ENV = False
    try:
        lat2 = enc(x)
    finally:
        ops._NATIVE_ENV = old
    assert frob_err(lat, lat2) < 5e-2, frob_err(lat, lat2)


@pytest.mark.parametrize("M,K,N,bias", [
    (128, 512, 10, True),      # ResNet18 head
    (128, 400, 120, True),     # Net fc1 (K % 8 != 0 tail)
    (128, 84, 10, True),       # Net fc3 (tiny, K % 8 != 0)
    (128, 1600, 512, True),    # Net1 fc1 (largest)
    (128, 1024, 10, False),
])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_linear_kernels_vs_torch(M, K, N, bias, dtype):
    """csrc/linear.hip fwd/bwd-data/bwd-weight(+bias) vs fp32 F.linear."""
    ext = _ext()
    torch.manual_seed(23)
    x = torch.randn(M, K, device="cuda", dtype=dtype)
    w = torch.randn(N, K, device="cuda", dtype=dtype) * 0.05
    b = torch.randn(N, device="cuda") if bias else None
    y = ext.linear_fwd(x, w, b)
    want = F.linear(x.float(), w.float(), b)
    tol = 1e-5 if dtype == torch.float32 else 1e-2
    assert frob_err(y, want) < tol

    gy = torch.randn(M, N, device="cuda", dtype=dtype)
    gx = ext.linear_bwd_data(gy, w)
    outs = ext.linear_bwd_weight(gy, x, bias)
    xr = x.float().detach().requires_grad_(True)
    wr = w.float().detach().requires_grad_(True)
    br = b.detach().requires_grad_(True) if bias else None
    F.linear(xr, wr, br).backward(gy.float())
    assert frob_err(gx, xr.grad) < tol * 3
    assert frob_err(outs[0], wr.grad) < tol * 3
    if bias:
        assert frob_err(outs[1], br.grad) < tol * 3


def test_fedlinear_module_autograd():
    """FedLinear module end to end under bf16 vs eager fp32."""
    from fedkit.ops.linear import FedLinear
    import fedkit.ops as ops
    torch.manual_seed(29)
    m = FedLinear(512, 10).cuda()
    x = torch.randn(64, 512, device="cuda", dtype=torch.bfloat16,
                    requires_grad=True)
    y = m(x)
    gy = torch.randn_like(y)
    y.backward(gy)
    gx, gw, gb = x.grad.clone(), m.weight.grad.clone(), m.bias.grad.clone()
    x.grad = m.weight.grad = m.bias.grad = None
    old = ops._NATIVE_ENV
    ops._NATIVE_ENV = False
    try:
        y2 = m(x)
        y2.backward(gy)
    finally:
        ops._NATIVE_ENV = old
    assert frob_err(y, y2) < 2e-2
    assert frob_err(gx, x.grad) < 3e-2
    assert frob_err(gw, m.weight.grad) < 3e-2
    assert frob_err(gb, m.bias.grad) < 3e-2


def test_welford_update_fused_vs_torch():
    """Fused Welford grad-stats kernel vs the clone/axpy/addcmul chain."""
    ext = _ext()
    torch.manual_seed(31)
    n = 100000
    g = torch.randn(n, device="cuda")
    avg = torch.randn(n, device="cuda")
    sq = torch.rand(n, device="cuda")
    avg_r, sq_r = avg.clone(), sq.clone()
    it = 5
    out = ext.welford_update(g, avg, sq, 1.0 / it)
    d_old = g - avg_r
    avg_r += d_old / it
    sq_r += (g - avg_r) * d_old
    assert frob_err(avg, avg_r) < 1e-6
    assert frob_err(sq, sq_r) < 1e-6
    assert abs(float(out) - float(sq_r.sum())) / abs(float(sq_r.sum())) < 1e-4


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_bn_elu_pad_out_fusion(dtype):
    """bn_elu(pad_out=1): the padded side-buffer equals pad(elu(bn(x)))
    with zero borders, the autograd output is the interior view, and the
    backward (gy in the unpadded domain, saved-y read at padded coords)
    matches the composed autograd."""
    from fedkit.ops.norm import FedBatchNorm2d, bn_elu
    torch.manual_seed(37)
    C = 64
    bn = FedBatchNorm2d(C).cuda().train()
    x = torch.randn(8, C, 16, 16, device="cuda", dtype=dtype,
                    requires_grad=True)
    y = bn_elu(bn, x.contiguous(memory_format=torch.channels_last),
               pad_out=1)
    assert y.shape == (8, C, 16, 16)
    buf, pad = y._fedkit_padded
    assert pad == 1 and buf.shape == (8, C, 18, 18)
    assert float(buf[:, :, 0, :].abs().max()) == 0.0   # borders zero
    gy = torch.randn_like(x)
    y.backward(gy)
    gx = x.grad.clone()
    gw, gb = bn.weight.grad.clone(), bn.bias.grad.clone()
    x.grad = bn.weight.grad = bn.bias.grad = None

    bn2 = FedBatchNorm2d(C).cuda().train()
    with torch.no_grad():
        bn2.weight.copy_(bn.weight)
        bn2.bias.copy_(bn.bias)
    yref = F.elu(F.batch_norm(
        x.float(), bn2.running_mean, bn2.running_var, bn2.weight, bn2.bias,
        True, 0.1, 1e-5))
    yref.backward(gy.float())
    tol = 1e-3 if dtype == torch.float32 else 5e-2
    assert rel_err(y, yref) < tol
    assert rel_err(buf[:, :, 1:-1, 1:-1], yref) < tol
    assert rel_err(gx, x.grad) < tol
    assert rel_err(gw, bn2.weight.grad) < tol
    assert rel_err(gb, bn2.bias.grad) < tol


def test_resnet_block_pad_fusion_end_to_end():
    """A BasicBlock through the apply-into-pad path vs eager fp32."""
    import fedkit.ops as ops
    from fedkit.models.resnet import BasicBlock
    torch.manual_seed(41)
    blk = BasicBlock(64, 64).cuda().to(memory_format=torch.channels_last)
    x = torch.randn(16, 64, 16, 16, device="cuda").contiguous(
        memory_format=torch.channels_last)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        y = blk(x)
    loss = y.float().square().mean()
    loss.backward()
    nat = {n: p.grad.float().clone() for n, p in blk.named_parameters()}
    blk.zero_grad(set_to_none=True)
    old = ops._NATIVE_ENV
    ops._NATIVE_ENV = False
    try:
        y2 = blk(x)
        loss2 = y2.square().mean()
        loss2.backward()
    finally:
        ops._NATIVE_ENV = old
    assert frob_err(y, y2) < 5e-2
    for n, p in blk.named_parameters():
        assert frob_err(nat[n], p.grad.float()) < 8e-2, n


def test_bn_elu_padded_residual():
    """bn_elu with a producer-PADDED residual (phase-B fusion): values and
    the residual's padded-domain gradient vs the composed form."""
    from fedkit.ops.norm import FedBatchNorm2d, bn_elu
    torch.manual_seed(43)
    C = 64
    bn_a = FedBatchNorm2d(C).cuda().train()
    bn_b = FedBatchNorm2d(C).cuda().train()
    x0 = torch.randn(8, C, 16, 16, device="cuda", requires_grad=True)
    xmid = torch.randn(8, C, 16, 16, device="cuda")
    # producer: padded side-buffer (the "block input")
    blk_in = bn_elu(bn_a, x0.contiguous(memory_format=torch.channels_last),
                    pad_out=1)
    assert blk_in._fedkit_padded[1] == 1
    # consumer bn2: unpadded conv output + the marked residual (its padded
    # buffer is read at interior coordinates in-kernel)
    y = bn_elu(bn_b, xmid.contiguous(memory_format=torch.channels_last),
               residual=blk_in)
    assert y.shape == (8, C, 16, 16)
    loss = y.float().square().sum()
    loss.backward()
    gx0 = x0.grad.clone()
    x0.grad = None
    for m in (bn_a, bn_b):
        m.zero_grad(set_to_none=True)

    bn_a2 = FedBatchNorm2d(C).cuda().train()
    bn_b2 = FedBatchNorm2d(C).cuda().train()
    with torch.no_grad():
        for dst, src in ((bn_a2, bn_a), (bn_b2, bn_b)):
            dst.weight.copy_(src.weight)
            dst.bias.copy_(src.bias)
    ref_in = F.elu(F.batch_norm(x0, bn_a2.running_mean, bn_a2.running_var,
                                bn_a2.weight, bn_a2.bias, True, 0.1, 1e-5))
    yref = F.elu(F.batch_norm(xmid, bn_b2.running_mean, bn_b2.running_var,
                              bn_b2.weight, bn_b2.bias, True, 0.1, 1e-5)
                 + ref_in)
    yref.float().square().sum().backward()
    assert rel_err(y, yref) < 1e-3
    assert rel_err(gx0, x0.grad) < 1e-3


def test_round_checkpoint_resume_gpu(tmp_path):
    """Kill-and-resume on GPU (CUDA RNG state in the sidecar): the resumed
    FedAvg run reproduces the uninterrupted run's final weights."""
    from fedkit.parallel import FedConfig, FederatedJob

    def cfg_for(sub, **kw):
        d = tmp_path / sub
        d.mkdir(exist_ok=True)
        return FedConfig(K=2, default_batch=32, Nloop=2, Nepoch=1, Nadmm=1,
                         use_cuda=True, check_results=False, dtype="bf16",
                         max_steps_per_epoch=2, save_model=False,
                         strategy="fedavg", model="Net",
                         round_checkpoint=True, ckpt_prefix=str(d / "s"),
                         **kw)

    job_a = FederatedJob(cfg_for("a"))
    job_a.run()
    sd_a = {ck: {k: v.clone() for k, v in job_a.nets[ck].state_dict().items()}
            for ck in (0, 1)}

    class Killed(Exception):
        pass

    nl = {"v": 0, "seen": -1}

    def hook(job, ci):
        if ci <= nl["seen"]:
            nl["v"] += 1
        nl["seen"] = ci
        if (nl["v"], ci) == (1, 2):
            raise Killed

    job_b = FederatedJob(cfg_for("b"), block_hook=hook)
    with pytest.raises(Killed):
        job_b.run()
    job_c = FederatedJob(cfg_for("b", load_model=True))
    job_c.run()
    for ck in (0, 1):
        sd_c = job_c.nets[ck].state_dict()
        for k in sd_a[ck]:
            assert torch.allclose(sd_a[ck][k].float(), sd_c[k].float(),
                                  atol=1e-6), (ck, k)


def test_fused_adam_matches_torch_adam():
    """FusedAdam (one HIP kernel/step) == torch.optim.Adam over many steps,
    including bias correction and L2 weight decay; state-dict layout
    identical (checkpoint contract)."""
    from fedkit.optim import FusedAdam
    torch.manual_seed(47)
    shapes = [(64, 3, 3, 3), (64,), (512, 256), (10,), (7, 11)]
    p1 = [torch.randn(s, device="cuda", requires_grad=True) for s in shapes]
    p2 = [p.detach().clone().requires_grad_(True) for p in p1]
    o1 = FusedAdam(p1, lr=3e-3, weight_decay=0.01)
    o2 = torch.optim.Adam(p2, lr=3e-3, weight_decay=0.01)
    for it in range(10):
        torch.manual_seed(100 + it)
        gs = [torch.randn(s, device="cuda") for s in shapes]
        for p, g in zip(p1, gs):
            p.grad = g.clone()
        for p, g in zip(p2, gs):
            p.grad = g.clone()
        o1.step()
        o2.step()
    for a, b in zip(p1, p2):
        assert frob_err(a, b) < 1e-5
    sd1 = o1.state_dict()["state"][0]
    assert set(sd1.keys()) == {"step", "exp_avg", "exp_avg_sq"}
    for m1, m2 in zip(o1.state_dict()["state"].values(),
                      o2.state_dict()["state"].values()):
        assert frob_err(m1["exp_avg"], m2["exp_avg"]) < 1e-5
        # second moment: g*g accumulation order differs (fma vs addcmul),
        # measured 1.3e-5 relative after 10 steps — rounding, not math
        assert frob_err(m1["exp_avg_sq"], m2["exp_avg_sq"]) < 1e-4


def test_fused_adam_past_one_table():
    """50 parameters (two 48-tensor tables) of numels around the 4-wide
    unit, two steps, against torch.optim.Adam."""
    from fedkit.optim import FusedAdam
    torch.manual_seed(48)
    numels = [(1, 3, 4, 5, 7)[i % 5] for i in range(50)]
    p1 = [torch.randn(n, device="cuda", requires_grad=True) for n in numels]
    p2 = [p.detach().clone().requires_grad_(True) for p in p1]
    o1 = FusedAdam(p1, lr=3e-3, weight_decay=0.01)
    o2 = torch.optim.Adam(p2, lr=3e-3, weight_decay=0.01)
    for it in range(2):
        torch.manual_seed(200 + it)
        for a, b in zip(p1, p2):
            a.grad = torch.randn_like(a)
            b.grad = a.grad.clone()
        o1.step()
        o2.step()
    for a, b in zip(p1, p2):
        assert frob_err(a, b) < 1e-5
    for m1, m2 in zip(o1.state_dict()["state"].values(),
                      o2.state_dict()["state"].values()):
        assert frob_err(m1["exp_avg"], m2["exp_avg"]) < 1e-5
        assert frob_err(m1["exp_avg_sq"], m2["exp_avg_sq"]) < 1e-4


@pytest.mark.parametrize("case", ["late_state_dtype", "grad_numel"])
def test_adam_step_rejects_before_launch(case):
    ext = _ext()
    torch.manual_seed(49)
    n = 50 if case == "late_state_dtype" else 3
    ps = [torch.randn(7, device="cuda") for _ in range(n)]
    gs = [torch.randn(7, device="cuda") for _ in range(n)]
    ms = [torch.randn(7, device="cuda") for _ in range(n)]
    vs = [torch.rand(7, device="cuda") for _ in range(n)]
    if case == "late_state_dtype":
        vs[-1] = vs[-1].to(torch.bfloat16)
    else:
        gs[1] = torch.randn(6, device="cuda")
    _assert_rejected_untouched(
        lambda: ext.adam_step(ps, gs, ms, vs, 1e-3, 0.9, 0.999, 1e-8, 1, 0.0),
        ps + ms + vs)


def test_fused_adam_bumps_param_versions():
    """The raw-pointer Adam write must advance version counters so frozen
    weight caches invalidate (same hazard as put_trainable_values)."""
    from fedkit.optim import FusedAdam
    p = torch.randn(32, device="cuda", requires_grad=True)
    opt = FusedAdam([p], lr=1e-3)
    p.grad = torch.randn(32, device="cuda")
    v0 = p._version
    opt.step()
    assert p._version > v0
