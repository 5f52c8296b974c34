"""csrc/linear_mfma.hip (linear_mfma_fwd / _bwd_data / _bwd_weight) against
the float64 product of the same bf16 inputs, and FedLinear's dispatch to it.

Mode `int`: x, gy in {-1, 0, 1}, w in {-2..2}, integer bias: every partial
sum is an integer below 2^24, fp32 accumulation is exact in any order, so the
results are required bit for bit (a wrong lane map, a wrong tail or a lost
split partial cannot hide in a tolerance).

Mode `randn`: per element |out - ref| <= 2 (R + 2) 2^-24 S + e, R the
reduction length, S the same product over absolute values (plus |b| in
forward), e = 2^-8 |ref| for bf16 outputs and 0 for fp32 ones: bf16 x bf16 is
exact in fp32, an fp32 sum of R terms in any order errs by at most about
R 2^-24 sum |terms|, and one rounding to bf16's 8 significant bits moves a
value v by at most 2^-8 |v| (half an ulp at the bottom of a binade), so e
itself has no slack and the factor 2 of the first term is the margin.

Plans of the shapes (csrc/linear_plan.h): (130, 264, 136) splits the
reduction in forward (3 slabs) and in bwd-data (2), the Net layers split in
both, (1, 8, 8) and (17, 72, 24) in neither.
"""

import pytest
import torch

from fedkit import ops
from fedkit.ops.linear import FedLinear

pytestmark = pytest.mark.gpu

SHAPES = [(1, 8, 8), (17, 72, 24), (130, 264, 136), (40, 512, 1024),
          (128, 1600, 512)]


def _inputs(M, K, N, mode):
    g = torch.Generator().manual_seed(23)
    if mode == "int":
        ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g)  # noqa: E731
        x, w, gy = ri(-1, 1, M, K), ri(-2, 2, N, K), ri(-1, 1, M, N)
        b = ri(-3, 3, N).float()
    else:
        rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
        x, w, gy, b = rn(M, K), rn(N, K) * 0.05, rn(M, N), rn(N)
    return [t.to("cuda", torch.bfloat16) for t in (x, w, gy)] + [b.cuda()]


def _check(name, out, ref, R, S, mode, rounded):
    """out against the float64 ref; rounded: out went through a bf16 cast"""
    if mode == "int":
        want = ref.float().to(torch.bfloat16) if rounded else ref.float()
        assert torch.equal(out.to(want.dtype), want), name
        return
    err = (out.double() - ref).abs()
    bound = 2 * (R + 2) * 2.0 ** -24 * S
    if rounded:
        bound = bound + 2.0 ** -8 * ref.abs()
    print(f"{name}: max err / bound {float((err / bound).max()):.3g}")
    assert bool((err <= bound).all()), name


def _check_all(y, gx, gw, gb, x, w, gy, b, mode, gw_rounded):
    xd, wd, gd, bd = x.double(), w.double(), gy.double(), b.double()
    M, K = x.shape
    N = w.shape[0]
    _check("y", y, xd @ wd.T + bd, K, xd.abs() @ wd.abs().T + bd.abs(), mode,
           True)
    _check("gx", gx, gd @ wd, N, gd.abs() @ wd.abs(), mode, True)
    _check("gw", gw, gd.T @ xd, M, gd.abs().T @ xd.abs(), mode, gw_rounded)
    _check("gb", gb, gd.sum(0), M, gd.abs().sum(0), mode, False)


@pytest.mark.parametrize("mode", ["int", "randn"])
@pytest.mark.parametrize("M,K,N", SHAPES)
def test_linear_mfma_passes_vs_float64(M, K, N, mode):
    ext = ops.require_ext()
    x, w, gy, b = _inputs(M, K, N, mode)
    y = ext.linear_mfma_fwd(x, w, b)
    assert torch.equal(y, ext.linear_mfma_fwd(x, w, b))
    gx = ext.linear_mfma_bwd_data(gy, w)
    gw, gb = ext.linear_mfma_bwd_weight(gy, x, True)
    assert y.dtype == gx.dtype == torch.bfloat16
    assert gw.dtype == gb.dtype == torch.float32
    _check_all(y, gx, gw, gb, x, w, gy, b, mode, False)


def test_shapes_cover_split_and_unsplit_plans():
    plans = [ops.require_ext().linear_mfma_plan(M, N, K) for M, K, N in SHAPES]
    for p in (0, 1):                       # forward, bwd-data
        splits = [pl[p][2] for pl in plans]
        assert min(splits) == 1 and max(splits) > 1, splits
    assert all(pl[2][2] == 1 for pl in plans)      # bwd-weight never splits


def test_fedlinear_dispatches_large_fc_to_mfma():
    torch.manual_seed(29)
    m = FedLinear(1600, 512).cuda()
    x = torch.randn(40, 1600, device="cuda", dtype=torch.bfloat16,
                    requires_grad=True)
    y = m(x)
    assert type(y.grad_fn).__name__.startswith("_LinearMfmaFn")
    gy = torch.randn_like(y)
    y.backward(gy)
    w16 = m.weight.detach().to(torch.bfloat16)
    _check_all(y.detach(), x.grad, m.weight.grad, m.bias.grad, x.detach(), w16,
               gy, m.bias.detach(), "randn", True)
    head = FedLinear(512, 10).cuda()(torch.randn(
        40, 512, device="cuda", dtype=torch.bfloat16))
    assert type(head.grad_fn).__name__.startswith("_LinearFn")


def test_linear_mfma_preconditions():
    ext = ops.require_ext()
    bf = dict(device="cuda", dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="multiples of 8"):
        ext.linear_mfma_fwd(torch.zeros(4, 12, **bf), torch.zeros(8, 12, **bf))
    with pytest.raises(RuntimeError, match="bf16"):
        ext.linear_mfma_fwd(torch.zeros(4, 16, device="cuda"),
                            torch.zeros(8, 16, **bf))
