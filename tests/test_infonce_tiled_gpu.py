"""csrc/infonce_tiled.hip (info_nce_tiled_fwd / _bwd, 64 < P <= 1024) against
the float64 evaluation of the info_nce formula on the same inputs, and
info_nce's three-way dispatch.

Shapes are (B, C, px, py), D = B C, P = px py:
  (1, 3, 5, 13)     D 3, P 65: one past the gate, tile tail of 1, D < a chunk
  (2, 12, 15, 7)    D 24, P 105: tails on both P tiles, D no chunk multiple
  (4, 50, 10, 13)   D 200, P 130: three P tiles, tail of 2, D split
  (128, 32, 15, 7)  D 4096, P 105: the CPC driver's D, D split
  (1, 8, 32, 32)    D 8, P 1024: the upper limit, unsplit

Kernel outputs: |zz - zz64| <= 2 (D + 4) 2^-24 (an fp32 dot of D terms in any
order errs by at most D 2^-24 sum |a b| <= D 2^-24 nz nzh, the two norms add
as much again relative to |zz| <= 1, + 4 for the roots and the divide);
|norms - norms64| <= (D + 4) 2^-24 norms64; soft rows sum to 1 within
P 2^-23; a second call returns the same bits.

Public function: e = max |out - ref64| / max |ref64| of loss, z.grad and
zhat.grad must be at most 4 x the same figure of the fp32 torch sequence on
the same GPU and inputs (two summation orders of one fp32 computation), with
a floor of 2 (D + 4) 2^-24, plus 2^-8 on the gradients of bf16 inputs for the
one rounding of the store.
"""

import functools

import pytest
import torch

from fedkit import ops
from fedkit.ops.losses import info_nce

pytestmark = pytest.mark.gpu

SHAPES = [(1, 3, 5, 13), (2, 12, 15, 7), (4, 50, 10, 13), (128, 32, 15, 7),
          (1, 8, 32, 32)]
CASES = [(s, torch.float32) for s in SHAPES] + [
    (SHAPES[1], torch.bfloat16), (SHAPES[2], torch.bfloat16)]
EPS = 2.0 ** -24


def _formula(z, zhat):
    """(loss, zz, norms [2, P]) of the info_nce formula in z's dtype"""
    P = z.shape[2] * z.shape[3]
    Z, Zhat = z.reshape(-1, P), zhat.reshape(-1, P)
    nz, nzh = Z.norm(dim=0, keepdim=True), Zhat.norm(dim=0, keepdim=True)
    zz = (Z / nz).t() @ (Zhat / nzh)
    loss = -torch.log(torch.softmax(zz, dim=1).diagonal() + 1e-6).sum()
    return loss, zz, torch.cat([nz, nzh])


@functools.lru_cache(maxsize=None)
def _case(shape, dtype):
    """inputs and their float64 reference, built once per case"""
    g = torch.Generator().manual_seed(31)
    z, zhat = (torch.randn(*shape, generator=g).to("cuda", dtype)
               for _ in range(2))
    z64, zh64 = (t.double().requires_grad_() for t in (z, zhat))
    loss, zz, norms = _formula(z64, zh64)
    loss.backward()
    return z, zhat, dict(loss=loss.detach(), zz=zz.detach(),
                         norms=norms.detach(), gz=z64.grad, gzh=zh64.grad)


def _rel(out, ref):
    return float((out.double() - ref).abs().max() / ref.abs().max())


def _loss_and_grads(z, zhat):
    z, zhat = (t.detach().clone().requires_grad_() for t in (z, zhat))
    loss = info_nce(z, zhat)
    loss.backward()
    return loss.detach(), z.grad, zhat.grad


@pytest.mark.parametrize("shape,dtype", CASES)
def test_tiled_fwd_outputs_vs_float64(shape, dtype):
    z, zhat, ref = _case(shape, dtype)
    P = shape[2] * shape[3]
    Z, Zhat = z.reshape(-1, P), zhat.reshape(-1, P)
    D = Z.shape[0]
    ext = ops.require_ext()
    loss, zz, soft, norms = ext.info_nce_tiled_fwd(Z, Zhat)
    assert loss.shape == () and loss.dtype == torch.float32
    assert zz.shape == soft.shape == (P, P) and norms.shape == (2, P)
    zz_err = float((zz.double() - ref["zz"]).abs().max())
    n_err = float(((norms.double() - ref["norms"]).abs() / ref["norms"]).max())
    row_err = float((soft.double().sum(1) - 1).abs().max())
    print(f"zz err {zz_err:.3g} / {2 * (D + 4) * EPS:.3g}, norms rel err "
          f"{n_err:.3g} / {(D + 4) * EPS:.3g}, row sums {row_err:.3g}")
    assert zz_err <= 2 * (D + 4) * EPS
    assert n_err <= (D + 4) * EPS
    assert row_err <= P * 2.0 ** -23
    again = ext.info_nce_tiled_fwd(Z, Zhat)
    for a, b in zip((loss, zz, soft, norms), again):
        assert torch.equal(a, b)


@pytest.mark.parametrize("shape,dtype", CASES)
def test_info_nce_vs_float64_and_torch_sequence(shape, dtype):
    z, zhat, ref = _case(shape, dtype)
    D = shape[0] * shape[1]
    native = _loss_and_grads(z, zhat)
    assert native[1].dtype == native[2].dtype == dtype
    old = ops._NATIVE_ENV
    ops._NATIVE_ENV = False
    try:
        torch_seq = _loss_and_grads(z.float(), zhat.float())
    finally:
        ops._NATIVE_ENV = old
    for k, (name, key) in enumerate((("loss", "loss"), ("z.grad", "gz"),
                                     ("zhat.grad", "gzh"))):
        e_nat, e_seq = _rel(native[k], ref[key]), _rel(torch_seq[k], ref[key])
        bound = max(4 * e_seq, 2 * (D + 4) * EPS)
        if k and dtype == torch.bfloat16:
            bound += 2.0 ** -8
        print(f"{shape} {str(dtype)[6:]} {name}: native {e_nat:.3g} "
              f"torch {e_seq:.3g} bound {bound:.3g}")
        assert e_nat <= bound, name


def test_dispatch_and_limits():
    ext = ops.require_ext()
    rn = lambda *s: torch.randn(*s, device="cuda", requires_grad=True)  # noqa: E731
    name = lambda px, py: type(  # noqa: E731
        info_nce(rn(2, 4, px, py), rn(2, 4, px, py)).grad_fn).__name__
    assert name(15, 7).startswith("_InfoNceTiledFn")
    assert name(7, 7).startswith("_InfoNceFn")
    assert "InfoNce" not in name(32, 33)
    for P in (49, 1056):
        with pytest.raises(RuntimeError, match="64 < P <= 1024"):
            ext.info_nce_tiled_fwd(rn(8, P).detach(), rn(8, P).detach())
    with pytest.raises(RuntimeError, match="differ in shape"):
        ext.info_nce_tiled_fwd(rn(8, 105).detach(), rn(9, 105).detach())
    splits = [ext.info_nce_tiled_plan(B * C, px * py)[1]
              for B, C, px, py in SHAPES]
    assert splits[2] > 1 and splits[3] > 1 and splits[4] == 1, splits
