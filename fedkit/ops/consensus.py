"""Consensus penalty and ADMM update ops (FedProx / consensus ADMM hot path).

The closure of a FedProx/ADMM client adds, on every call,

    [y.(x-z)] + (rho/2)||x-z||^2 + lambda1 ||x||_1 + lambda2 ||x||^2

over the trainable block x (consensus_multi.py:209-218,
fedprox_multi.py:183-190, federated_multi.py:183-187).  On MI355X
`penalty` evaluates it with ONE streaming reduction that reads the
parameter tensors in place and differentiates it with ONE elementwise
kernel writing the closed-form gradient (csrc/consensus.hip) — no cat of
the block, no autograd tape over a dozen elementwise ops.  The aggregation
side has `admm_dual_update` (y += rho (x-z) fused with the primal-residual
norm) and `bb_stats` (the six Barzilai-Borwein inner products in one pass).

All vectors are fp32 in PHYSICAL (storage) element order, the order
flat.pack / paramvec.flat_physical use.  Dispatch follows the package rule:
native on a ROCm tensor (raising when the extension is missing), stock
torch on CPU.  The CPU expressions are the ones the engine and the
strategies have always used, in the same order, so CPU runs stay
bit-identical.
"""

from typing import Optional, Sequence

import torch
from torch.autograd.function import once_differentiable

from .flat import _flat_views


def _use_native(t: torch.Tensor) -> bool:
    from . import native_enabled
    return native_enabled(t)


def _flat_physical(p: torch.Tensor) -> torch.Tensor:
    # same as fedkit.utils.paramvec.flat_physical (utils imports ops)
    if p.dim() == 4 and p.is_contiguous(memory_format=torch.channels_last):
        return p.permute(0, 2, 3, 1).reshape(-1)
    return p.reshape(-1)


def _penalty_torch(params, z, y, rho, lambda1, lambda2):
    """The expression sequence of FederatedJob's closure + Strategy.penalty."""
    vec = torch.cat([_flat_physical(p) for p in params])
    out = None
    if z is not None:
        xdelta = vec - z
        out = 0.5 * rho * (torch.norm(xdelta, 2) ** 2)
        if y is not None:
            out = torch.dot(y, xdelta) + out
    if lambda1 or lambda2:
        if lambda1:
            reg1 = lambda1 * torch.norm(vec, 1)
            out = reg1 if out is None else out + reg1
        reg2 = lambda2 * (torch.norm(vec, 2) ** 2)
        out = reg2 if out is None else out + reg2
    if out is None:
        out = vec.sum() * 0.0
    return out


class _PenaltyFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, y, rho, lambda1, lambda2, *params):
        from . import require_ext
        ctx.save_for_backward(*params)
        ctx.consts = (z, y, rho, lambda1, lambda2)
        return require_ext().penalty_fwd([p.detach() for p in params], z, y,
                                         rho, lambda1, lambda2)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        from . import require_ext
        params = ctx.saved_tensors
        z, y, rho, lambda1, lambda2 = ctx.consts
        flat = require_ext().penalty_bwd(
            [p.detach() for p in params], z, y, rho, lambda1, lambda2,
            grad_out.to(torch.float32).contiguous())
        return (None,) * 5 + tuple(_flat_views(flat, params))


def penalty(params: Sequence[torch.Tensor], z: Optional[torch.Tensor] = None,
            y: Optional[torch.Tensor] = None, rho: float = 0.0,
            lambda1: float = 0.0, lambda2: float = 0.0) -> torch.Tensor:
    """[y.(x-z)] + (rho/2)||x-z||^2 + lambda1||x||_1 + lambda2||x||^2 with x
    the physical-order concatenation of `params`; differentiable w.r.t. the
    parameters.  z=None drops both proximal terms (regulariser only), y=None
    only the dual term (FedProx).  Under no_grad only the value is computed.
    """
    params = list(params)
    assert len(params) > 0, "penalty needs at least one parameter tensor"
    assert z is not None or y is None, "a dual vector y needs a target z"
    assert z is None or not z.requires_grad, "z must not require grad"
    assert y is None or not y.requires_grad, "y must not require grad"
    rho, lambda1, lambda2 = float(rho), float(lambda1), float(lambda2)
    if _use_native(params[0]):
        return _PenaltyFn.apply(z, y, rho, lambda1, lambda2, *params)
    return _penalty_torch(params, z, y, rho, lambda1, lambda2)


def admm_dual_update(y: torch.Tensor, x: torch.Tensor, z: torch.Tensor,
                     rho: float) -> torch.Tensor:
    """y += rho (x - z) in place; returns the scalar tensor
    sum((rho (x - z))^2) (the squared primal-residual norm)."""
    if _use_native(y):
        from . import require_ext
        return require_ext().admm_dual_update(y, x.contiguous(),
                                              z.contiguous(), float(rho))
    ydelta = rho * (x - z)
    y.add_(ydelta)
    return torch.norm(ydelta) ** 2


def bb_stats(y: torch.Tensor, yhat0: torch.Tensor, x: torch.Tensor,
             z: torch.Tensor, x0: torch.Tensor) -> torch.Tensor:
    """fp32 [6] = (a.a, a.b, b.b, a.dx, b.dx, dx.dx) with a = y - yhat0,
    b = x - z, dx = x - x0 (the BB spectral-stepsize statistics)."""
    if _use_native(y):
        from . import require_ext
        return require_ext().bb_stats(y.contiguous(), yhat0.contiguous(),
                                      x.contiguous(), z.contiguous(),
                                      x0.contiguous())
    a = y - yhat0
    b = x - z
    dx = x - x0
    return torch.stack([a.dot(a), a.dot(b), b.dot(b),
                        a.dot(dx), b.dot(dx), dx.dot(dx)])
