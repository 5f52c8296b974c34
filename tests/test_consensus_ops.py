"""fedkit.ops.consensus on CPU: the stock-torch fallbacks, their gradients,
the bit-compatibility promise for CPU runs, and Strategy.penalty_args."""

import pytest
import torch

from fedkit.algos import ConsensusADMM, FedProx
from fedkit.algos.strategies import Strategy
from fedkit.ops import consensus
from fedkit.parallel.comm import LocalComm

RHO, L1, L2 = 0.3, 1e-2, 1e-3
MODES = ["admm", "fedprox", "reg"]


def _params(dtype, away_from_zero=False):
    """A small parameter list with a channels_last conv weight in it."""
    g = torch.Generator().manual_seed(11)
    shapes = [(7,), (5, 3), (4, 3, 2, 2), (1,)]
    ps = []
    for s in shapes:
        t = torch.randn(*s, generator=g, dtype=dtype)
        if away_from_zero:
            t = t + torch.sign(t) * 0.5
        if len(s) == 4:
            t = t.contiguous(memory_format=torch.channels_last)
        ps.append(t)
    n = sum(p.numel() for p in ps)
    z = torch.randn(n, generator=g, dtype=dtype)
    y = torch.randn(n, generator=g, dtype=dtype)
    return ps, z, y


def _physical(ps):
    return torch.cat([p.permute(0, 2, 3, 1).reshape(-1) if p.dim() == 4
                      else p.reshape(-1) for p in ps])


def _mode_args(mode, z, y):
    if mode == "admm":
        return {"z": z, "y": y, "rho": RHO}
    if mode == "fedprox":
        return {"z": z, "y": None, "rho": RHO}
    return {}


def _formula(x, mode, z, y, l1, l2):
    """The penalty written out by hand (any dtype)."""
    out = l1 * x.abs().sum() + l2 * (x * x).sum()
    if mode in ("admm", "fedprox"):
        d = x - z
        out = out + 0.5 * RHO * (d * d).sum()
        if mode == "admm":
            out = out + (y * d).sum()
    return out


@pytest.mark.parametrize("mode", MODES)
def test_fallback_matches_formula_float64(mode):
    ps, z, y = _params(torch.float64)
    got = consensus.penalty(ps, lambda1=L1, lambda2=L2,
                            **_mode_args(mode, z, y))
    ref = _formula(_physical(ps), mode, z, y, L1, L2)
    assert got.dtype == torch.float64
    assert torch.allclose(got, ref, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("mode", MODES)
def test_fallback_gradcheck(mode):
    ps, z, y = _params(torch.float64, away_from_zero=True)
    ps = [p.requires_grad_() for p in ps]
    kw = _mode_args(mode, z, y)
    assert torch.autograd.gradcheck(
        lambda *p: consensus.penalty(p, lambda1=L1, lambda2=L2, **kw), ps)


@pytest.mark.parametrize("lambda1", [0.0, L1])
@pytest.mark.parametrize("mode", ["admm", "fedprox"])
def test_fallback_bit_identical_to_closure_expression(mode, lambda1):
    """penalty == strategy.penalty + lambda1*norm1 + lambda2*norm2**2, bit
    for bit: a CPU run computes what it computed before the op existed."""
    ps, z, y = _params(torch.float32)
    n = z.numel()
    comm = LocalComm(2, device=torch.device("cpu"))
    strat = ConsensusADMM(rho0=RHO) if mode == "admm" else FedProx(rho0=RHO)
    st = strat.init_block(comm, n, "cpu")
    st["z"] = z
    if mode == "admm":
        st["y"][1] = y
    vec = _physical(ps)
    expect = strat.penalty(st, 1, vec)
    if lambda1:
        expect = expect + lambda1 * torch.norm(vec, 1)
    expect = expect + L2 * (torch.norm(vec, 2) ** 2)
    got = consensus.penalty(ps, lambda1=lambda1, lambda2=L2,
                            **strat.penalty_args(st, 1))
    assert torch.equal(got, expect)


def test_fallback_regulariser_only_bit_identical():
    ps, _, _ = _params(torch.float32)
    vec = _physical(ps)
    expect = L1 * torch.norm(vec, 1) + L2 * (torch.norm(vec, 2) ** 2)
    assert torch.equal(consensus.penalty(ps, lambda1=L1, lambda2=L2), expect)


def test_fallback_no_grad_and_asserts():
    ps, z, y = _params(torch.float32)
    ps = [p.requires_grad_() for p in ps]
    with torch.no_grad():
        v = consensus.penalty(ps, z=z, y=y, rho=RHO)
    assert v.grad_fn is None and not v.requires_grad
    with pytest.raises(AssertionError):
        consensus.penalty(ps, z=z.clone().requires_grad_(), rho=RHO)
    with pytest.raises(AssertionError):
        consensus.penalty(ps, z=z, y=y.clone().requires_grad_(), rho=RHO)


def test_bb_stats_fallback():
    g = torch.Generator().manual_seed(3)
    y, yh, x, z, x0 = (torch.randn(101, generator=g) for _ in range(5))
    a, b, dx = y - yh, x - z, x - x0
    ref = torch.stack([a.dot(a), a.dot(b), b.dot(b),
                       a.dot(dx), b.dot(dx), dx.dot(dx)])
    got = consensus.bb_stats(y, yh, x, z, x0)
    assert got.shape == (6,)
    assert torch.equal(got, ref)


def test_admm_dual_update_fallback():
    g = torch.Generator().manual_seed(4)
    y, x, z = (torch.randn(101, generator=g) for _ in range(3))
    y_ref = y + RHO * (x - z)
    sq_ref = torch.norm(RHO * (x - z)) ** 2
    sq = consensus.admm_dual_update(y, x, z, RHO)
    assert torch.equal(y, y_ref)
    assert torch.allclose(sq, sq_ref, rtol=1e-6)


def test_penalty_args():
    comm = LocalComm(2, device=torch.device("cpu"))
    n = 9
    assert Strategy().penalty_args({}, 0) is None

    prox = FedProx(rho0=2.0)
    st = prox.init_block(comm, n, "cpu", block_idx=3)
    pa = prox.penalty_args(st, 1)
    assert set(pa) == {"z", "y", "rho"}
    assert pa["z"] is st["z"] and pa["y"] is None and pa["rho"] == 2.0

    admm = ConsensusADMM(rho0=0.25)
    st = admm.init_block(comm, n, "cpu")
    pa = admm.penalty_args(st, 1)
    assert set(pa) == {"z", "y", "rho"}
    assert pa["z"] is st["z"] and pa["y"] is st["y"][1]
    assert pa["rho"] == 0.25

    for strat in (FedProx(rho0=2.0, warmup_rounds=1),
                  ConsensusADMM(rho0=0.25, warmup_rounds=1)):
        st = strat.init_block(comm, n, "cpu")
        assert strat.penalty_args(st, 0) is None
        assert strat.penalty(st, 0, torch.zeros(n)) is None
        st["round"] = 1
        assert strat.penalty_args(st, 0) is not None


def test_fused_penalty_is_a_cli_flag():
    from fedkit.parallel import FedConfig
    from fedkit.utils.cli import config_from_cli
    assert FedConfig().fused_penalty is True
    cfg = config_from_cli(FedConfig(), ["--fused_penalty", "0"])
    assert cfg.fused_penalty is False
