"""consensus.pairwise_sqdist / krum_round (csrc/krum.hip) against float64 and
the torch sequence that defines the round.  K covers both MFMA shapes, the
16 | 17 boundary and the limits; n = 3 is a tail only, 65 under one tile,
1029 = 4 * 256 + 5 the tile and wave-share boundaries, 524295 a second
grid-stride trip that ends in a tail.

Inputs: centre c = 0.05 randn, honest client k = c + 0.01 (1 + 0.05 k) randn,
the f clients K-1, K-3, ... replaced by c - 4 (x - c) + 0.02.

Distance bound |D - D64| <= C 2^-24 (|a_i|^2 + |a_j|^2), a = x - c: C is 4 x
the largest scaled error of torch's own fp32 A @ A.T of the centred stack
over the grid of test_pairwise_sqdist on the MI355X (the two accumulation
orders differ, and rounding error grows with the chain length).  Measured:
torch 125.89 (84..126 at n = 524295, at most 5.51 at the smaller n), the
kernel 4.46.
"""

import math

import pytest
import torch

from fedkit.algos.strategies import FedAvg, FedProx
from fedkit.ops import consensus
from fedkit.parallel.comm import LocalComm

gpu = pytest.mark.gpu
RHO = 0.1
MODES = ["fedavg", "fedprox"]
K_F = [(5, 1), (10, 2), (16, 3), (17, 7), (24, 5), (32, 0), (32, 14)]
C_SQDIST = 4 * 125.89      # see the docstring


def _clients(K, f, n, offset=0, seed=0):
    """(xs, c, attackers); offset=1: slices 4 bytes past 16-byte alignment"""
    g = torch.Generator().manual_seed(1000 * K + 10 * f + seed)
    rn = lambda: torch.randn(n + offset, generator=g)  # noqa: E731
    c = 0.05 * rn()
    xs = [c + 0.01 * (1 + 0.05 * k) * rn() for k in range(K)]
    bad = [K - 1 - 2 * j for j in range(f)]
    for k in bad:
        xs[k] = c - 4 * (xs[k] - c) + 0.02
    return [x.cuda()[offset:] for x in xs], c.cuda()[offset:], bad


def _sqdist64(xs):
    A = torch.stack(xs).double()
    return torch.stack([((A - A[i]) ** 2).sum(1) for i in range(len(xs))])


def _check_sqdist(K, n, offset=0):
    xs, c, _ = _clients(K, 0, n, offset)
    xs0, c0 = [x.clone() for x in xs], c.clone()
    D, again = (consensus.pairwise_sqdist(xs, c) for _ in range(2))
    assert D.dtype == torch.float32 and D.shape == (K, K)
    assert torch.equal(D, D.T) and not bool(D.diagonal().any())
    assert torch.equal(D, again)
    assert torch.equal(c, c0)
    assert all(torch.equal(a, b) for a, b in zip(xs, xs0))
    sq = ((torch.stack(xs).double() - c.double()) ** 2).sum(1)
    scaled = (D.double() - _sqdist64(xs)).abs() / \
        (2.0 ** -24 * (sq[:, None] + sq[None, :]))
    print("sqdist", K, n, "scaled err", scaled.max().item())
    assert bool((scaled <= C_SQDIST).all())


@gpu
@pytest.mark.parametrize("n", [3, 65, 1029, 524295])
@pytest.mark.parametrize("K", [1, 2, 3, 10, 16, 17, 32])
def test_pairwise_sqdist(K, n):
    _check_sqdist(K, n)


@gpu
def test_pairwise_sqdist_unaligned_operands():
    _check_sqdist(17, 1029, offset=1)


@gpu
@pytest.mark.parametrize("n", [65, 1029, 524295])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("rule", consensus.KRUM_RULES)
@pytest.mark.parametrize("K,f", K_F)
def test_krum_round_matches_reference(K, f, rule, mode, n):
    xs, z, bad = _clients(K, f, n)
    m = 1 if rule == "krum" else K - f
    D = _sqdist64(xs).fill_diagonal_(math.inf)
    s = D.sort(1).values[:, :K - f - 2].sum(1).sort().values
    gap = ((s[1:] - s[:-1]) / s[1:]).min().item()
    print("krum", K, f, n, "score gap", gap)
    assert gap >= 1e-4          # a condition on the inputs
    zt, _, _ = consensus.krum_round_torch(xs, z, RHO, mode, f, m)
    _, rd, sd = consensus.krum_round_torch([x.double() for x in xs],
                                           z.double(), RHO, mode, f, m)
    znew, res, sel = consensus.krum_round(xs, z, RHO, mode, f, m)
    assert sel.dtype == torch.bool and torch.equal(sel, sd)
    assert int(sel.sum()) == m and not bool(sel[bad].any())
    assert torch.equal(znew, zt)
    assert res.dtype == torch.float32 and res.shape == rd.shape
    assert bool(((res.double() - rd).abs() <= 1e-5 * rd).all()), \
        (res.tolist(), rd.tolist())


@gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("poison", ["nan", "inf", "-inf", "1e6"])
@pytest.mark.parametrize("K,f", [(5, 1), (17, 3)])
def test_krum_round_bad_client(K, f, poison, mode):
    n, bad = 65, 2
    xs, z, _ = _clients(K, 0, n)
    xs[bad] = torch.full((n,), float(poison)).cuda()
    if poison == "nan":
        xs[bad].view(torch.int32)[1::2] |= -2 ** 31    # both sign bits
    znew, res, sel = consensus.krum_round(xs, z, RHO, mode, f)
    assert int(sel.sum()) == K - f and not bool(sel[bad])
    zt = torch.zeros_like(z)
    for k in sel.nonzero().flatten().tolist():
        zt += xs[k]
    zt /= K - f
    assert bool(znew.isfinite().all()) and torch.equal(znew, zt)
    finite = res.isfinite()
    if mode == "fedprox":
        assert bool(finite[1 + bad]) == (poison == "1e6")
        finite[1 + bad] = True
    assert bool(finite.all())


@gpu
@pytest.mark.parametrize("case", ["K33", "f", "m0", "mK1", "short_x",
                                  "strided_x", "fp64_z", "center", "rho0"])
def test_krum_round_rejects_before_launch(case):
    K, n = (33 if case == "K33" else 4), 65
    xs, z, _ = _clients(K, 0, n)
    f, m, rho, center = (2 if case == "f" else 1), 2, RHO, None
    if case in ("m0", "mK1"):
        m = 0 if case == "m0" else K + 1
    elif case == "short_x":
        xs[2] = xs[2][:-1]
    elif case == "strided_x":
        xs[2] = _clients(1, 0, 2 * n)[1][::2]
    elif case == "fp64_z":
        z = z.double()
    elif case == "center":
        center = z[:-1]
    elif case == "rho0":
        rho = 0.0
    with pytest.raises(RuntimeError):
        consensus.krum_round(xs, z, rho, "fedprox", f, m, center)
    torch.cuda.synchronize()


@gpu
@pytest.mark.parametrize("cls", [FedAvg, FedProx])
def test_krum_strategies_fused_equals_torch_sequence(cls):
    N, K = 1029, 5
    out = []
    for fused in (True, False):
        strat = cls(robust="multi_krum", trim_frac=0.2)
        strat.fused_aggregate = fused
        comm = LocalComm(K, device=torch.device("cuda"))
        state = strat.init_block(comm, N, torch.device("cuda"))
        state["z"] = _clients(K, 1, N)[1]
        infos = [strat.aggregate(comm, state,
                                 dict(enumerate(_clients(K, 1, N, seed=r)[0])),
                                 r) for r in range(2)]
        assert state["krum_selected"].tolist() == [True] * 4 + [False]
        out.append((state["z"], infos))
    (za, ia), (zb, ib) = out
    assert torch.equal(za, zb)
    for a, b in zip(ia, ib):
        assert a.keys() == b.keys()
        for key in a:
            assert float(a[key]) == pytest.approx(float(b[key]), rel=1e-5)
