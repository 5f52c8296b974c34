"""consensus.bulyan_round (csrc/bulyan.hip) against float64 and the torch
sequence that defines the round.  (K, f) covers the least K for f = 1 and 2,
the drivers' K, the Gram 16 | 17 switch, every sort bucket and the limits;
n = 3 is a tail only, 257 one tile and an element, 1029 four tiles and a unit
tail.

Inputs: test_krum_gpu.py's (centre c = 0.05 randn, honest client k =
c + 0.01 (1 + 0.05 k) randn, the f clients K-1, K-3, ... replaced by
c - 4 (x - c) + 0.02), every value rounded to a multiple of 2^-16: every fp32
subtraction of the slide and every window sum is then exact, so znew differs
from float64 by the rounding of 1 / beta and of the product, 2^-23 in all.
"""

import math

import pytest
import torch

from fedkit.algos.strategies import FedProx
from fedkit.ops import consensus
from fedkit.parallel.comm import LocalComm

gpu = pytest.mark.gpu
RHO = 0.1
MODES = ["fedavg", "fedprox"]
K_F = [(7, 1), (10, 1), (11, 2), (16, 3), (17, 3), (24, 5), (32, 7), (32, 0)]


def _clients(K, f, n, offset=0, seed=0):
    """(xs, c, attackers); offset=1: slices 4 bytes past 16-byte alignment"""
    g = torch.Generator().manual_seed(1000 * K + 10 * f + seed)
    rn = lambda: torch.randn(n + offset, generator=g)  # noqa: E731
    c = 0.05 * rn()
    xs = [c + 0.01 * (1 + 0.05 * k) * rn() for k in range(K)]
    bad = [K - 1 - 2 * j for j in range(f)]
    for k in bad:
        xs[k] = c - 4 * (xs[k] - c) + 0.02
    grid = lambda v: (torch.round(v * 65536) / 65536).cuda()[offset:]  # noqa: E731
    return [grid(x) for x in xs], grid(c), bad


@gpu
@pytest.mark.parametrize("n", [3, 257, 1029])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("K,f", K_F)
def test_bulyan_round_matches_reference(K, f, mode, n):
    # seed 0 leaves a relative score gap of 4.4e-5 at (32, 7, 1029)
    xs, z, bad = _clients(K, f, n, seed=int((K, f, n) == (32, 7, 1029)))
    A = torch.stack(xs).double()
    D = torch.stack([((A - A[i]) ** 2).sum(1) for i in range(K)])
    D.fill_diagonal_(math.inf)
    left, gap = list(range(K)), math.inf
    while len(left) > 2 * f:            # the float64 selection, pick by pick
        q = max(1, len(left) - f - 2)
        sc = D[left][:, left].sort(1).values[:, :q].sum(1)
        above = sc[sc > sc.min()]       # exact ties are allowed
        if len(above):
            gap = min(gap, float((above.min() - sc.min()) / above.min()))
        left.pop(int(sc.argsort(stable=True)[0]))
    print("bulyan", K, f, n, "score gap", gap)
    assert gap >= 1e-4                  # a condition on the inputs
    zt, _, _ = consensus.bulyan_round_torch(xs, z, RHO, mode, f)
    z64, rd, sd = consensus.bulyan_round_torch([x.double() for x in xs],
                                               z.double(), RHO, mode, f)
    assert sorted(set(range(K)) - set(left)) == sd.nonzero().flatten().tolist()
    znew, res, sel = consensus.bulyan_round(xs, z, RHO, mode, f)
    assert sel.dtype == torch.bool and torch.equal(sel, sd)
    assert int(sel.sum()) == K - 2 * f and not bool(sel[bad].any())
    assert torch.equal(znew, zt)
    assert bool(((znew.double() - z64).abs() <= 2.0 ** -22 * z64.abs()).all())
    assert res.dtype == torch.float32 and res.shape == rd.shape
    assert bool(((res.double() - rd).abs() <= 1e-5 * rd).all()), \
        (res.tolist(), rd.tolist())


@gpu
@pytest.mark.parametrize("mode", MODES)
def test_bulyan_round_off_the_grid(mode):
    g = torch.Generator().manual_seed(3)
    z, *xs = [torch.randn(1029, generator=g).cuda() for _ in range(11)]
    zt, _, st = consensus.bulyan_round_torch(xs, z, RHO, mode, 1)
    znew, _, sel = consensus.bulyan_round(xs, z, RHO, mode, 1)
    assert torch.equal(sel, st) and torch.equal(znew, zt)


@gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("poison", ["nan", "inf", "-inf", "1e6"])
@pytest.mark.parametrize("K,f", [(7, 1), (17, 3)])
def test_bulyan_round_bad_client(K, f, poison, mode):
    n, bad = 65, 2
    xs, z, _ = _clients(K, 0, n)
    xs[bad] = torch.full((n,), float(poison)).cuda()
    if poison == "nan":
        xs[bad].view(torch.int32)[1::2] |= -2 ** 31    # both sign bits
    znew, res, sel = consensus.bulyan_round(xs, z, RHO, mode, f)
    assert int(sel.sum()) == K - 2 * f and not bool(sel[bad])
    zt = consensus.bulyan_window_torch(xs, sel, f)
    assert bool(znew.isfinite().all()) and torch.equal(znew, zt)
    finite = res.isfinite()
    if mode == "fedprox":
        assert bool(finite[1 + bad]) == (poison == "1e6")
        finite[1 + bad] = True
    assert bool(finite.all())


@gpu
def test_bulyan_round_unaligned_operands():
    xs, z, _ = _clients(17, 3, 1029, offset=1)
    zt, _, st = consensus.bulyan_round_torch(xs, z, RHO, "fedprox", 3)
    znew, _, sel = consensus.bulyan_round(xs, z, RHO, "fedprox", 3)
    assert torch.equal(sel, st) and torch.equal(znew, zt)


@gpu
@pytest.mark.parametrize("case", ["K33", "f", "short_x", "strided_x",
                                  "fp64_z", "center", "rho0"])
def test_bulyan_round_rejects_before_launch(case):
    K, n = (33 if case == "K33" else 7), 65
    xs, z, _ = _clients(K, 0, n)
    f, rho, center = 1, RHO, None
    if case == "f":
        xs = xs[:6]                     # K = 4 f + 2
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
        consensus.bulyan_round(xs, z, rho, "fedprox", f, center)
    torch.cuda.synchronize()


@gpu
def test_bulyan_strategy_fused_equals_torch_sequence():
    N, K = 1029, 7
    out = []
    for fused in (True, False):
        strat = FedProx(robust="bulyan", trim_frac=0.15)
        strat.fused_aggregate = fused
        comm = LocalComm(K, device=torch.device("cuda"))
        state = strat.init_block(comm, N, torch.device("cuda"))
        state["z"] = _clients(K, 1, N)[1]
        infos = [strat.aggregate(comm, state,
                                 dict(enumerate(_clients(K, 1, N, seed=r)[0])),
                                 r) for r in range(2)]
        sel = state["bulyan_selected"]
        assert int(sel.sum()) == 5 and not bool(sel[K - 1])
        out.append((state["z"], infos, sel))
    (za, ia, sa), (zb, ib, sb) = out
    assert torch.equal(za, zb) and torch.equal(sa, sb)
    for a, b in zip(ia, ib):
        assert a.keys() == b.keys()
        for key in a:
            assert float(a[key]) == pytest.approx(float(b[key]), rel=1e-5)
