"""consensus.robust_round (csrc/robust.hip) against the torch sequence that
defines it: bitwise in fp32 on the same device, and within the rounding of
an m-term fp32 sum of the same sequence in float64.  K covers every network
bucket, the unit-width boundary (16 | 17) and the limits 1 and 32; n = 3 is
a tail only, 65 is 16 units + 1 element, 524295 = 512*256*4 + 7 a second
grid-stride trip that still ends in a tail.
"""

import pytest
import torch

from fedkit.algos.strategies import FedAvg, FedProx
from fedkit.ops import consensus
from fedkit.parallel.comm import LocalComm

gpu = pytest.mark.gpu
RHO = 0.1
MODES = ["fedavg", "fedprox"]
K_TRIM = [(K, t) for K in [1, 2, 3, 4, 5, 10, 16, 17, 32]
          for t in sorted({0, 1, (K - 1) // 2}) if 2 * t < K]


def _vecs(count, n, seed, offset=0):
    """offset=1: slices 4 bytes past the 16-byte alignment of their buffers"""
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(n + offset, generator=g) * 0.05).cuda()[offset:]
            for _ in range(count)]


def _check_round(mode, K, trim, n, offset=0):
    xs, z = _vecs(K, n, 1, offset), _vecs(1, n, 3, offset)[0]
    xs0, z0 = [x.clone() for x in xs], z.clone()
    zt, _ = consensus.robust_round_torch(xs, z, RHO, mode, trim)
    zd, rd = consensus.robust_round_torch([x.double() for x in xs],
                                          z.double(), RHO, mode, trim)
    (znew, res), again = (consensus.robust_round(xs, z, RHO, mode, trim)
                          for _ in range(2))
    assert torch.equal(znew, zt)
    # an m-term fp32 sum and the scale: m + 1 roundings of at most max |x_k|
    bound = (K - 2 * trim + 1) * 2.0 ** -24 * \
        torch.stack(xs).abs().amax(0).double()
    assert bool(((znew.double() - zd).abs() <= bound).all())
    assert res.dtype == torch.float32 and res.shape == rd.shape
    err = (res.double() - rd).abs()
    print(mode, K, trim, n, "res rel err", (err / rd).max().item())
    assert bool((err <= 1e-5 * rd).all()), (res.tolist(), rd.tolist())
    assert torch.equal(z, z0)
    assert all(torch.equal(a, b) for a, b in zip(xs, xs0))
    assert torch.equal(again[0], znew) and torch.equal(again[1], res)


@gpu
@pytest.mark.parametrize("n", [3, 65, 524295])
@pytest.mark.parametrize("K,trim", K_TRIM)
@pytest.mark.parametrize("mode", MODES)
def test_robust_round_matches_torch_sequence(mode, K, trim, n):
    _check_round(mode, K, trim, n)


@gpu
@pytest.mark.parametrize("mode", MODES)
def test_robust_round_unaligned_operands(mode):
    _check_round(mode, 5, 1, 65, offset=1)


@gpu
@pytest.mark.parametrize("bad", ["inf", "nan", "nans"])
@pytest.mark.parametrize("K,trim", [(5, 1), (5, 2), (17, 1), (17, 8)])
def test_robust_round_order_semantics(K, trim, bad):
    """Three levels, so ties dominate, with both zeros; then +inf and -inf
    clients, a NaN client (both sign bits), or trim + 1 clients that are NaN
    from element 8 j on: the first 8 trim elements stay finite."""
    n = 65
    g = torch.Generator().manual_seed(7)
    xs = []
    for _ in range(K):
        q = torch.randint(-1, 2, (n,), generator=g).float() * 0.05
        xs.append(torch.where(torch.rand(n, generator=g) < 0.5, -q, q).cuda())
    nan = torch.full((n,), float("nan"))
    nan.view(torch.int32)[1::2] |= -2 ** 31
    if bad == "inf":
        xs[0], xs[1] = torch.full_like(xs[0], float("inf")), \
            torch.full_like(xs[1], float("-inf"))
    for j in range({"inf": 0, "nan": 1, "nans": trim + 1}[bad]):
        xs[K - 1 - 2 * j][8 * j:] = nan.cuda()[8 * j:]
    z = _vecs(1, n, 3)[0]
    zt, _ = consensus.robust_round_torch(xs, z, RHO, "fedprox", trim)
    znew, _ = consensus.robust_round(xs, z, RHO, "fedprox", trim)
    mask = zt.isnan()
    assert bool(mask.any()) == (bad == "nans")
    assert not bool(mask[:8 * trim].any())
    assert torch.equal(znew.isnan(), mask)
    assert torch.equal(znew[~mask], zt[~mask])
    assert bool(znew[~mask].isfinite().all())


@gpu
@pytest.mark.parametrize("case", ["K33", "trim", "short_x", "strided_x",
                                  "fp64_z", "rho0"])
def test_robust_round_rejects_before_launch(case):
    K, n, rho = (33 if case == "K33" else 4), 65, (0.0 if case == "rho0" else RHO)
    xs, z, trim = _vecs(K, n, 1), _vecs(1, n, 3)[0], (2 if case == "trim" else 1)
    if case == "short_x":
        xs[2] = xs[2][:-1]
    elif case == "strided_x":
        xs[2] = _vecs(1, 2 * n, 4)[0][::2]
    elif case == "fp64_z":
        z = z.double()
    with pytest.raises(RuntimeError):
        consensus.robust_round(xs, z, rho, "fedprox", trim)
    torch.cuda.synchronize()


@gpu
@pytest.mark.parametrize("cls", [FedAvg, FedProx])
def test_robust_strategies_fused_equals_torch_sequence(cls):
    N, K = 1029, 3
    out = []
    for fused in (True, False):
        strat = cls(robust="median")
        strat.fused_aggregate = fused
        comm = LocalComm(K, device=torch.device("cuda"))
        state = strat.init_block(comm, N, torch.device("cuda"))
        state["z"] = _vecs(1, N, 10)[0]
        infos = [strat.aggregate(comm, state,
                                 dict(enumerate(_vecs(K, N, 20 + r))), r)
                 for r in range(2)]
        out.append((state["z"], infos))
    (za, ia), (zb, ib) = out
    assert torch.equal(za, zb)
    for a, b in zip(ia, ib):
        assert a.keys() == b.keys()
        for key in a:
            assert float(a[key]) == pytest.approx(float(b[key]), rel=1e-5)
