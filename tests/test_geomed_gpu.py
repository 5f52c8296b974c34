"""consensus.geomed_round (csrc/geomed.hip) against geomed_round_torch on
float64 copies and the torch sequence that defines znew.  K covers both MFMA
shapes, the 8 | 9 and 16 | 17 bucket boundaries and the limits; n = 3 is a
tail only, 65 under one tile, 1029 = 4 * 256 + 5 the tile and wave-share
boundaries, 524295 a second grid-stride trip that ends in a tail.

Inputs: the recipe of test_krum_gpu.py: centre c = 0.05 randn, honest client
k = c + 0.01 (1 + 0.05 k) randn, the f clients K-1, K-3, ... replaced by
c - 4 (x - c) + 0.02.

Weight bound |c - c64| <= T max(c64): T is 4 x the largest such error of the
float64 Gram-space solver fed torch's own fp32 A @ A.T of the centred stack,
over the grid of the main test on the MI355X (the two accumulation orders
differ).  Measured: torch 1.022e-6 (3.7e-7..1.02e-6 at n = 524295, at most
1.75e-7 at the smaller n), the kernel 1.73e-7 (K = 5, n = 3; at most 1.19e-7
elsewhere).
"""

import pytest
import torch

from fedkit import ops
from fedkit.algos.strategies import FedAvg, FedProx
from fedkit.ops import consensus
from fedkit.parallel.comm import LocalComm

gpu = pytest.mark.gpu
RHO = 0.1
MODES = ["fedavg", "fedprox"]
K_F = [(1, 0), (2, 0), (5, 1), (8, 2), (9, 2), (16, 3), (17, 7), (32, 0),
       (32, 14)]
T_WEIGHTS = 4 * 1.022e-6      # see the docstring


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


def _native(xs, z, mode, rho=RHO, iters=16, nu=1e-3):
    """(znew, res, c, keep, d) of the extension"""
    return ops.require_ext().geomed_round(xs, z, rho, MODES.index(mode), iters,
                                          nu)


def _sequence(xs, z, c, keep):
    zt = z.clone()
    for k in keep.nonzero().flatten().tolist():
        zt += c[k] * (xs[k] - z)
    return zt


def _bits_equal(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def _check_round(K, f, mode, n, offset=0):
    xs, z, _ = _clients(K, f, n, offset)
    xs0, z0 = [x.clone() for x in xs], z.clone()
    znew, res, c = consensus.geomed_round(xs, z, RHO, mode)
    again = _native(xs, z, mode)
    keep = again[3]
    assert all(torch.equal(a, b) for a, b in zip((znew, res, c), again))
    assert torch.equal(z, z0)
    assert all(torch.equal(a, b) for a, b in zip(xs, xs0))
    assert keep.dtype == torch.int32 and keep.shape == (K,) and bool(keep.all())
    assert c.dtype == torch.float32 and c.shape == (K,)
    assert _bits_equal(znew, _sequence(xs, z, c, keep))
    c64 = consensus.geomed_round_torch([x.double() for x in xs],
                                       z.double())[2]
    err = ((c.double() - c64).abs().max() / c64.max()).item()
    print("geomed", K, f, mode, n, "weight err", err)
    assert err <= T_WEIGHTS
    r64 = [((z.double() - znew.double()) ** 2).sum()]
    if mode == "fedprox":
        r64 += [((RHO * (x.double() - znew.double())) ** 2).sum() for x in xs]
    r64 = torch.stack(r64)
    assert res.dtype == torch.float32 and res.shape == r64.shape
    assert bool(((res.double() - r64).abs() <= 1e-5 * r64).all()), \
        (res.tolist(), r64.tolist())


@gpu
@pytest.mark.parametrize("n", [3, 65, 1029, 524295])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("K,f", K_F)
def test_geomed_round_matches_reference(K, f, mode, n):
    _check_round(K, f, mode, n)


@gpu
def test_geomed_round_unaligned_operands():
    _check_round(17, 7, "fedprox", 1029, offset=1)


@gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("poison", ["nan", "inf", "-inf", "1e6"])
@pytest.mark.parametrize("K,f", [(5, 1), (17, 7)])
def test_geomed_round_bad_client(K, f, poison, mode):
    n = 65
    xs, z, _ = _clients(K, 0, n)
    bad = [K - 1 - 2 * j for j in range(f)]
    for k in bad:
        xs[k] = torch.full((n,), float(poison)).cuda()
        if poison == "nan":
            xs[k].view(torch.int32)[1::2] |= -2 ** 31    # both sign bits
    good = [k for k in range(K) if k not in bad]
    znew, res, c, keep, _ = _native(xs, z, mode)
    assert bool(keep[good].all())
    if poison != "1e6":
        assert not bool(keep[bad].any()) and not bool(c[bad].any())
    assert bool(znew.isfinite().all())
    assert _bits_equal(znew, _sequence(xs, z, c, keep))
    if poison == "1e6":     # the geometric median's breakdown bound
        H = torch.stack([xs[k] for k in good]).double()
        spread = (H - H.mean(0)).norm(dim=1).max()
        dist = (znew.double() - H.mean(0)).norm()
        print("geomed", K, f, mode, "dist / spread", (dist / spread).item())
        assert dist <= 2 * (K - f) / (K - 2 * f) * spread
    finite = res.isfinite()
    if mode == "fedprox":
        at = [1 + k for k in bad]
        assert finite[at].tolist() == [poison == "1e6"] * f
        finite[at] = True
    assert bool(finite.all())


@gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", ["at_z", "neg_zero_K1", "neg_zero_K5"])
def test_geomed_round_degenerate(case, mode):
    """neg_zero: a skipped NaN client must not turn z's -0.0 into +0.0.
    The first kept client's term does that in any case (-0.0 + +0.0 is
    +0.0, and x - z is never -0.0 where z is), so the sign shows only where
    no client is kept: one NaN client of one, and five of five, which takes
    the masked step of fedprox five times."""
    K, n = (1 if case == "neg_zero_K1" else 5), 65
    xs, z, _ = _clients(K, 0, n)
    if case == "at_z":
        xs = [z.clone() for _ in range(K)]
    else:
        z[::2] = -0.0
        xs = [torch.full_like(z, float("nan")) for _ in range(K)]
    znew, _, c, keep, _ = _native(xs, z, mode)
    assert keep.tolist() == [int(case == "at_z")] * K
    assert _bits_equal(znew, _sequence(xs, z, c, keep))
    assert _bits_equal(znew, z)
    if case == "at_z":
        assert torch.equal(c.cpu(), torch.full((K,), 1 / K))
    else:
        assert not bool(c.any())


@gpu
@pytest.mark.parametrize("case", ["K33", "short_x", "strided_x", "fp64_z",
                                  "iters0", "nu0", "rho0", "admm"])
def test_geomed_round_rejects_before_launch(case):
    K, n = (33 if case == "K33" else 4), 65
    xs, z, _ = _clients(K, 0, n)
    mode, kw = ("admm" if case == "admm" else "fedprox"), {}
    if case == "short_x":
        xs[2] = xs[2][:-1]
    elif case == "strided_x":
        xs[2] = _clients(1, 0, 2 * n)[1][::2]
    elif case == "fp64_z":
        z = z.double()
    elif case == "iters0":
        kw = {"iters": 0}
    elif case == "nu0":
        kw = {"nu": 0.0}
    with pytest.raises(RuntimeError):
        consensus.geomed_round(xs, z, 0.0 if case == "rho0" else RHO, mode,
                               **kw)
    torch.cuda.synchronize()


@gpu
@pytest.mark.parametrize("cls", [FedAvg, FedProx])
def test_geomed_strategies_fused_matches_torch_sequence(cls):
    """z of the two paths to the tolerance T of the weights, relative to the
    largest |z|; the weights themselves to T of the largest weight."""
    N, K = 1029, 5
    out = []
    for fused in (True, False):
        strat = cls(robust="geomed")
        strat.fused_aggregate = fused
        comm = LocalComm(K, device=torch.device("cuda"))
        state = strat.init_block(comm, N, torch.device("cuda"))
        state["z"] = _clients(K, 1, N)[1]
        infos = [strat.aggregate(comm, state,
                                 dict(enumerate(_clients(K, 1, N, seed=r)[0])),
                                 r) for r in range(2)]
        out.append((state["z"], state["geomed_weights"], infos))
    (za, ca, ia), (zb, cb, ib) = out
    assert float((ca - cb).abs().max()) <= T_WEIGHTS * float(cb.max())
    assert float((za - zb).abs().max()) <= T_WEIGHTS * float(zb.abs().max())
    for a, b in zip(ia, ib):
        assert a.keys() == b.keys()
        for key in a:
            assert float(a[key]) == pytest.approx(float(b[key]), rel=1e-5)
