"""Centred clipping with bucketing on the CPU, and the inputs (the recipe of
test_geomed_gpu.py) and grid that test_cclip_gpu.py shares.  The fixed tau is
1.5 x the honest spread of the bucket means: the largest honest |x_k - c| over
sqrt(s).  Three iterations, one for K = 2: at the iteration's fixed point two
buckets are both clipped or both unclipped, and an honest pair is there at the
second step, while the first splits them at the auto radius.  Every case with
B >= 2 buckets then has a clipped and an unclipped bucket in the last step of
the float64 rule; B = 1 (K = 1; K = 2 with s = 2) cannot."""

import pytest
import torch

from fedkit.algos.strategies import FedAvg, FedProx
from fedkit.ops import consensus
from fedkit.parallel.comm import LocalComm
from fedkit.parallel.runtime import FedConfig
from fedkit.utils.cli import config_from_cli

K_F = [(1, 0), (2, 0), (5, 1), (8, 2), (9, 2), (16, 3), (17, 7), (32, 14)]
SOLVES = [(1, "auto"), (2, "auto"), (3, "fixed")]
CASES = [(K, f, s, kind) for K, f in K_F for s, kind in SOLVES if s <= K]
SIZES = [3, 65, 1029, 524295]


def clients(K, f, n, offset=0, seed=0):
    """(xs, c, attackers); offset=1: slices 4 bytes past 16-byte alignment"""
    g = torch.Generator().manual_seed(1000 * K + 10 * f + seed)
    rn = lambda: torch.randn(n + offset, generator=g)  # noqa: E731
    c = 0.05 * rn()
    xs = [c + 0.01 * (1 + 0.05 * k) * rn() for k in range(K)]
    bad = [K - 1 - 2 * j for j in range(f)]
    for k in bad:
        xs[k] = c - 4 * (xs[k] - c) + 0.02
    return [x[offset:] for x in xs], c[offset:], bad


def solve_args(xs, z, bad, s, kind):
    """(iters, tau, bucket, perm) of a grid case"""
    K = len(xs)
    spread = max((xs[k].double() - z.double()).norm().item()
                 for k in range(K) if k not in bad) / s ** 0.5
    perm = None
    if s > 1:
        g = torch.Generator().manual_seed(10 * K + s)
        perm = torch.randperm(K, generator=g).tolist()
        if perm == list(range(K)):
            perm.reverse()
    return (1 if K == 2 else 3, 1.5 * spread if kind == "fixed" else 0.0, s,
            perm)


def solve64(xs, z, args):
    """float64 rule: w; a clipped and an unclipped bucket at the end, or B = 1"""
    w, _, sb, _ = consensus.cclip_solve_torch([x.double() for x in xs],
                                              z.double(), *args)
    return w, len(sb) == 1 or bool((sb < 1).any() and (sb == 1).any())


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("K,f,s,kind", CASES)
def test_grid_cases_clip_and_pass(K, f, s, kind, n):
    xs, z, bad = clients(K, f, n)
    assert solve64(xs, z, solve_args(xs, z, bad, s, kind))[1]


def _direct(xs, z, iters, tau, s, perm):
    """the rule on explicit bucket-mean vectors"""
    A = torch.stack(xs) - z
    order = [k for k in perm if bool((A[k] ** 2).sum().isfinite())]
    U = torch.stack([A[order[i:i + s]].mean(0)
                     for i in range(0, len(order), s)])
    t = tau if tau > 0 else U.norm(dim=1).sort().values[(len(U) - 1) // 2]
    v = torch.zeros_like(z)
    for _ in range(iters):
        d = (U - v).norm(dim=1)
        sb = torch.where(d > t, t / d, torch.ones_like(d))
        v = v + (sb[:, None] * (U - v)).mean(0)
    return z + v


@pytest.mark.parametrize("tau", [0.0, 0.12])
@pytest.mark.parametrize("nan_at", [None, 4])    # 4: inside a bucket
@pytest.mark.parametrize("shuffled", [False, True])
@pytest.mark.parametrize("s", [1, 2, 3])
def test_torch_sequence_is_the_rule(s, shuffled, nan_at, tau):
    """K' = 7 (divisible by neither 2 nor 3) or 6 with the NaN client"""
    K = 7
    xs, z, _ = clients(K, 2, 33)
    xs, z = [x.double() for x in xs], z.double()
    if nan_at is not None:
        xs[nan_at] = torch.full_like(z, float("nan"))
    perm = [3, 0, 4, 6, 1, 5, 2] if shuffled else list(range(K))
    znew, res, w = consensus.cclip_round_torch(
        xs, z, 0.1, "fedprox", 4, tau, s, perm if shuffled else None)
    want = _direct(xs, z, 4, tau, s, perm)
    assert float((znew - want).abs().max()) <= 1e-12 * float(want.abs().max())
    assert res.shape == (1 + K,)
    assert nan_at is None or float(w[nan_at]) == 0.0


@pytest.mark.parametrize("tau", [0.0, 0.05])
@pytest.mark.parametrize("s", [1, 2])
def test_radius_bounds_the_move(s, tau):
    iters = 5
    xs, z, _ = clients(6, 0, 65)
    xs, z = [x.double() for x in xs], z.double()
    xs[2] = torch.full_like(z, 1e6)
    znew = consensus.cclip_round_torch(xs, z, None, "fedavg", iters, tau, s)[0]
    used = consensus.cclip_solve_torch(xs, z, iters, tau, s)[3]
    assert 0 < float((znew - z).norm()) <= iters * float(used) * (1 + 1e-6)


def test_flags_reach_the_strategies_and_fill_the_weights():
    cfg = config_from_cli(FedConfig(strategy="fedprox"),
                          ["--robust_agg", "cclip", "--cclip_iters", "2",
                           "--cclip_tau", "0.5", "--agg_bucket", "2"])
    strat = cfg.make_strategy()
    assert (type(strat), strat.robust, strat.cclip_iters, strat.cclip_tau,
            strat.agg_bucket, strat.agg_seed) == (FedProx, "cclip", 2, 0.5, 2,
                                                  cfg.seed)
    K, n = 5, 65
    for strat in (strat, FedAvg(robust="cclip", agg_bucket=2)):
        comm = LocalComm(K, device=torch.device("cpu"))
        state = strat.init_block(comm, n, torch.device("cpu"))
        for r in range(2):
            strat.aggregate(comm, state, dict(enumerate(clients(K, 1, n)[0])),
                            r)
        assert state["cclip_weights"].shape == (K,)
        assert not torch.equal(strat._bucket_perm(K, 0),
                               strat._bucket_perm(K, 1))


@pytest.mark.parametrize("kw", [{"iters": 0}, {"iters": 1025}, {"tau": -1.0},
                                {"tau": float("inf")}, {"bucket": 0},
                                {"bucket": 5}, {"perm": [0, 1, 2]},
                                {"perm": [0, 1, 2, 2]}, {"mode": "admm"}])
def test_bad_arguments_raise(kw):
    xs, z, _ = clients(4, 0, 9)
    with pytest.raises(ValueError):
        consensus.cclip_round(xs, z, **{"rho": 0.1, **kw})
    with pytest.raises(ValueError):     # bucketing is for cclip only
        FedAvg(robust="geomed", agg_bucket=2)
    with pytest.raises(ValueError):
        config_from_cli(FedConfig(strategy="admm"),
                        ["--robust_agg", "cclip"]).make_strategy()
