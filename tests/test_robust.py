"""Robust aggregation (trimmed mean / median) through the strategies, the
configuration flags and the distributed gather, on the CPU."""

import os

import pytest
import torch

from fedkit.algos.strategies import FedAvg, FedProx
from fedkit.parallel.comm import LocalComm
from fedkit.parallel.runtime import FedConfig
from fedkit.utils.cli import config_from_cli

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _vec(n, seed):
    return torch.randn(n, generator=torch.Generator().manual_seed(seed)) * 0.05


@pytest.mark.parametrize("poison", [1e6, float("nan")])
def test_median_survives_one_bad_client(poison):
    N, K, bad = 257, 5, 2
    x = {k: _vec(N, k) for k in range(K)}
    x[bad] = torch.full((N,), poison)
    honest = torch.stack([x[k] for k in range(K) if k != bad])
    lo, hi = honest.amin(0), honest.amax(0)
    z = {}
    for robust in (None, "median"):
        strat = FedAvg(robust=robust)
        comm = LocalComm(K, device=torch.device("cpu"))
        state = strat.init_block(comm, N, torch.device("cpu"))
        strat.aggregate(comm, state, x, 0)
        z[robust] = state["z"]
    assert bool(((z["median"] >= lo) & (z["median"] <= hi)).all())
    assert not bool(((z[None] >= lo) & (z[None] <= hi)).any())


def test_robust_flags_reach_the_strategy():
    assert FedConfig().make_strategy().robust is None
    cfg = config_from_cli(FedConfig(strategy="fedprox"),
                          ["--robust_agg", "trimmed_mean", "--trim_frac", "0.2"])
    strat = cfg.make_strategy()
    assert isinstance(strat, FedProx)
    assert (strat.robust, strat.trim_frac) == ("trimmed_mean", 0.2)
    cfg = config_from_cli(FedConfig(strategy="admm"), ["--robust_agg", "median"])
    with pytest.raises(ValueError):
        cfg.make_strategy()


def two_rounds(comm):
    """z of a FedAvg and a FedProx block after two median rounds; a rank
    builds only its own clients' vectors, from seeds"""
    out = []
    for strat in (FedAvg(robust="median"), FedProx(rho0=0.5, robust="median")):
        state = strat.init_block(comm, 1029, torch.device("cpu"))
        for r in range(2):
            x = {ck: _vec(1029, 10 * r + ck) for ck in comm.my_clients}
            strat.aggregate(comm, state, x, r)
        out.append(state["z"])
    return out


WORKER = r"""
import os, sys
sys.path[:0] = [%r, %r]
import torch
from fedkit.parallel.comm import DistComm
from test_robust import two_rounds
comm = DistComm(2, backend="gloo")
torch.save(two_rounds(comm), os.path.join(sys.argv[1], f"z{comm.rank}.pt"))
"""


def test_robust_gloo_world2_equals_local(tmp_path):
    from test_dist_gloo import run_torchrun
    run_torchrun(WORKER % (REPO, os.path.join(REPO, "tests")), str(tmp_path))
    local = two_rounds(LocalComm(2, device=torch.device("cpu")))
    for rank in range(2):
        dist = torch.load(tmp_path / f"z{rank}.pt", weights_only=False)
        assert all(torch.equal(a, b) for a, b in zip(dist, local))
