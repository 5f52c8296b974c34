"""Geometric-median (RFA) aggregation through the strategies and the
configuration flags, on the CPU."""

import pytest
import torch

from fedkit.algos.strategies import FedAvg, FedProx
from fedkit.ops import consensus
from fedkit.parallel.comm import LocalComm
from fedkit.parallel.runtime import FedConfig
from fedkit.utils.cli import config_from_cli


def _vec(n, seed):
    return torch.randn(n, generator=torch.Generator().manual_seed(seed)) * 0.05


def _round(strat, x):
    comm = LocalComm(len(x), device=torch.device("cpu"))
    state = strat.init_block(comm, x[0].numel(), torch.device("cpu"))
    strat.aggregate(comm, state, x, 0)
    return state


@pytest.mark.parametrize("poison", [1e6, float("nan")])
def test_geomed_survives_one_bad_client(poison):
    """z stays within the breakdown bound 2 (K - f) / (K - 2 f) times the
    honest spread of the honest mean; the plain mean does not."""
    N, K, bad = 257, 5, 2
    x = {k: _vec(N, k) for k in range(K)}
    x[bad] = torch.full((N,), poison)
    honest = torch.stack([x[k] for k in range(K) if k != bad])
    centre = honest.mean(0)
    bound = 2 * (K - 1) / (K - 2) * (honest - centre).norm(dim=1).max()
    state = _round(FedAvg(robust="geomed"), x)
    c = state["geomed_weights"]
    assert float(c.sum()) == pytest.approx(1.0, abs=1e-6)
    assert float(c[bad]) < 1e-3
    assert float((state["z"] - centre).norm()) <= float(bound)
    assert not float((_round(FedAvg(), x)["z"] - centre).norm()) <= float(bound)


def test_geomed_flags_reach_the_strategy():
    cfg = config_from_cli(FedConfig(strategy="fedprox"),
                          ["--robust_agg", "geomed", "--geomed_iters", "8"])
    strat = cfg.make_strategy()
    assert isinstance(strat, FedProx)
    assert (strat.robust, strat.geomed_iters) == ("geomed", 8)


def test_geomed_refusals():
    cfg = config_from_cli(FedConfig(strategy="admm"), ["--robust_agg", "geomed"])
    with pytest.raises(ValueError):
        cfg.make_strategy()
    xs = [_vec(9, k) for k in range(4)]
    with pytest.raises(ValueError):
        consensus.geomed_round(xs, xs[0], 0.1, "admm")
    with pytest.raises(ValueError):
        consensus.geomed_round(xs, xs[0], iters=0)
