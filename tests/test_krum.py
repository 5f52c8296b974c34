"""Krum / Multi-Krum aggregation through the strategies and the configuration
flags, on the CPU."""

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
def test_multi_krum_survives_one_bad_client(poison):
    N, K, bad = 257, 5, 2
    x = {k: _vec(N, k) for k in range(K)}
    x[bad] = torch.full((N,), poison)
    honest = torch.stack([x[k] for k in range(K) if k != bad])
    lo, hi = honest.amin(0), honest.amax(0)
    state = _round(FedAvg(robust="multi_krum", trim_frac=0.2), x)
    z, mean = state["z"], _round(FedAvg(), x)["z"]
    assert state["krum_selected"].tolist() == [k != bad for k in range(K)]
    assert bool(((z >= lo) & (z <= hi)).all())
    assert not bool(((mean >= lo) & (mean <= hi)).any())


def test_krum_keeps_one_honest_client():
    x = {k: _vec(65, k) for k in range(6)}
    x[5] = -4 * x[5] + 0.02
    state = _round(FedProx(rho0=0.5, robust="krum", trim_frac=0.2), x)
    sel = state["krum_selected"].tolist()
    assert sum(sel) == 1 and not sel[5]
    assert torch.equal(state["z"], x[sel.index(True)])


def test_krum_flags_reach_the_strategy():
    cfg = config_from_cli(FedConfig(strategy="fedprox"),
                          ["--robust_agg", "krum", "--trim_frac", "0.2"])
    strat = cfg.make_strategy()
    assert isinstance(strat, FedProx)
    assert (strat.robust, strat.trim_frac) == ("krum", 0.2)
    assert consensus.krum_params("krum", 0.2, 10) == (2, 1)
    assert consensus.krum_params("multi_krum", 0.2, 10) == (2, 8)


def test_krum_refusals():
    cfg = config_from_cli(FedConfig(strategy="admm"),
                          ["--robust_agg", "multi_krum"])
    with pytest.raises(ValueError):
        cfg.make_strategy()
    xs = [_vec(9, k) for k in range(4)]
    with pytest.raises(ValueError):
        consensus.krum_round(xs, xs[0], 0.1, "admm", 1)
    with pytest.raises(ValueError):             # K - f - 2 = 0
        consensus.krum_round(xs, xs[0], f=2)
    with pytest.raises(ValueError):
        consensus.krum_params("krum", 0.5, 4)
    with pytest.raises(ValueError):
        _round(FedAvg(robust="krum", trim_frac=0.4), dict(enumerate(xs[:3])))
