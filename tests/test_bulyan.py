"""Bulyan on the CPU: consensus.bulyan_round_torch against a plain
per-coordinate Python statement of the rule in float64, its parameters, and
the way from the flag to the strategies."""

import pytest
import torch

from fedkit.algos.strategies import FedAvg, FedProx
from fedkit.ops import consensus
from fedkit.parallel.comm import LocalComm
from fedkit.parallel.runtime import FedConfig
from fedkit.utils.cli import config_from_cli


def _clients(K, f, n, seed=0):
    """(xs, c, attackers) in float64, the recipe of test_krum_gpu.py"""
    g = torch.Generator().manual_seed(1000 * K + 10 * f + seed)
    rn = lambda: torch.randn(n, generator=g, dtype=torch.float64)  # noqa: E731
    c = 0.05 * rn()
    xs = [c + 0.01 * (1 + 0.05 * k) * rn() for k in range(K)]
    bad = [K - 1 - 2 * j for j in range(f)]
    for k in bad:
        xs[k] = c - 4 * (xs[k] - c) + 0.02
    return xs, c, bad


@pytest.mark.parametrize("K,f", [(7, 1), (11, 2)])
def test_torch_sequence_is_the_rule(K, f):
    n, theta, beta = 33, K - 2 * f, K - 4 * f
    xs, z, bad = _clients(K, f, n)
    znew, res, sel = consensus.bulyan_round_torch(xs, z, 0.1, "fedprox", f)
    D = [[float(((a - b) ** 2).sum()) for b in xs] for a in xs]
    left, picked = list(range(K)), []
    while len(picked) < theta:
        q = max(1, len(left) - f - 2)
        score = {i: sum(sorted(D[i][j] for j in left if j != i)[:q])
                 for i in left}
        picked.append(min(left, key=lambda i: (score[i], i)))
        left.remove(picked[-1])
    assert sel.nonzero().flatten().tolist() == sorted(picked)
    assert not set(picked) & set(bad)
    for e in range(n):
        s = sorted(float(xs[k][e]) for k in picked)
        med = s[(theta - 1) // 2]
        near = sorted(range(theta), key=lambda r: (abs(s[r] - med), r))[:beta]
        want = sum(s[r] for r in near) / beta
        assert abs(float(znew[e]) - want) <= 1e-12 * abs(want)
    assert res.shape == (1 + K,)
    assert float(res[0]) == pytest.approx(float(((z - znew) ** 2).sum()))


def test_params():
    assert consensus.bulyan_params(0.15, 7) == (1, 5, 3)
    assert consensus.bulyan_params(0.0, 3) == (0, 3, 3)
    with pytest.raises(ValueError):
        consensus.bulyan_params(0.2, 10)        # f = 2: K = 4 f + 2
    with pytest.raises(ValueError):
        consensus.bulyan_round(_clients(6, 1, 9)[0], torch.zeros(9), f=1)


def test_flag_reaches_the_strategies():
    cfg = config_from_cli(FedConfig(strategy="fedprox"),
                          ["--robust_agg", "bulyan", "--trim_frac", "0.15"])
    strat = cfg.make_strategy()
    assert (type(strat), strat.robust) == (FedProx, "bulyan")
    with pytest.raises(ValueError):
        config_from_cli(FedConfig(strategy="admm"),
                        ["--robust_agg", "bulyan"]).make_strategy()
    K, n = 7, 65
    xs, z, bad = _clients(K, 1, n)
    xs, z = [x.float() for x in xs], z.float()
    strat = FedAvg(robust="bulyan", trim_frac=0.15)
    comm = LocalComm(K, device=torch.device("cpu"))
    state = strat.init_block(comm, n, torch.device("cpu"))
    state["z"] = z
    strat.aggregate(comm, state, dict(enumerate(xs)), 0)
    want, _, sel = consensus.bulyan_round(xs, z, None, "fedavg", 1)
    assert torch.equal(state["z"], want)
    assert torch.equal(state["bulyan_selected"], sel)
    assert int(sel.sum()) == 5 and not bool(sel[bad].any())
