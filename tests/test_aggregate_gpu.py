"""Fused aggregation round (consensus.aggregate_round, csrc/consensus.hip)
against the torch sequence the strategies run without it: bitwise in fp32 on
the same device, and within fp32 rounding of the same sequence in float64.

Inputs are parameter-sized (randn * 0.05).  K covers both sides of the
register / LDS boundary (16 | 17) and the table limit 32; n = 3 is a tail
only, 65 is 16 units + 1 element, 524295 = 512*256*4 + 7 makes a workgroup
take a second grid-stride trip and still end in a tail.
"""

import pytest
import torch

from fedkit.algos.strategies import ConsensusADMM, FedAvg, FedProx
from fedkit.ops import consensus
from fedkit.parallel.comm import LocalComm

gpu = pytest.mark.gpu
RHO = 0.1
MODES = ["fedavg", "fedprox", "admm"]
K_REG_MAX = 16


def _vecs(count, n, dev, seed, offset=0):
    """`count` vectors of n elements; offset=1: slices 4 bytes past the
    16-byte alignment of their buffers."""
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(n + offset, generator=g) * 0.05).to(dev)[offset:]
            for _ in range(count)]


def _torch_round(xs, z, ys, rho, mode):
    """The strategies' expression sequence; returns (znew, new ys, squared
    residual norms) in the dtype of the operands, which are not modified."""
    K = len(xs)
    contrib = [y + rho * x for x, y in zip(xs, ys)] if mode == "admm" else xs
    znew = torch.zeros_like(contrib[0])
    for c in contrib:
        znew += c
    znew /= (K * rho) if mode == "admm" else K
    res = [(z - znew).square().sum()]
    ynew = []
    for k, x in enumerate(xs if mode != "fedavg" else []):
        ydelta = rho * (x - znew)
        res.append(ydelta.square().sum())
        if mode == "admm":
            ynew.append(ys[k] + ydelta)
    return znew, ynew, torch.stack(res)


def _check_round(mode, K, n, offset=0):
    xs = _vecs(K, n, "cuda", 1, offset)
    ys = _vecs(K, n, "cuda", 2, offset) if mode == "admm" else []
    z = _vecs(1, n, "cuda", 3, offset)[0]
    xs0, z0 = [x.clone() for x in xs], z.clone()
    zt, yt, _ = _torch_round(xs, z, ys, RHO, mode)
    zd, yd, rd = _torch_round([x.double() for x in xs], z.double(),
                              [y.double() for y in ys], RHO, mode)
    runs = []
    for _ in range(2):
        yk = [y.clone() for y in ys]
        znew, res = consensus.aggregate_round(xs, z, yk, rho=RHO, mode=mode)
        runs.append((znew, yk, res))
    znew, yk, res = runs[0]
    assert znew.data_ptr() != z.data_ptr()
    assert torch.equal(znew, zt)
    assert torch.allclose(znew.double(), zd, rtol=1e-6, atol=1e-6)
    for k in range(len(ys)):
        assert torch.equal(yk[k], yt[k]), k
        assert torch.allclose(yk[k].double(), yd[k], rtol=1e-6, atol=1e-6)
    assert res.dtype == torch.float32 and res.shape == rd.shape
    err = (res.double() - rd).abs()
    print(mode, K, n, "res rel err", (err / rd.clamp_min(1e-300)).max().item())
    assert bool((err <= 1e-5 * rd).all()), (res.tolist(), rd.tolist())
    assert torch.equal(z, z0)
    assert all(torch.equal(a, b) for a, b in zip(xs, xs0))
    assert torch.equal(runs[1][0], znew) and torch.equal(runs[1][2], res)
    assert all(torch.equal(a, b) for a, b in zip(runs[1][1], yk))


@gpu
@pytest.mark.parametrize("n", [3, 65, 524295])
@pytest.mark.parametrize("K", [1, 3, K_REG_MAX, K_REG_MAX + 1, 32])
@pytest.mark.parametrize("mode", MODES)
def test_aggregate_round_matches_torch_sequence(mode, K, n):
    _check_round(mode, K, n)


@gpu
@pytest.mark.parametrize("mode", MODES)
def test_aggregate_round_unaligned_operands(mode):
    _check_round(mode, 3, 65, offset=1)


def _two_rounds(cls, fused, dev, N=1029, K=3):
    strat = cls()
    strat.fused_aggregate = fused
    comm = LocalComm(K, device=torch.device(dev))
    state = strat.init_block(comm, N, torch.device(dev))
    state["z"] = _vecs(1, N, dev, 10)[0]
    if "y" in state:
        state["y"] = dict(enumerate(_vecs(K, N, dev, 11)))
    infos = []
    for r in range(2):
        x = dict(enumerate(_vecs(K, N, dev, 20 + r)))
        infos.append(strat.aggregate(comm, state, x, r))
    return state, infos


@gpu
@pytest.mark.parametrize("cls", [FedAvg, FedProx, ConsensusADMM])
def test_strategies_fused_equals_torch_sequence(cls):
    (sa, ia), (sb, ib) = (_two_rounds(cls, f, "cuda") for f in (True, False))
    assert torch.equal(sa["z"], sb["z"])
    for k in sa.get("y", {}):
        assert torch.equal(sa["y"][k], sb["y"][k]), k
    for a, b in zip(ia, ib):
        assert a.keys() == b.keys()
        for key in a:
            assert float(a[key]) == pytest.approx(float(b[key]), rel=1e-5)


@gpu
@pytest.mark.parametrize("case", ["short_x", "strided_y", "fp64_z", "K33",
                                  "rho0"])
def test_aggregate_round_rejects_before_launch(case):
    K, n, rho = (33 if case == "K33" else 3), 65, RHO
    xs, ys = _vecs(K, n, "cuda", 1), _vecs(K, n, "cuda", 2)
    z = _vecs(1, n, "cuda", 3)[0]
    if case == "short_x":
        xs[2] = xs[2][:-1]
    elif case == "strided_y":
        ys[2] = _vecs(1, 2 * n, "cuda", 4)[0][::2]
    elif case == "fp64_z":
        z = z.double()
    elif case == "rho0":
        rho = 0.0
    before = [y.clone() for y in ys]
    with pytest.raises(RuntimeError):
        consensus.aggregate_round(xs, z, ys, rho=rho, mode="admm")
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(ys, before))


@pytest.mark.parametrize("cls,mode", [(FedAvg, "fedavg"), (FedProx, "fedprox"),
                                      (ConsensusADMM, "admm")])
def test_cpu_fallback_reproduces_strategies(cls, mode):
    N, K = 1029, 3
    strat = cls()
    comm = LocalComm(K, device=torch.device("cpu"))
    state = strat.init_block(comm, N, torch.device("cpu"))
    state["z"] = _vecs(1, N, "cpu", 10)[0]
    if mode == "admm":
        state["y"] = dict(enumerate(_vecs(K, N, "cpu", 11)))
    x = dict(enumerate(_vecs(K, N, "cpu", 20)))
    ys = [y.clone() for y in state.get("y", {}).values()]
    rho = state.get("rho")
    znew, res = consensus.aggregate_round(list(x.values()), state["z"], ys,
                                          rho=rho, mode=mode)
    info = strat.aggregate(comm, state, x, 0)
    assert torch.equal(znew, state["z"])
    for k, y in enumerate(ys):
        assert torch.equal(y, state["y"][k])
    assert float(res[0].sqrt()) / N == pytest.approx(float(info["dual"]),
                                                     rel=1e-6)
    if mode != "fedavg":
        assert float(res[1:].sqrt().sum()) / N == pytest.approx(
            info["primal"], rel=1e-6)


def test_fused_aggregate_flag_reaches_the_strategy():
    from fedkit.parallel.runtime import FedConfig
    from fedkit.utils.cli import config_from_cli
    assert FedConfig(strategy="admm").make_strategy().fused_aggregate is True
    cfg = config_from_cli(FedConfig(strategy="fedprox"),
                          ["--fused_aggregate", "0"])
    assert cfg.make_strategy().fused_aggregate is False
