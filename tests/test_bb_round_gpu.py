"""Adaptive-rho (BB) round in two passes (csrc/consensus.hip): bb_stats_round
against bb_stats and float64, the BB carry of aggregate_round against the
torch sequence of ConsensusADMM._bb_update.  Shapes as in
test_aggregate_gpu.py; offset 1 = operands 4 bytes past 16-byte alignment;
K = 4 | 5 straddles a statistics bucket.
"""

import pytest
import torch

from fedkit.algos.strategies import BBConfig, ConsensusADMM
from fedkit.ops import consensus
from fedkit.parallel.comm import LocalComm

RHO = 0.1
RHO_USED = [RHO * (1 + k / 64) for k in range(32)]    # distinct per client


def _vecs(count, n, dev, seed, offset=0):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(n + offset, generator=g) * 0.05).to(dev)[offset:]
            for _ in range(count)]


def _operands(K, n, dev, offset=0):
    ys, yh, xs, x0 = (_vecs(K, n, dev, s, offset) for s in (2, 4, 1, 5))
    return ys, yh, xs, _vecs(1, n, dev, 3, offset)[0], x0


@pytest.mark.gpu
@pytest.mark.parametrize("K,n,offset", [(K, n, 0) for K in (1, 4, 5, 32)
                                        for n in (3, 65)]
                         + [(5, 524295, 0), (3, 65, 1)])
def test_bb_stats_round_matches_bb_stats(K, n, offset):
    ys, yh, xs, z, x0 = _operands(K, n, "cuda", offset)
    out = consensus.bb_stats_round(ys, yh, xs, z, x0)
    assert out.shape == (K, 6) and out.dtype == torch.float32 and out.is_cuda
    for k in range(K):
        assert torch.equal(
            out[k], consensus.bb_stats(ys[k], yh[k], xs[k], z, x0[k])), k
        a, b, dx = ((ys[k] - yh[k]).double(), (xs[k] - z).double(),
                    (xs[k] - x0[k]).double())
        pairs = [(a, a), (a, b), (b, b), (a, dx), (b, dx), (dx, dx)]
        ref = torch.stack([u.dot(v) for u, v in pairs])
        mag = torch.stack([(u * v).abs().sum() for u, v in pairs])
        err = (out[k].double() - ref).abs()
        assert bool((err <= 1e-5 * mag).all()), (k, out[k].tolist())
    assert torch.equal(consensus.bb_stats_round(ys, yh, xs, z, x0), out)


def _torch_round(xs, z, ys, rho, rho_used):
    """The strategy's carry + admm round: yhat0s, x0s, znew, ys, residuals"""
    yhat0 = [y + r * (x - z) for x, y, r in zip(xs, ys, rho_used)]
    znew = torch.zeros_like(xs[0])
    for c in [y + rho * x for x, y in zip(xs, ys)]:
        znew += c
    znew /= (len(xs) * rho)
    ydelta = [rho * (x - znew) for x in xs]
    res = [(z - znew).square().sum()] + [d.square().sum() for d in ydelta]
    return (yhat0, [x.clone() for x in xs], znew,
            [y + d for y, d in zip(ys, ydelta)], torch.stack(res))


@pytest.mark.gpu
@pytest.mark.parametrize("n,offset", [(3, 0), (65, 0), (524295, 0), (65, 1)])
@pytest.mark.parametrize("K", [1, 3, 16, 17, 32])
@pytest.mark.parametrize("carry", ["x0", "full"])
def test_carry_round_matches_torch_sequence(carry, K, n, offset):
    ys, _, xs, z, _ = _operands(K, n, "cuda", offset)
    xs0, z0, rho_used = [x.clone() for x in xs], z.clone(), RHO_USED[:K]
    yh_t, x0_t, z_t, y_t, _ = _torch_round(xs, z, ys, RHO, rho_used)
    if carry == "x0":
        yh_t = [torch.full_like(x, 7.0) for x in xs]   # yhat0s are left alone
    res_d = _torch_round([x.double() for x in xs], z.double(),
                         [y.double() for y in ys], RHO, rho_used)[4]
    y_plain = [y.clone() for y in ys]
    z_plain, res_plain = consensus.aggregate_round(xs, z, y_plain, rho=RHO,
                                                   mode="admm")
    runs = []
    for _ in range(2):
        yk = [y.clone() for y in ys]
        x0 = [torch.full_like(x, 7.0) for x in xs]
        yh = [torch.full_like(x, 7.0) for x in xs]
        kw = {"x0s": x0}
        if carry == "full":
            kw.update(yhat0s=yh, rho_used=rho_used)
        znew, res = consensus.aggregate_round(xs, z, yk, rho=RHO, mode="admm",
                                              **kw)
        runs.append([znew, res] + yk + x0 + yh)
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    assert torch.equal(znew, z_t) and torch.equal(znew, z_plain)
    assert torch.equal(res, res_plain)
    err = (res.double() - res_d).abs()
    print(carry, K, n, "res rel err", (err / res_d).max().item())
    assert bool((err <= 1e-5 * res_d).all()), (res.tolist(), res_d.tolist())
    for k in range(K):
        assert torch.equal(yk[k], y_t[k]) and torch.equal(yk[k], y_plain[k]), k
        assert torch.equal(x0[k], x0_t[k]) and torch.equal(yh[k], yh_t[k]), k
    assert all(torch.equal(a, b) for a, b in zip(xs + [z], xs0 + [z0]))


def _bb_rounds(fused, dev, T, rounds=4, N=1029, K=3):
    strat = ConsensusADMM(rho0=RHO, bb=BBConfig(
        True, period_T=T, alphacorrmin=0.0, epsilon=1e-9, rhomax=0.5))
    strat.fused_aggregate = fused
    comm = LocalComm(K, device=torch.device(dev))
    state = strat.init_block(comm, N, torch.device(dev),
                             x0=dict(enumerate(_vecs(K, N, dev, 5))))
    infos, rhos = [], []
    for r in range(rounds):
        x = dict(enumerate(_vecs(K, N, dev, 20 + r)))
        infos.append(strat.aggregate(comm, state, x, r))
        rhos.append(state["rho"])
    return state, infos, rhos, strat, comm


@pytest.mark.gpu
@pytest.mark.parametrize("T", [1, 2])
def test_bb_strategy_fused_equals_unfused(T):
    (sa, ia, ra, *_), (sb, ib, rb, *_) = (_bb_rounds(f, "cuda", T)
                                          for f in (True, False))
    assert ra == rb
    assert any(r != RHO for r in ra), "rho never moved: the chain is untested"
    for key in ("y", "yhat0", "x0"):
        assert all(torch.equal(sa[key][k], sb[key][k]) for k in sa[key]), key
    assert torch.equal(sa["z"], sb["z"])
    for a, b in zip(ia, ib):
        assert a.keys() == b.keys()
        assert all(float(a[k]) == pytest.approx(float(b[k]), rel=1e-5)
                   for k in a), (a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["yhat0_is_y", "short_x0", "short_rho_used",
                                  "fedprox", "strided_stats_yhat0"])
def test_rejects_before_launch(case):
    K, n = 3, 65
    ys, yh, xs, z, x0 = _operands(K, n, "cuda")
    kw = dict(rho=RHO, mode="admm", x0s=x0, yhat0s=yh, rho_used=RHO_USED[:K])
    swap = {"yhat0_is_y": (yh, 1, ys[1]), "short_x0": (x0, 2, x0[2][:-1]),
            "strided_stats_yhat0": (yh, 2, _vecs(1, 2 * n, "cuda", 6)[0][::2])}
    if case in swap:
        vs, k, bad = swap[case]
        vs[k] = bad
    elif case == "short_rho_used":
        kw["rho_used"] = RHO_USED[:K - 1]
    else:
        kw["mode"] = "fedprox"
    before = [v.clone() for v in ys + yh + x0]
    with pytest.raises((RuntimeError, ValueError)):
        if case == "strided_stats_yhat0":
            consensus.bb_stats_round(ys, yh, xs, z, x0)
        else:
            consensus.aggregate_round(
                xs, z, ys if kw["mode"] == "admm" else None, **kw)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(ys + yh + x0, before))


@pytest.mark.parametrize("T", [1, 2])
def test_cpu_fallback_reproduces_unfused_strategy(T):
    """Round 2, a BB round at both T, from the strategy's state before it."""
    N, K, last = 1029, 3, 2
    state, _, _, strat, comm = _bb_rounds(False, "cpu", T, rounds=last)
    full, _, rhos, *_ = _bb_rounds(False, "cpu", T, rounds=last + 1)
    x, z = _vecs(K, N, "cpu", 20 + last), state["z"]
    ys, yh, x0 = (list(state[key].values()) for key in ("y", "yhat0", "x0"))
    stats = consensus.bb_stats_round(ys, yh, x, z, x0)
    assert torch.equal(stats, torch.stack(
        [consensus.bb_stats(*v, z, p) for *v, p in zip(ys, yh, x, x0)]))
    rho_used = strat._bb_rho_chain(
        comm, state, comm.gather_scalar_rows(dict(enumerate(stats.tolist()))),
        last)
    assert state["rho"] == rhos[last] != rhos[last - 1]
    znew, _ = consensus.aggregate_round(
        x, z, ys, rho=state["rho"], mode="admm", x0s=x0, yhat0s=yh,
        rho_used=rho_used)
    assert torch.equal(znew, full["z"])
    for key, vs in zip(("y", "yhat0", "x0"), (ys, yh, x0)):
        assert all(torch.equal(vs[k], full[key][k]) for k in range(K)), key
