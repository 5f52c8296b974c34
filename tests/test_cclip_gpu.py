"""consensus.cclip_round (csrc/cclip.hip) against the float64 rule on the
vectors and the torch sequence that defines znew; inputs and grid (that of
test_geomed_gpu.py, times three bucket / radius settings): test_cclip.py.

Weight bound |w - w64| <= T max(w64): T is 4 x the largest such error of a
float64 Gram-space solver fed torch's own fp32 A @ A.T of the centred stack,
over the grid of the main test on the MI355X (the two accumulation orders
differ).  Measured: torch 1.820e-6 (K = 17, s = 3, n = 524295; at most
1.23e-7 at the smaller n), the kernel 1.83e-7 (K = 17, s = 3, n = 65; at most
7.4e-8 at the other n).
"""

import pytest
import torch

from fedkit import ops
from fedkit.algos.strategies import FedAvg, FedProx
from fedkit.ops import consensus
from fedkit.parallel.comm import LocalComm
from test_cclip import CASES, SIZES, clients, solve64, solve_args

gpu = pytest.mark.gpu
RHO = 0.1
MODES = ["fedavg", "fedprox"]
T_WEIGHTS = 4 * 1.820e-6      # see the docstring


def _cuda(K, f, n, offset=0, seed=0):
    xs, z, bad = clients(K, f, n, offset, seed)
    return [x.cuda() for x in xs], z.cuda(), bad


def _native(xs, z, mode, iters=3, tau=0.0, bucket=1, perm=None, rho=RHO):
    """(znew, res, w, keep, d, tau_used) of the extension"""
    perm = list(range(len(xs))) if perm is None else perm
    return ops.require_ext().cclip_round(
        xs, z, rho, consensus.AGGREGATE_MODES.index(mode), iters, tau, bucket,
        torch.tensor(perm, dtype=torch.int32).cuda())


def _is_sequence(znew, xs, z, w, keep):
    zt = z.clone()
    for k in keep.nonzero().flatten().tolist():
        zt += w[k] * (xs[k] - z)
    return torch.equal(znew.view(torch.int32), zt.view(torch.int32))


def _check_round(K, f, s, kind, mode, n, offset=0):
    xs, z, bad = _cuda(K, f, n, offset)
    args = solve_args(xs, z, bad, s, kind)
    xs0, z0 = [x.clone() for x in xs], z.clone()
    znew, res, w = consensus.cclip_round(xs, z, RHO, mode, *args)
    again = _native(xs, z, mode, *args)
    keep = again[3]
    assert all(torch.equal(a, b) for a, b in zip((znew, res, w), again))
    assert all(torch.equal(a, b) for a, b in zip(xs + [z], xs0 + [z0]))
    assert keep.dtype == torch.int32 and keep.shape == (K,) and bool(keep.all())
    assert (w.dtype, w.shape, znew.dtype, znew.shape) == (
        torch.float32, (K,), torch.float32, z.shape)
    assert _is_sequence(znew, xs, z, w, keep)
    w64, clips_and_passes = solve64(xs, z, args)
    assert clips_and_passes
    err = ((w.double() - w64).abs().max() / w64.max()).item()
    print("cclip", K, f, s, kind, mode, n, "weight err", err)
    assert err <= T_WEIGHTS
    diffs = [z - znew.double()] + [RHO * (x - znew.double()) for x in xs]
    r64 = torch.stack([(v.double() ** 2).sum() for v in diffs])[:res.numel()]
    assert res.dtype == torch.float32
    assert res.shape == (1 + K * (mode == "fedprox"),)
    assert bool(((res.double() - r64).abs() <= 1e-5 * r64).all()), \
        (res.tolist(), r64.tolist())


@gpu
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("K,f,s,kind", CASES)
def test_cclip_round_matches_reference(K, f, s, kind, mode, n):
    _check_round(K, f, s, kind, mode, n)


@gpu
def test_cclip_round_unaligned_operands():
    _check_round(17, 7, 2, "auto", "fedprox", 1029, offset=1)


@gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("s", [1, 2])
@pytest.mark.parametrize("poison", ["nan", "inf", "1e6"])
@pytest.mark.parametrize("K,f", [(5, 1), (17, 7)])
def test_cclip_round_bad_client(K, f, poison, s, mode):
    n, iters = 65, 3
    xs, z, _ = _cuda(K, 0, n)
    bad = [K - 1 - 2 * j for j in range(f)]
    for k in bad:
        xs[k] = torch.full((n,), float(poison)).cuda()
    znew, res, w, keep, _, tau_used = _native(xs, z, mode, iters, bucket=s)
    live = poison == "1e6"      # kept, with a positive weight
    ok = [live or k not in bad for k in range(K)]
    assert keep.tolist() == [int(v) for v in ok]
    assert (w[bad] > 0).tolist() == [live] * f
    assert bool(znew.isfinite().all()) and _is_sequence(znew, xs, z, w, keep)
    move = (znew.double() - z.double()).norm().item()
    assert 0 < move <= iters * tau_used.item()
    assert res.isfinite().tolist() == [True] + ok * (mode == "fedprox")


@gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", ["at_z", "neg_zero_K1", "neg_zero_K5"])
def test_cclip_round_degenerate(case, mode):
    """neg_zero: a skipped NaN client must not turn z's -0.0 into +0.0"""
    K = 1 if case == "neg_zero_K1" else 5
    xs, z, _ = _cuda(K, 0, 65)
    if case == "at_z":
        xs = [z.clone() for _ in range(K)]
    else:
        z[::2] = -0.0
        xs = [torch.full_like(z, float("nan")) for _ in range(K)]
    znew, _, w, keep, _, tau_used = _native(xs, z, mode)
    assert keep.tolist() == [int(case == "at_z")] * K
    assert torch.equal(znew.view(torch.int32), z.view(torch.int32))
    assert torch.equal(w.cpu(), torch.full((K,), (case == "at_z") / K))


@gpu
@pytest.mark.parametrize("case,kw", [
    ("K33", {}), ("strided_x", {}), ("fp64_z", {}), ("iters0", {"iters": 0}),
    ("tau_neg", {"tau": -1.0}), ("bucket0", {"bucket": 0}),
    ("bucket_K1", {"bucket": 5}), ("short_perm", {"perm": [0, 1, 2]}),
    ("admm", {"mode": "admm"})])
def test_cclip_round_rejects_before_launch(case, kw):
    xs, z, _ = _cuda(33 if case == "K33" else 4, 0, 65)
    if case == "strided_x":
        xs[2] = torch.randn(130).cuda()[::2]
    elif case == "fp64_z":
        z = z.double()
    with pytest.raises(RuntimeError):
        _native(xs, z, **{"mode": "fedprox", **kw})
    torch.cuda.synchronize()


@gpu
@pytest.mark.parametrize("cls", [FedAvg, FedProx])
def test_cclip_strategies_fused_matches_torch_sequence(cls):
    """z and the weights to T of their largest entry"""
    N, K = 1029, 5
    out = []
    for fused in (True, False):
        strat = cls(robust="cclip", agg_bucket=2, agg_seed=69)
        strat.fused_aggregate = fused
        comm = LocalComm(K, device=torch.device("cuda"))
        state = strat.init_block(comm, N, torch.device("cuda"))
        state["z"] = _cuda(K, 1, N)[1]
        infos = [strat.aggregate(
            comm, state, dict(enumerate(_cuda(K, 1, N, seed=r)[0])), r)
            for r in range(2)]
        out.append((state["z"], state["cclip_weights"], infos))
    (za, wa, ia), (zb, wb, ib) = out
    assert float((wa - wb).abs().max()) <= T_WEIGHTS * float(wb.max())
    assert float((za - zb).abs().max()) <= T_WEIGHTS * float(zb.abs().max())
    for a, b in zip(ia, ib):
        assert {k: float(v) for k, v in a.items()} == pytest.approx(
            {k: float(v) for k, v in b.items()}, rel=1e-5)
