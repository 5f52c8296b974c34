"""GPU tests of the fused consensus penalty / ADMM update kernels
(csrc/consensus.hip) against the same formulas in float64 torch, of the
engine's fused closure path against its torch path, and the first FedProx /
ADMM jobs on the GPU.

Value bound: |got - ref| <= 1e-5 * sum|term_i| (sum in float64).  fp32 eps
6e-8 times an accumulation depth of ~20 (per-thread chain, wave tree,
workgroup, finalize) is ~1e-6 of the summed magnitudes; the bound leaves
10x.  For the penalty the terms are its four aggregate terms (never larger
than the elementwise sum), for the dot-product statistics the elementwise
products.  Gradients are elementwise: allclose(rtol=1e-5, atol=1e-6) for
inputs of order 1.
"""

import functools
import json
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

RHO, L1, L2 = 0.1, 1e-2, 1e-3
MODES = ["admm", "fedprox", "reg"]
DEV = "cuda"


def _physical(t):
    """Flat tensor in storage order (channels_last 4-D -> NHWC)."""
    if t.dim() == 4 and t.is_contiguous(memory_format=torch.channels_last):
        return t.permute(0, 2, 3, 1).reshape(-1)
    return t.reshape(-1)


def _randn(g, *shape):
    return torch.randn(*shape, generator=g).to(DEV)


def _make_set(name):
    g = torch.Generator().manual_seed(
        {"A": 1, "B": 2, "C": 3, "D": 4, "E": 5}[name])
    if name == "A":
        ps = [_randn(g, n) for n in (1, 63, 64, 65, 255, 257, 1000)]
        ps.append(_randn(g, 5, 7))
        ps.append(_randn(g, 8, 3, 3, 3).contiguous(
            memory_format=torch.channels_last))
    elif name == "B":
        ps = [_randn(g, 3) for _ in range(50)] + [_randn(g, 70001)]
    elif name == "C":
        ps = [_randn(g, 1000003)]
    elif name == "D":
        # more than 2048 x 256 threads x 4 elements: the gradient kernel's
        # grid-stride loop takes a second trip and ends in an odd tail
        ps = [_randn(g, 2100003)]
    else:
        # the first 48 tensors hold 143 elements, so the second launch's
        # slices of z, y and the flat gradient start 12 bytes past a 16-byte
        # boundary: dword loads and stores on the flat side
        ps = [_randn(g, 2)] + [_randn(g, 3) for _ in range(47)] \
            + [_randn(g, 70001), _randn(g, 6)]
    # some exact zeros: sign(0) must be 0
    for p in ps:
        flat = _physical(p)
        flat[::7] = 0.0
    n = sum(p.numel() for p in ps)
    z = _randn(g, n)
    y = _randn(g, n)
    return ps, z, y


@functools.lru_cache(maxsize=None)
def _set(name):
    """(params, z, y, x64, z64, y64) built once per set and never modified."""
    ps, z, y = _make_set(name)
    x64 = torch.cat([_physical(p) for p in ps]).double()
    return ps, z, y, x64, z.double(), y.double()


def _kw(mode, z, y, l1, l2=L2):
    kw = {"lambda1": l1, "lambda2": l2}
    if mode in ("admm", "fedprox"):
        kw.update(z=z, rho=RHO)
    if mode == "admm":
        kw.update(y=y)
    return kw


def _ref(x, z, y, mode, l1, l2=L2, rho=RHO):
    """float64 value, sum of |terms| and gradient of the penalty."""
    terms = [l1 * x.abs().sum(), l2 * (x * x).sum()]
    grad = l1 * torch.sign(x) + 2.0 * l2 * x
    if mode in ("admm", "fedprox"):
        d = x - z
        terms.append(0.5 * rho * (d * d).sum())
        grad = grad + rho * d
        if mode == "admm":
            terms.append((y * d).sum())
            grad = grad + y
    val = sum(terms)
    mag = sum(t.abs() for t in terms)
    return float(val), float(mag), grad


def _leaves(ps):
    out = []
    for p in ps:
        q = p.detach().clone(memory_format=torch.preserve_format)
        out.append(q.requires_grad_())
    return out


def _flat_grads(ps):
    return torch.cat([_physical(p.grad) for p in ps])


def _penalty(*a, **kw):
    from fedkit.ops import consensus
    return consensus.penalty(*a, **kw)


def _check_value_and_grad(name, mode, l1):
    ps, z, y, x64, z64, y64 = _set(name)
    val, mag, g64 = _ref(x64, z64, y64, mode, l1)
    leaves = _leaves(ps)
    pen = _penalty(leaves, **_kw(mode, z, y, l1))
    assert pen.shape == () and pen.dtype == torch.float32
    err = abs(pen.item() - val)
    print(f"set {name} {mode} l1={l1}: value {pen.item():.9g} ref {val:.9g} "
          f"err {err:.3g} bound {1e-5 * mag:.3g}")
    assert err <= 1e-5 * mag
    pen.backward()
    for p, q in zip(ps, leaves):
        assert q.grad.shape == p.shape and q.grad.stride() == p.stride()
    got = _flat_grads(leaves).double()
    print(f"  max grad err {float((got - g64).abs().max()):.3g}")
    assert torch.allclose(got, g64, rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("l1", [0.0, L1])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_penalty_value_and_grad(name, mode, l1):
    _check_value_and_grad(name, mode, l1)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["D", "E"])
def test_penalty_grad_second_trip_and_unaligned_chunk(name, mode):
    """Set D: N > 2048*256*4, so the gradient kernel (grid cap 2048, four
    elements per thread) strides; set E: an odd chunk base, so the flat side
    of the second launch is not 16-byte aligned."""
    ps = _set(name)[0]
    n = sum(p.numel() for p in ps)
    if name == "D":
        assert n > 2048 * 256 * 4 and n % 4
    else:
        assert len(ps) > 48 and sum(p.numel() for p in ps[:48]) % 4
    _check_value_and_grad(name, mode, L1)


def test_sign_of_zero_is_zero():
    """regulariser-only, lambda2 = 0: the gradient IS lambda1 * sign(x)."""
    ps, _, _, x64, _, _ = _set("A")
    leaves = _leaves(ps)
    _penalty(leaves, lambda1=L1).backward()
    got = _flat_grads(leaves)
    assert bool((x64 == 0).any())
    assert torch.equal(got, (L1 * torch.sign(x64)).float())


def test_grad_out_scales():
    ps, z, y, x64, z64, y64 = _set("A")
    _, _, g64 = _ref(x64, z64, y64, "admm", L1)
    leaves = _leaves(ps)
    (3 * _penalty(leaves, **_kw("admm", z, y, L1))).backward()
    assert torch.allclose(_flat_grads(leaves).double(), 3.0 * g64,
                          rtol=1e-5, atol=1e-6)


def test_grad_accumulates_with_data_loss():
    ps, z, y, _, _, _ = _set("A")

    def data_loss(leaves):
        return sum((q * q * q).sum() for q in leaves)

    a = _leaves(ps)
    data_loss(a).backward()
    b = _leaves(ps)
    _penalty(b, **_kw("admm", z, y, L1)).backward()
    c = _leaves(ps)
    (data_loss(c) + _penalty(c, **_kw("admm", z, y, L1))).backward()
    assert torch.allclose(_flat_grads(c), _flat_grads(a) + _flat_grads(b),
                          rtol=1e-6, atol=1e-6)


def test_x_equals_z_has_zero_proximal_gradient():
    ps, _, _, x64, _, _ = _set("A")
    z = x64.float()
    leaves = _leaves(ps)
    pen = _penalty(leaves, z=z, rho=RHO)
    pen.backward()
    g = _flat_grads(leaves)
    assert pen.item() == 0.0
    assert bool(torch.isfinite(g).all()) and bool((g == 0).all())


def test_no_grad_returns_value_only():
    ps, z, y, x64, z64, y64 = _set("A")
    val, mag, _ = _ref(x64, z64, y64, "admm", L1)
    leaves = _leaves(ps)
    with torch.no_grad():
        pen = _penalty(leaves, **_kw("admm", z, y, L1))
    assert pen.grad_fn is None and not pen.requires_grad
    assert abs(float(pen) - val) <= 1e-5 * mag


@pytest.mark.parametrize("name", ["B", "C"])
def test_penalty_is_deterministic(name):
    ps, z, y, _, _, _ = _set(name)
    res = []
    for _ in range(2):
        leaves = _leaves(ps)
        pen = _penalty(leaves, **_kw("admm", z, y, L1))
        pen.backward()
        res.append((pen.detach().clone(), _flat_grads(leaves)))
    assert torch.equal(res[0][0], res[1][0])
    assert torch.equal(res[0][1], res[1][1])


@pytest.mark.parametrize("mode", MODES)
def test_params_in_place_equal_packed_vector(mode):
    """Reading set A's tensors in place == packing them first and passing
    the one flat tensor: the physical-order pairing with z, channels_last
    included."""
    from fedkit.ops import flat
    ps, z, y, x64, z64, y64 = _set("A")
    _, mag, _ = _ref(x64, z64, y64, mode, L1)
    leaves = _leaves(ps)
    pen = _penalty(leaves, **_kw(mode, z, y, L1))
    pen.backward()
    packed = flat.pack(ps).requires_grad_()
    assert torch.equal(packed.detach().double(), x64)
    pen_p = _penalty([packed], **_kw(mode, z, y, L1))
    pen_p.backward()
    # same elements, another summation order / another FMA contraction
    assert abs(pen.item() - pen_p.item()) <= 1e-5 * mag
    assert torch.allclose(_flat_grads(leaves), packed.grad,
                          rtol=1e-6, atol=1e-6)


def test_unaligned_parameter_storage():
    """Parameters that start 4, 8 and 12 bytes past a 16-byte boundary."""
    g = torch.Generator().manual_seed(5)
    ps = []
    for off, n in ((1, 301), (2, 1026), (3, 64)):
        buf = _randn(g, off + n)
        ps.append(buf[off:])
    n = sum(p.numel() for p in ps)
    z, y = _randn(g, n + 1)[1:], _randn(g, n + 3)[3:]
    x64 = torch.cat(ps).double()
    val, mag, g64 = _ref(x64, z.double(), y.double(), "admm", L1)
    leaves = [p.requires_grad_() for p in ps]
    pen = _penalty(leaves, **_kw("admm", z, y, L1))
    pen.backward()
    assert abs(pen.item() - val) <= 1e-5 * mag
    assert torch.allclose(_flat_grads(leaves).double(), g64,
                          rtol=1e-5, atol=1e-6)


@functools.lru_cache(maxsize=None)
def _vectors(n):
    g = torch.Generator().manual_seed(n)
    return tuple(_randn(g, n) for _ in range(5))


@pytest.mark.parametrize("n", [1000003, 65])
def test_bb_stats(n):
    from fedkit.ops import consensus
    y, yh, x, z, x0 = _vectors(n)
    got = consensus.bb_stats(y, yh, x, z, x0)
    assert got.shape == (6,) and got.dtype == torch.float32
    a, b, dx = (y.double() - yh.double(), x.double() - z.double(),
                x.double() - x0.double())
    pairs = [(a, a), (a, b), (b, b), (a, dx), (b, dx), (dx, dx)]
    got = got.tolist()
    for i, (u, v) in enumerate(pairs):
        ref, mag = float((u * v).sum()), float((u * v).abs().sum())
        print(f"bb_stats n={n} [{i}]: {got[i]:.9g} ref {ref:.9g} "
              f"bound {1e-5 * mag:.3g}")
        assert abs(got[i] - ref) <= 1e-5 * mag
    assert consensus.bb_stats(y, yh, x, z, x0).tolist() == got


@pytest.mark.parametrize("n", [1000003, 65])
def test_admm_dual_update(n):
    from fedkit.ops import consensus
    y0, _, x, z, _ = _vectors(n)
    yd = RHO * (x.double() - z.double())
    res = []
    for _ in range(2):
        y = y0.clone()
        sq = consensus.admm_dual_update(y, x, z, RHO)
        res.append((y, sq))
    y, sq = res[0]
    assert sq.shape == () and sq.dtype == torch.float32
    assert torch.allclose(y.double(), y0.double() + yd, rtol=1e-6, atol=1e-6)
    ref = float((yd * yd).sum())
    assert abs(float(sq) - ref) <= 1e-5 * ref
    assert torch.equal(res[1][0], y) and torch.equal(res[1][1], sq)


# ------------------------------------------------------ engine: one closure

def _smoke_cfg(**kw):
    from fedkit.parallel import FedConfig
    return FedConfig(K=2, default_batch=32, Nloop=1, Nepoch=1, Nadmm=1,
                     check_results=False, save_model=False, use_cuda=True,
                     max_steps_per_epoch=2, be_verbose=False, **kw)


class _ProbeOptimizer:
    """Evaluates the closure once and takes no step."""

    def __init__(self, net):
        self.net = net
        self.loss = None

    def zero_grad(self):
        for p in self.net.parameters():
            p.grad = None

    def step(self, closure):
        self.loss = closure().detach().clone()


@pytest.mark.parametrize("strategy", ["admm", "fedprox"])
def test_closure_fused_equals_torch_path(strategy):
    from fedkit.parallel import FederatedJob
    from fedkit.utils import trainable_params, unfreeze_one_block
    cfg = _smoke_cfg(model="Net", strategy=strategy, admm_rho0=0.1)
    cfg.max_steps_per_epoch = 1
    cfg.diagnostic_forward = False
    job = FederatedJob(cfg)
    ci, ck = 4, 0                       # Net's regularised block
    for k in job.comm.my_clients:
        unfreeze_one_block(job.nets[k], ci)
    net = job.nets[ck]
    tps = trainable_params(net)
    N = sum(p.numel() for p in tps)
    st = job.strategy.init_block(job.comm, N, job.device, None, block_idx=ci)
    g = torch.Generator().manual_seed(9)
    st["z"] = _randn(g, N)
    if strategy == "admm":
        for k in st["y"]:
            st["y"][k] = _randn(g, N)
    job._state = st
    gen_state = job.train_loaders[ck].generator.get_state()
    out = {}
    for fused in (True, False):
        job.train_loaders[ck].generator.set_state(gen_state)
        job.cfg.fused_penalty = fused
        probe = _ProbeOptimizer(net)
        job._local_epoch(ck, probe, st, ci, 0, 0)
        out[fused] = (float(probe.loss),
                      torch.cat([_physical(p.grad) for p in tps]).clone())
    x64 = torch.cat([_physical(p.detach()) for p in tps]).double()
    y64 = st["y"][ck].double() if strategy == "admm" else None
    val, mag, _ = _ref(x64, st["z"].double(), y64, strategy, cfg.lambda1,
                       cfg.lambda2, rho=0.1)
    mag += abs(out[False][0] - val)      # the data-loss term
    print(f"{strategy}: fused {out[True][0]:.9g} torch {out[False][0]:.9g} "
          f"bound {1e-5 * mag:.3g}")
    assert abs(out[True][0] - out[False][0]) <= 1e-5 * mag
    assert torch.allclose(out[True][1], out[False][1], rtol=1e-5, atol=1e-6)


# --------------------------------------------------------------------- jobs

def _run_job(tmp_path, tag, nadmm, kw):
    from fedkit.parallel import FederatedJob
    path = tmp_path / f"{tag}.jsonl"
    cfg = _smoke_cfg(model="Net", jsonl_path=str(path), **kw)
    cfg.Nadmm = nadmm
    job = FederatedJob(cfg)
    job.run()
    for ck in job.comm.my_clients:
        for p in job.nets[ck].parameters():
            assert torch.isfinite(p).all()
    recs = [json.loads(line) for line in path.read_text().splitlines()]
    return job._state["z"].clone(), recs


@pytest.fixture
def deterministic_convs():
    """Net's fp32 convolutions run in the vendor library (only the bf16
    path has hand-written conv kernels), whose default backward-weight
    algorithm is not run-to-run reproducible: two identical fp32 FedAvg
    jobs already differ in the last bits of every conv block's z.  The
    determinism asserted below is that of the engine and of the penalty /
    ADMM kernels, so the library is asked for its reproducible algorithms
    while the jobs run."""
    old = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    yield
    torch.backends.cudnn.deterministic = old


@pytest.mark.parametrize("nadmm,kw", [
    (2, dict(strategy="fedprox")),
    (3, dict(strategy="admm", bb_update=True)),
], ids=["fedprox", "admm_bb"])
def test_penalty_job_gpu(tmp_path, deterministic_convs, nadmm, kw):
    """FedProx and BB-ADMM jobs on the GPU: finite, and deterministic."""
    zs = []
    for tag in ("a", "b"):
        z, recs = _run_job(tmp_path, tag, nadmm, kw)
        assert len(recs) == 5 * nadmm     # Net: 5 blocks x Nadmm rounds
        for r in recs:
            assert math.isfinite(r["primal"]) and r["primal"] > 0
            assert math.isfinite(r["dual"]) and r["dual"] > 0
        zs.append(z)
    assert torch.equal(zs[0], zs[1])
