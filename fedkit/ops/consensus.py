"""Consensus penalty and ADMM update ops (FedProx / consensus ADMM hot path).

The closure of a FedProx/ADMM client adds, on every call,

    [y.(x-z)] + (rho/2)||x-z||^2 + lambda1 ||x||_1 + lambda2 ||x||^2

over the trainable block x (consensus_multi.py:209-218,
fedprox_multi.py:183-190, federated_multi.py:183-187).  On MI355X
`penalty` evaluates it with ONE streaming reduction that reads the
parameter tensors in place and differentiates it with ONE elementwise
kernel writing the closed-form gradient (csrc/consensus.hip) — no cat of
the block, no autograd tape over a dozen elementwise ops.  The aggregation
side has `admm_dual_update` (y += rho (x-z) fused with the primal-residual
norm) and `bb_stats` (the six Barzilai-Borwein inner products in one pass);
`aggregate_round` runs a whole round of K local clients (z-update, dual
update, residuals) as one pass over the operands.  With adaptive rho,
`bb_stats_round` forms the statistics of all K clients in one pass and
`aggregate_round` writes the BB carry (yhat0, x0) from the operands it holds.
`robust_round` is the Byzantine-robust form of a FedAvg / FedProx round: the
coordinate-wise trimmed mean or median over the K clients in one pass
(csrc/robust.hip).  `krum_round` is the distance-based form (Krum /
Multi-Krum): `pairwise_sqdist` from an MFMA Gram pass over the centred
vectors, the selection on the device, and the mean of the selected clients
(csrc/krum.hip).  `geomed_round` is the geometric median (RFA): smoothed
Weiszfeld re-weighting of the clients, iterated on the same Gram matrix on
the device, and one weighted pass (csrc/geomed.hip).  `cclip_round` is
centred clipping with bucketing: the clients are averaged in random groups,
the group means are clipped towards the old consensus, again iterated on the
Gram matrix on the device, and the same weighted pass (csrc/cclip.hip).
`bulyan_round` composes the two families: iterated Krum on the Gram distances
selects the clients on the device, and a sorting-network pass averages, per
coordinate, the selected values closest to their median (csrc/bulyan.hip).

All vectors are fp32 in PHYSICAL (storage) element order, the order
flat.pack / paramvec.flat_physical use.  Dispatch follows the package rule:
native on a ROCm tensor (raising when the extension is missing), stock
torch on CPU.  The CPU expressions are the ones the engine and the
strategies have always used, in the same order, so CPU runs stay
bit-identical.
"""

import math
from typing import Optional, Sequence

import torch
from torch.autograd.function import once_differentiable

from .flat import _flat_views


def _use_native(t: torch.Tensor) -> bool:
    from . import native_enabled
    return native_enabled(t)


def _flat_physical(p: torch.Tensor) -> torch.Tensor:
    # same as fedkit.utils.paramvec.flat_physical (utils imports ops)
    if p.dim() == 4 and p.is_contiguous(memory_format=torch.channels_last):
        return p.permute(0, 2, 3, 1).reshape(-1)
    return p.reshape(-1)


def _penalty_torch(params, z, y, rho, lambda1, lambda2):
    """The expression sequence of FederatedJob's closure + Strategy.penalty."""
    vec = torch.cat([_flat_physical(p) for p in params])
    out = None
    if z is not None:
        xdelta = vec - z
        out = 0.5 * rho * (torch.norm(xdelta, 2) ** 2)
        if y is not None:
            out = torch.dot(y, xdelta) + out
    if lambda1 or lambda2:
        if lambda1:
            reg1 = lambda1 * torch.norm(vec, 1)
            out = reg1 if out is None else out + reg1
        reg2 = lambda2 * (torch.norm(vec, 2) ** 2)
        out = reg2 if out is None else out + reg2
    if out is None:
        out = vec.sum() * 0.0
    return out


class _PenaltyFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, y, rho, lambda1, lambda2, *params):
        from . import require_ext
        ctx.save_for_backward(*params)
        ctx.consts = (z, y, rho, lambda1, lambda2)
        return require_ext().penalty_fwd([p.detach() for p in params], z, y,
                                         rho, lambda1, lambda2)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        from . import require_ext
        params = ctx.saved_tensors
        z, y, rho, lambda1, lambda2 = ctx.consts
        flat = require_ext().penalty_bwd(
            [p.detach() for p in params], z, y, rho, lambda1, lambda2,
            grad_out.to(torch.float32).contiguous())
        return (None,) * 5 + tuple(_flat_views(flat, params))


def penalty(params: Sequence[torch.Tensor], z: Optional[torch.Tensor] = None,
            y: Optional[torch.Tensor] = None, rho: float = 0.0,
            lambda1: float = 0.0, lambda2: float = 0.0) -> torch.Tensor:
    """[y.(x-z)] + (rho/2)||x-z||^2 + lambda1||x||_1 + lambda2||x||^2 with x
    the physical-order concatenation of `params`; differentiable w.r.t. the
    parameters.  z=None drops both proximal terms (regulariser only), y=None
    only the dual term (FedProx).  Under no_grad only the value is computed.
    """
    params = list(params)
    assert len(params) > 0, "penalty needs at least one parameter tensor"
    assert z is not None or y is None, "a dual vector y needs a target z"
    assert z is None or not z.requires_grad, "z must not require grad"
    assert y is None or not y.requires_grad, "y must not require grad"
    rho, lambda1, lambda2 = float(rho), float(lambda1), float(lambda2)
    if _use_native(params[0]):
        return _PenaltyFn.apply(z, y, rho, lambda1, lambda2, *params)
    return _penalty_torch(params, z, y, rho, lambda1, lambda2)


def admm_dual_update(y: torch.Tensor, x: torch.Tensor, z: torch.Tensor,
                     rho: float) -> torch.Tensor:
    """y += rho (x - z) in place; returns the scalar tensor
    sum((rho (x - z))^2) (the squared primal-residual norm)."""
    if _use_native(y):
        from . import require_ext
        return require_ext().admm_dual_update(y, x.contiguous(),
                                              z.contiguous(), float(rho))
    ydelta = rho * (x - z)
    y.add_(ydelta)
    return torch.norm(ydelta) ** 2


AGGREGATE_MODES = ("fedavg", "fedprox", "admm")
MAX_FUSED_CLIENTS = 32     # kMaxClients of csrc/consensus.hip


def aggregate_round(xs: Sequence[torch.Tensor], z: torch.Tensor,
                    ys: Optional[Sequence[torch.Tensor]] = None,
                    rho: Optional[float] = None, mode: str = "fedavg",
                    x0s: Optional[Sequence[torch.Tensor]] = None,
                    yhat0s: Optional[Sequence[torch.Tensor]] = None,
                    rho_used: Optional[Sequence[float]] = None):
    """One aggregation round over the K client vectors `xs` held in this
    process; returns (znew, res).

      fedavg   znew = (x_0 + ... + x_{K-1}) / K
      fedprox  same znew
      admm     znew = sum_k (y_k + rho x_k) / (K rho), then
               ys[k] += rho (xs[k] - znew) in place

    `res` is fp32 on z's device: res[0] = sum (z - znew)^2 and, except in
    fedavg mode, res[1 + k] = sum (rho (xs[k] - znew))^2.  `z` and `xs` are
    not modified and znew is a new tensor.  On the GPU this is one pass over
    the operands (csrc/consensus.hip, 1 <= K <= 32) whose znew and ys are
    bitwise those of the torch sequence below.

    BB carry (admm only; what adaptive rho keeps from one BB round to the
    next, written in place by the same pass, from `ys` as they came in and
    the old `z`):
      x0s                      x0s[k] = xs[k]   (round 0)
      x0s, yhat0s, rho_used    also yhat0s[k] = ys[k] + rho_used[k] (xs[k] - z)
    `rho_used` is K floats, the rho the BB chain had at client k's turn.  The
    outputs may not overlap an operand or each other.
    """
    assert mode in AGGREGATE_MODES, f"unknown mode {mode!r}"
    xs = list(xs)
    ys = list(ys) if ys is not None else []
    if mode == "admm":
        assert len(ys) == len(xs), "admm needs one dual vector per client"
    if mode != "fedavg":
        assert rho is not None, f"{mode} needs rho"
    carry = [v is not None for v in (x0s, yhat0s, rho_used)]
    if any(carry) and mode != "admm":
        raise ValueError("x0s / yhat0s / rho_used are admm operands")
    if carry not in ([False] * 3, [True, False, False], [True] * 3):
        raise ValueError("the BB carry is x0s alone, or x0s, yhat0s and "
                         "rho_used together")
    x0s = list(x0s) if carry[0] else []
    yhat0s = list(yhat0s) if carry[1] else []
    rho_used = [float(r) for r in rho_used] if carry[2] else []
    if _use_native(z):
        from . import require_ext
        znew, res = require_ext().aggregate_round(
            xs, z, ys if mode == "admm" else [],
            0.0 if rho is None else float(rho), AGGREGATE_MODES.index(mode),
            x0s, yhat0s, rho_used)
        return znew, res
    K = len(xs)
    if any(len(v) != K for v in (x0s, yhat0s, rho_used) if v):
        raise ValueError(f"the BB carry needs one entry per client ({K})")
    # ConsensusADMM._bb_update's carry, before the duals move
    for k in range(len(yhat0s)):
        yhat0s[k].copy_(ys[k] + rho_used[k] * (xs[k] - z))
    for k in range(len(x0s)):
        x0s[k].copy_(xs[k])
    contrib = [y + rho * x for x, y in zip(xs, ys)] if mode == "admm" else xs
    znew = torch.zeros_like(contrib[0])
    for c in contrib:
        znew += c
    znew /= (K * rho) if mode == "admm" else K
    res = [torch.norm(z - znew) ** 2]
    if mode != "fedavg":
        for k, x in enumerate(xs):
            ydelta = rho * (x - znew)
            res.append(torch.norm(ydelta) ** 2)
            if mode == "admm":
                ys[k].add_(ydelta)
    return znew, torch.stack(res)


KRUM_RULES = ("krum", "multi_krum")
ROBUST_RULES = ("trimmed_mean", "median") + KRUM_RULES + ("geomed", "cclip",
                                                          "bulyan")


def robust_trim(rule: str, trim_frac: float, K: int) -> int:
    """Ranks dropped at each end: floor(trim_frac * K) for "trimmed_mean",
    (K - 1) // 2 for "median" (the middle value for odd K, the mean of the
    two middle values for even K)."""
    if rule not in ("trimmed_mean", "median"):
        raise ValueError(f"{rule!r} is not a coordinate-wise robust rule")
    trim = (K - 1) // 2 if rule == "median" else math.floor(trim_frac * K)
    if not 0 <= 2 * trim < K:
        raise ValueError(f"trim_frac {trim_frac} drops {2 * trim} of {K} "
                         "clients; it must leave at least one")
    return trim


def robust_round_torch(xs: Sequence[torch.Tensor], z: torch.Tensor,
                       rho: Optional[float] = None, mode: str = "fedavg",
                       trim: int = 0):
    """The torch sequence that defines `robust_round` bit for bit, on the
    operands' device and in their dtype."""
    K, m = len(xs), len(xs) - 2 * trim
    s = torch.sort(torch.stack(list(xs)), dim=0).values
    znew = torch.zeros_like(z)
    for r in range(trim, K - trim):
        znew += s[r]
    znew /= m
    res = [torch.norm(z - znew) ** 2]
    if mode != "fedavg":
        res += [torch.norm(rho * (x - znew)) ** 2 for x in xs]
    return znew, torch.stack(res)


def robust_round(xs: Sequence[torch.Tensor], z: torch.Tensor,
                 rho: Optional[float] = None, mode: str = "fedavg",
                 trim: int = 0):
    """One Byzantine-robust aggregation round over the K client vectors
    `xs`: the coordinate-wise trimmed mean (Yin et al., 2018).  Per element
    the K values are sorted ascending in torch.sort's order (-inf < finite <
    +inf < NaN), the `trim` smallest and `trim` largest are dropped
    (0 <= 2 * trim < K) and the other m = K - 2 * trim are averaged;
    trim = (K - 1) // 2 is the median.  Up to `trim` clients may hold
    anything, NaN and Inf included, and znew stays within the range of the
    others.

    Returns (znew, res) as `aggregate_round` does: res[0] = sum (z - znew)^2
    and, in fedprox mode, res[1 + k] = sum (rho (xs[k] - znew))^2 (NaN for a
    NaN client: that is the signal).  Modes are fedavg and fedprox; there is
    no robust ADMM round.  On the GPU this is one pass over the operands
    (csrc/robust.hip, 1 <= K <= 32), with znew bitwise that of
    `robust_round_torch`, which is the CPU path.
    """
    if mode == "admm":
        raise ValueError("there is no robust ADMM round; use fedavg or fedprox")
    assert mode in AGGREGATE_MODES, f"unknown mode {mode!r}"
    xs = list(xs)
    if mode != "fedavg":
        assert rho is not None, f"{mode} needs rho"
    if _use_native(z):
        from . import require_ext
        znew, res = require_ext().robust_round(
            xs, z, 0.0 if rho is None else float(rho),
            AGGREGATE_MODES.index(mode), int(trim))
        return znew, res
    if not 1 <= len(xs) or not 0 <= 2 * trim < len(xs):
        raise ValueError(f"robust_round needs 0 <= 2 * trim < K, got trim "
                         f"{trim} for {len(xs)} clients")
    return robust_round_torch(xs, z, rho, mode, trim)


def krum_params(rule: str, trim_frac: float, K: int):
    """(f, m) of a Krum round: f = floor(trim_frac * K) clients may be bad
    (the `trim_frac` knob read as that fraction); "krum" averages m = 1
    client, "multi_krum" m = K - f."""
    if rule not in KRUM_RULES:
        raise ValueError(f"unknown Krum rule {rule!r}; one of {KRUM_RULES}")
    f = math.floor(trim_frac * K)
    if K - f - 2 < 1:
        raise ValueError(f"Krum scores need K - f - 2 >= 1 neighbours; "
                         f"trim_frac {trim_frac} gives f = {f} of K = {K}")
    return f, (1 if rule == "krum" else K - f)


def _check_krum(K: int, f: int, m: int, mode: str):
    if mode == "admm":
        raise ValueError("there is no robust ADMM round; use fedavg or fedprox")
    assert mode in AGGREGATE_MODES, f"unknown mode {mode!r}"
    if f < 0 or K - f - 2 < 1 or not 1 <= m <= K:
        raise ValueError(f"krum_round needs f >= 0, K - f - 2 >= 1 and "
                         f"1 <= m <= K, got K = {K}, f = {f}, m = {m}")


def _pairwise_sqdist_torch(xs):
    K = len(xs)
    d = {(i, j): ((xs[i] - xs[j]) ** 2).sum()
         for i in range(K) for j in range(i + 1, K)}
    d.update({(i, i): xs[0].new_zeros(()) for i in range(K)})
    D = torch.stack([d[min(i, j), max(i, j)]
                     for i in range(K) for j in range(K)]).reshape(K, K)
    return torch.where(D.isfinite(), D, torch.full_like(D, math.inf))


def pairwise_sqdist(xs: Sequence[torch.Tensor],
                    center: torch.Tensor) -> torch.Tensor:
    """[K, K] squared distances D_ij = sum (xs[i] - xs[j])^2, exactly
    symmetric with a zero diagonal; a non-finite entry counts as +inf.  On
    the GPU (fp32, 1 <= K <= 32) D_ij = G_ii + G_jj - 2 G_ij from one MFMA
    Gram pass over xs[k] - center (csrc/krum.hip): the error scales with
    ||xs[i] - center||^2 + ||xs[j] - center||^2, so `center` should be
    close to the clients (the old consensus is).  The CPU forms D from the
    differences, in the operands' dtype, and does not read `center`."""
    xs = list(xs)
    if _use_native(center):
        from . import require_ext
        return require_ext().pairwise_sqdist(xs, center)
    return _pairwise_sqdist_torch(xs)


def krum_round_torch(xs: Sequence[torch.Tensor], z: torch.Tensor,
                     rho: Optional[float] = None, mode: str = "fedavg",
                     f: int = 0, m: Optional[int] = None):
    """The torch sequence that defines `krum_round`, on the operands' device
    and in their dtype; returns (znew, res, sel)."""
    xs = list(xs)
    K = len(xs)
    m = K - f if m is None else m
    _check_krum(K, f, m, mode)
    D = _pairwise_sqdist_torch(xs)
    D.fill_diagonal_(math.inf)          # D_ii is excluded
    near = torch.sort(D, dim=1, stable=True).values
    score = torch.zeros_like(near[:, 0])
    for r in range(K - f - 2):          # ascending order
        score += near[:, r]
    order = torch.argsort(score, stable=True)
    sel = torch.zeros(K, dtype=torch.bool, device=z.device)
    sel[order[:m]] = True
    znew = torch.zeros_like(z)
    for k in order[:m].sort().values.tolist():
        znew += xs[k]
    znew /= m
    res = [torch.norm(z - znew) ** 2]
    if mode != "fedavg":
        res += [torch.norm(rho * (x - znew)) ** 2 for x in xs]
    return znew, torch.stack(res), sel


def krum_round(xs: Sequence[torch.Tensor], z: torch.Tensor,
               rho: Optional[float] = None, mode: str = "fedavg", f: int = 0,
               m: Optional[int] = None, center: Optional[torch.Tensor] = None):
    """One Krum / Multi-Krum aggregation round (Blanchard et al., 2017) over
    the K client vectors `xs`, of which up to `f` may be Byzantine: client i
    is scored by the sum of its K - f - 2 smallest squared distances to the
    other clients, and the `m` clients of lowest score (ties to the lower
    index; m = None means K - f, m = 1 is Krum) are averaged in ascending
    client order.  Unlike the coordinate-wise rules this rejects a client
    whose every coordinate is in range while the vector as a whole is not.

    Returns (znew, res, sel): znew and res as `robust_round` (res[1 + k] for
    all K clients in fedprox mode, NaN for a NaN client), sel a bool [K]
    tensor on z's device, formed without a host sync.  Needs f >= 0,
    K - f - 2 >= 1 and 1 <= m <= K; modes are fedavg and fedprox.  On the
    GPU (csrc/krum.hip, K <= 32) the distances come from `pairwise_sqdist`
    around `center` (None means z) and znew is bitwise that of
    `krum_round_torch`, the CPU path, over the same selection.
    """
    xs = list(xs)
    m = len(xs) - f if m is None else m
    if mode != "fedavg" and mode != "admm":
        assert rho is not None, f"{mode} needs rho"
    if _use_native(z):
        if mode == "admm":
            raise ValueError("there is no robust ADMM round; use fedavg or "
                             "fedprox")
        assert mode in AGGREGATE_MODES, f"unknown mode {mode!r}"
        from . import require_ext
        znew, res, sel, _, _ = require_ext().krum_round(
            xs, z, z if center is None else center,
            0.0 if rho is None else float(rho), AGGREGATE_MODES.index(mode),
            int(f), int(m))
        return znew, res, sel.bool()
    return krum_round_torch(xs, z, rho, mode, f, m)


def geomed_round_torch(xs: Sequence[torch.Tensor], z: torch.Tensor,
                       rho: Optional[float] = None, mode: str = "fedavg",
                       iters: int = 16, nu: float = 1e-3):
    """The torch sequence that defines `geomed_round` (the rule is stated
    there), on the operands' device and in their dtype, directly on the
    vectors; returns (znew, res, c).  It reads the kept set on the host."""
    if mode == "admm":
        raise ValueError("there is no robust ADMM round; use fedavg or fedprox")
    assert mode in AGGREGATE_MODES, f"unknown mode {mode!r}"
    if not 1 <= iters <= 1024 or not (nu > 0 and math.isfinite(nu)):
        raise ValueError(f"geomed_round needs 1 <= iters <= 1024 and a finite "
                         f"nu > 0, got iters = {iters}, nu = {nu}")
    xs = list(xs)
    sq = torch.stack([((x - z) ** 2).sum() for x in xs])
    kept = sq.isfinite().nonzero().flatten().tolist()
    Kp = len(kept)
    mid = (Kp - 1) // 2
    c = torch.zeros_like(sq)
    floor = nu * sq[kept].sort().values[mid].sqrt() if Kp else 0.0
    if Kp == 0:
        pass
    elif float(floor) == 0.0 or Kp <= 2:
        c[kept] = 1.0 / Kp
    else:
        pair = {(i, j): ((xs[i] - xs[j]) ** 2).sum()
                for i in kept for j in kept if i < j}
        r = torch.stack([
            torch.stack([pair[min(i, j), max(i, j)] for j in kept if j != i])
            .sort().values[mid] for i in kept]).sqrt()
        w = 1.0 / torch.maximum(floor, r)
        ck = w / w.sum()
        for _ in range(iters):
            v = z.clone()
            for j, k in enumerate(kept):
                v += ck[j] * (xs[k] - z)
            d = torch.stack([((xs[k] - v) ** 2).sum() for k in kept]).sqrt()
            w = 1.0 / torch.maximum(floor, d)
            ck = w / w.sum()
        c[kept] = ck
    znew = z.clone()
    for k in kept:
        znew += c[k] * (xs[k] - z)
    res = [torch.norm(z - znew) ** 2]
    if mode != "fedavg":
        res += [torch.norm(rho * (x - znew)) ** 2 for x in xs]
    return znew, torch.stack(res), c


def geomed_round(xs: Sequence[torch.Tensor], z: torch.Tensor,
                 rho: Optional[float] = None, mode: str = "fedavg",
                 iters: int = 16, nu: float = 1e-3):
    """One geometric-median aggregation round (RFA: Pillutla, Kakade and
    Harchaoui, 2022) over the K client vectors `xs`: the clients are
    re-weighted by smoothed Weiszfeld steps, none is dropped, and up to half
    of them may hold anything.  The rule:

      1. keep[k] = sum((xs[k] - z)^2) is finite; a client that is not kept
         has weight exactly 0 and is multiplied by nothing.  K' = number
         kept; K' = 0 gives c = 0 and znew = z.
      2. r_k = the median distance from kept client k to the other kept
         clients, s = the median of the kept ||x_k - z||, both medians the
         value at 0-based index (K' - 1) // 2 of the ascending values.
      3. floor = nu * s.  floor == 0 or K' <= 2: c = 1 / K' on the kept
         clients.  Otherwise c_k ~ 1 / max(floor, r_k), normalised to sum 1,
         then exactly `iters` times d_k = max(floor, ||x_k - v||) with
         v = z + sum_j c_j (x_j - z), and c_k ~ 1 / d_k, normalised.
      4. znew = z.clone(); znew += c[k] * (xs[k] - z) for kept k ascending.

    The median-distance start and the median-scaled floor keep a colluding
    far-away minority from capturing the first iterate.

    Returns (znew, res, c): znew and res as `robust_round` (res[1 + k] for
    all K clients in fedprox mode, NaN for a NaN client), c the fp32 [K]
    weights on z's device, formed without a host sync.  Modes are fedavg and
    fedprox; 1 <= iters <= 1024, nu finite and > 0.  On the GPU
    (csrc/geomed.hip, K <= 32) Weiszfeld runs on the MFMA Gram matrix of
    xs[k] - z, two passes over the operands whatever `iters` is, and znew is
    bitwise the sequence of step 4 over the kernel's own c and keep; c
    agrees with `geomed_round_torch`, the CPU path, to the Gram matrix's
    rounding.  That error scales with ||xs[k] - z||^2, so z should be close
    to the clients (the old consensus is); at a block's round 0 the
    consensus is 0 and the conditioning is that of the raw vectors.
    Distances below about 7e-4 of the centred norm are not resolved, which
    is what the default nu covers.
    """
    xs = list(xs)
    if mode != "fedavg" and mode != "admm":
        assert rho is not None, f"{mode} needs rho"
    if _use_native(z):
        assert mode in AGGREGATE_MODES, f"unknown mode {mode!r}"
        from . import require_ext
        znew, res, c, _, _ = require_ext().geomed_round(
            xs, z, 0.0 if rho is None else float(rho),
            AGGREGATE_MODES.index(mode), int(iters), float(nu))
        return znew, res, c
    return geomed_round_torch(xs, z, rho, mode, iters, nu)


def _cclip_perm(perm, K: int):
    """`perm` as a list of K ints, checked on the host: a permutation of
    0..K-1 (None: the identity)."""
    if perm is None:
        return list(range(K))
    if isinstance(perm, torch.Tensor):
        if perm.device.type != "cpu":
            raise ValueError("cclip_round takes perm as a sequence or a CPU "
                             "tensor: its contents are checked on the host")
        perm = perm.tolist()
    perm = [int(p) for p in perm]
    if sorted(perm) != list(range(K)):
        raise ValueError(f"perm must be a permutation of 0..{K - 1}, got "
                         f"{perm}")
    return perm


def _check_cclip(K: int, mode: str, iters: int, tau: float, bucket: int):
    if mode == "admm":
        raise ValueError("there is no robust ADMM round; use fedavg or fedprox")
    assert mode in AGGREGATE_MODES, f"unknown mode {mode!r}"
    if (not 1 <= iters <= 1024 or not (tau >= 0 and math.isfinite(tau))
            or not 1 <= bucket <= K):
        raise ValueError(f"cclip_round needs 1 <= iters <= 1024, a finite "
                         f"tau >= 0 and 1 <= bucket <= K, got iters = {iters}, "
                         f"tau = {tau}, bucket = {bucket}, K = {K}")


def cclip_solve_torch(xs: Sequence[torch.Tensor], z: torch.Tensor,
                      iters: int = 3, tau: float = 0.0, bucket: int = 1,
                      perm=None):
    """Steps 1 to 5 of `cclip_round` directly on the vectors: returns (w,
    kept, s, tau_used) with w the [K] client weights, kept the ascending
    list of kept clients, s the [B] clip factors of the last iteration and
    tau_used the radius.  It reads the kept set on the host."""
    xs = list(xs)
    perm = _cclip_perm(perm, len(xs))
    sq = torch.stack([((x - z) ** 2).sum() for x in xs])
    keep = sq.isfinite().tolist()
    order = [k for k in perm if keep[k]]
    groups = [order[i:i + bucket] for i in range(0, len(order), bucket)]
    B = len(groups)
    w = torch.zeros_like(sq)
    if B == 0:
        return w, [], sq[:0], sq.new_zeros(())
    us = []
    for g in groups:
        u = torch.zeros_like(z)
        for k in g:
            u += xs[k] - z
        us.append(u / len(g))
    t = (sq.new_tensor(tau) if tau > 0 else
         torch.stack([u.norm() for u in us]).sort().values[(B - 1) // 2])
    c = sq.new_zeros(B)
    for _ in range(iters):
        v = torch.zeros_like(z)
        for b in range(B):
            v += c[b] * us[b]
        dist = torch.stack([(u - v).norm() for u in us])
        s = torch.where(dist > t, t / dist, torch.ones_like(dist))
        c = c * (1 - s.sum() / B) + s / B
    for b, g in enumerate(groups):
        w[g] = c[b] / len(g)
    return w, sorted(order), s, t


def cclip_round_torch(xs: Sequence[torch.Tensor], z: torch.Tensor,
                      rho: Optional[float] = None, mode: str = "fedavg",
                      iters: int = 3, tau: float = 0.0, bucket: int = 1,
                      perm=None):
    """The torch sequence that defines `cclip_round` (the rule is stated
    there), on the operands' device and in their dtype, directly on the
    vectors; returns (znew, res, w).  It reads the kept set on the host."""
    xs = list(xs)
    _check_cclip(len(xs), mode, iters, tau, bucket)
    w, kept, _, _ = cclip_solve_torch(xs, z, iters, tau, bucket, perm)
    znew = z.clone()
    for k in kept:
        znew += w[k] * (xs[k] - z)
    res = [torch.norm(z - znew) ** 2]
    if mode != "fedavg":
        res += [torch.norm(rho * (x - znew)) ** 2 for x in xs]
    return znew, torch.stack(res), w


def cclip_round(xs: Sequence[torch.Tensor], z: torch.Tensor,
                rho: Optional[float] = None, mode: str = "fedavg",
                iters: int = 3, tau: float = 0.0, bucket: int = 1, perm=None):
    """One centred-clipping aggregation round (Karimireddy, He and Jaggi,
    2021) with bucketing (the same authors, 2022) over the K client vectors
    `xs`: no client is dropped, there is no breakdown point at a fixed
    number of bad clients, and the clip radius bounds how far any set of
    clients moves the consensus: ||znew - z|| <= iters * tau.  The rule:

      1. keep[k] = sum((xs[k] - z)^2) is finite, as in `geomed_round`.
         K' = number kept; K' = 0 gives w = 0 and znew = z.
      2. Buckets: walk perm[0..K-1] (a permutation of 0..K-1, None = the
         identity), skip the clients that are not kept and cut the rest
         into consecutive groups of `bucket` = s; the last may be smaller,
         B = ceil(K' / s).  u_b = the mean of xs[k] - z over bucket b.
      3. The radius is `tau` if tau > 0, else the median of the ||u_b||:
         the value at 0-based index (B - 1) // 2 of the ascending values.
      4. c = 0 in R^B; exactly `iters` times dist_b = ||u_b - sum_j c_j u_j||,
         s_b = tau / dist_b if dist_b > tau else 1, S = sum_b s_b and
         c_b <- c_b (1 - S / B) + s_b / B, which is
         v <- v + (1 / B) sum_b s_b (u_b - v) written in coefficients.
      5. w_k = c_b(k) / |bucket b(k)| for kept k, 0 otherwise.  The weights
         need not sum to 1.
      6. znew = z.clone(); znew += w[k] * (xs[k] - z) for kept k ascending.

    Bucketing with a fresh random `perm` per round is what makes the rule
    (and any robust rule) usable on non-IID shards: the bucket means are
    closer to each other than the clients are.

    Returns (znew, res, w): znew and res as `robust_round` (res[1 + k] for
    all K clients in fedprox mode, NaN for a NaN client), w the fp32 [K]
    weights on z's device, formed without a host sync.  Modes are fedavg and
    fedprox; 1 <= iters <= 1024, tau finite and >= 0, 1 <= bucket <= K.
    `perm` is a sequence or a CPU tensor: its contents are checked on the
    host.  On the GPU (csrc/cclip.hip, K <= 32) the buckets are a
    contraction of the MFMA Gram matrix of xs[k] - z and the iteration runs
    on that B x B matrix: two passes over the operands whatever `iters` and
    `bucket` are, and znew is bitwise the sequence of step 6 over the
    kernel's own w and keep; w agrees with `cclip_round_torch`, the CPU
    path, to the Gram matrix's rounding.  A distance is inaccurate only
    where a bucket is close to the iterate, and there its clip factor is
    exactly 1.
    """
    xs = list(xs)
    if mode != "fedavg" and mode != "admm":
        assert rho is not None, f"{mode} needs rho"
    if _use_native(z):
        assert mode in AGGREGATE_MODES, f"unknown mode {mode!r}"
        from . import require_ext
        perm = torch.tensor(_cclip_perm(perm, len(xs)), dtype=torch.int32)
        znew, res, w, _, _, _ = require_ext().cclip_round(
            xs, z, 0.0 if rho is None else float(rho),
            AGGREGATE_MODES.index(mode), int(iters), float(tau), int(bucket),
            perm.to(z.device))
        return znew, res, w
    return cclip_round_torch(xs, z, rho, mode, iters, tau, bucket, perm)


def bulyan_params(trim_frac: float, K: int):
    """(f, theta, beta) of a Bulyan round: f = floor(trim_frac * K) clients
    may be bad, theta = K - 2 f are selected and beta = K - 4 f values are
    averaged per coordinate.  Needs K >= 4 f + 3."""
    f = math.floor(trim_frac * K)
    _check_bulyan(K, f, "fedavg")
    return f, K - 2 * f, K - 4 * f


def _check_bulyan(K: int, f: int, mode: str):
    if mode == "admm":
        raise ValueError("there is no robust ADMM round; use fedavg or fedprox")
    assert mode in AGGREGATE_MODES, f"unknown mode {mode!r}"
    if f < 0 or K < 4 * f + 3:
        raise ValueError(f"Bulyan needs f >= 0 and K >= 4 f + 3, got f = {f} "
                         f"of K = {K}")


def bulyan_window_torch(xs: Sequence[torch.Tensor], sel: torch.Tensor,
                        f: int) -> torch.Tensor:
    """Steps 3 and 4 of `bulyan_round` over the clients of the bool mask
    `sel`: znew, bit for bit."""
    picked = sel.nonzero().flatten().tolist()
    theta, beta = len(picked), len(picked) - 2 * f
    s = torch.sort(torch.stack([xs[k] for k in picked]), dim=0).values
    mid = (theta - 1) // 2
    med = s[mid]
    first = max(0, mid - beta + 1)
    lo = torch.full(med.shape, first, dtype=torch.long, device=med.device)
    go = torch.ones_like(lo, dtype=torch.bool)
    for c in range(first, min(mid, theta - beta)):
        go &= (s[c + beta] - med) < (med - s[c])
        lo += go
    znew = torch.zeros_like(med)
    for r in range(beta):
        znew += s.gather(0, (lo + r)[None])[0]
    znew /= beta
    return znew


def bulyan_round_torch(xs: Sequence[torch.Tensor], z: torch.Tensor,
                       rho: Optional[float] = None, mode: str = "fedavg",
                       f: int = 0):
    """The torch sequence that defines `bulyan_round` (the rule is stated
    there), on the operands' device and in their dtype, directly on the
    vectors; returns (znew, res, sel).  It reads each pick on the host."""
    xs = list(xs)
    K = len(xs)
    _check_bulyan(K, f, mode)
    D = _pairwise_sqdist_torch(xs)
    inf = torch.full_like(D, math.inf)
    D.fill_diagonal_(math.inf)          # D_ii is excluded
    sel = torch.zeros(K, dtype=torch.bool, device=z.device)
    for t in range(K - 2 * f):
        q = max(1, K - t - f - 2)
        near = torch.sort(torch.where(sel[None, :], inf, D), dim=1,
                          stable=True).values
        score = torch.zeros_like(near[:, 0])
        if K - t > 1:                   # a lone remaining client scores 0
            for r in range(q):          # ascending order
                score += near[:, r]
        left = (~sel).nonzero().flatten()
        sel[left[torch.argsort(score[left], stable=True)[0]]] = True
    znew = bulyan_window_torch(xs, sel, f)
    res = [torch.norm(z - znew) ** 2]
    if mode != "fedavg":
        res += [torch.norm(rho * (x - znew)) ** 2 for x in xs]
    return znew, torch.stack(res), sel


def bulyan_round(xs: Sequence[torch.Tensor], z: torch.Tensor,
                 rho: Optional[float] = None, mode: str = "fedavg", f: int = 0,
                 center: Optional[torch.Tensor] = None):
    """One Bulyan aggregation round (El Mhamdi, Guerraoui and Rouault, 2018)
    over the K client vectors `xs`, of which up to `f` may be Byzantine,
    K >= 4 f + 3.  Krum accepts a client that is close to the others in norm
    but wrong in a few coordinates; the coordinate-wise rules accept one whose
    every coordinate is in range while the vector is not.  Bulyan runs both:
    theta = K - 2 f clients are selected by iterated Krum and, per
    coordinate, the beta = K - 4 f selected values closest to their median
    are averaged.  f = 0 is the plain mean.  The rule:

      1. D is `pairwise_sqdist`: a non-finite entry counts as +inf, the
         diagonal is zero, the matrix is exactly symmetric.
      2. R = all K clients; theta times: q = max(1, |R| - f - 2) (the clamp
         serves the last iterations, where |R| < f + 3), score_i for i in R
         is the sum of the q smallest D_ij over the other j in R, added in
         ascending order (a lone remaining client scores 0), and the client
         of lowest score, ties to the lower index, moves from R to S.  With
         q = 1 two mutually nearest clients share one D entry and tie
         exactly; D's symmetry makes the index decide alike on every path.
      3. Per coordinate, s = the theta values of S in torch.sort's order
         (-inf < finite < +inf < NaN), mid = (theta - 1) // 2, med = s[mid],
         lo = max(0, mid - beta + 1), go = True, and for
         c = lo ... min(mid, theta - beta) - 1:
         go &= (s[c + beta] - med) < (med - s[c]); lo += go.  The window
         s[lo .. lo + beta - 1] always holds the median and, away from ties,
         is the beta values closest to it; a NaN compares false and never
         enters by sliding.  At most 2 f steps.
      4. znew = zeros; znew += s[lo + r] for r = 0 .. beta - 1; znew /= beta.

    Returns (znew, res, sel): znew and res as `robust_round` (res[1 + k] for
    all K clients in fedprox mode, NaN for a NaN client), sel the bool [K]
    mask of S on z's device, formed without a host sync.  Modes are fedavg
    and fedprox.  On the GPU (csrc/bulyan.hip, K <= 32) the distances come
    from the MFMA Gram pass around `center` (None means z), the selection
    runs in one workgroup and the window in a sorting-network pass; znew is
    bitwise steps 3 and 4 of `bulyan_round_torch`, the CPU path, over the
    same selection.
    """
    xs = list(xs)
    if mode != "fedavg" and mode != "admm":
        assert rho is not None, f"{mode} needs rho"
    if _use_native(z):
        if mode == "admm":
            raise ValueError("there is no robust ADMM round; use fedavg or "
                             "fedprox")
        assert mode in AGGREGATE_MODES, f"unknown mode {mode!r}"
        from . import require_ext
        znew, res, sel, _, _ = require_ext().bulyan_round(
            xs, z, z if center is None else center,
            0.0 if rho is None else float(rho), AGGREGATE_MODES.index(mode),
            int(f))
        return znew, res, sel.bool()
    return bulyan_round_torch(xs, z, rho, mode, f)


def bb_stats(y: torch.Tensor, yhat0: torch.Tensor, x: torch.Tensor,
             z: torch.Tensor, x0: torch.Tensor) -> torch.Tensor:
    """fp32 [6] = (a.a, a.b, b.b, a.dx, b.dx, dx.dx) with a = y - yhat0,
    b = x - z, dx = x - x0 (the BB spectral-stepsize statistics)."""
    if _use_native(y):
        from . import require_ext
        return require_ext().bb_stats(y.contiguous(), yhat0.contiguous(),
                                      x.contiguous(), z.contiguous(),
                                      x0.contiguous())
    a = y - yhat0
    b = x - z
    dx = x - x0
    return torch.stack([a.dot(a), a.dot(b), b.dot(b),
                        a.dot(dx), b.dot(dx), dx.dot(dx)])


def bb_stats_round(ys: Sequence[torch.Tensor], yhat0s: Sequence[torch.Tensor],
                   xs: Sequence[torch.Tensor], z: torch.Tensor,
                   x0s: Sequence[torch.Tensor]) -> torch.Tensor:
    """fp32 [K, 6] on z's device: row k is bb_stats(ys[k], yhat0s[k], xs[k],
    z, x0s[k]), bit for bit.  On the GPU the K <= 32 clients are served by
    one pass (csrc/consensus.hip) that reads z once per 4 clients, so a BB
    round costs one host read instead of K."""
    ys, yhat0s, xs, x0s = list(ys), list(yhat0s), list(xs), list(x0s)
    if not len(ys) == len(yhat0s) == len(xs) == len(x0s) >= 1:
        raise ValueError("bb_stats_round needs K >= 1 vectors in every list")
    if _use_native(z):
        from . import require_ext
        return require_ext().bb_stats_round(ys, yhat0s, xs, z, x0s)
    return torch.stack([bb_stats(ys[k], yhat0s[k], xs[k], z, x0s[k])
                        for k in range(len(xs))])
