#!/usr/bin/env python3
"""Microbenchmark: fused consensus penalty / ADMM statistics vs the torch
expressions they replace, same process, same inputs.

    python tools/bench_penalty.py [--out FILE.md] [--section NAME]

Two parameter lists: Net2's largest fc block (fc4: [1024,512] + [1024]) and
ResNet18's last conv block (two channels_last [512,512,3,3] weights + four
[512] BatchNorm vectors).  Random z and y, rho=0.1, lambda1=lambda2=1e-4.

Timed per list, for each of the two paths:
  fwd+bwd   penalty value, then backward into the parameters' .grad
  fwd       value only under no_grad (an LBFGS line-search probe)
and bb_stats against the six-dot form (device time, and wall time including
the host read of the six numbers, which is how the BB update consumes them).

Section `aggregate`: one aggregation round of K = 10 local clients,
consensus.aggregate_round against the torch sequence the strategies run
with --fused_aggregate 0 (clones, K adds, divide, norms, per-client dual
update), for fedavg / fedprox / admm at the ResNet18 last conv block's N and
at its linear head's N (512*10 + 10).  Device time, and for fedprox / admm
wall time including the host reads of the residuals (one .tolist() against
K+1 .item() calls).

Section `bb`: one adaptive-rho (BB) round of K = 10 local clients at the
same two N.  Fused: bb_stats_round, then aggregate_round with the full
carry.  Sequence: what ConsensusADMM ran for that round before the two
existed: bb_stats per client, then per client `y + rho_used * (x - z)` and
`x.clone()`, then aggregate_round.  The wall rows add the host reads (one
.tolist() of the [K, 6] statistics against K, and the residuals' .tolist()
on both sides); the host rho chain between the passes is the same code on
both sides and is not timed.

Section `robust`: one robust round of K = 10 local clients at the same two
N, consensus.robust_round (csrc/robust.hip) against the torch sequence that
defines it (stack, sort along the client axis, adds in rank order, divide,
norms), for fedavg / fedprox with trim = 1 and the median.  A further row
per mode times it against the plain mean of aggregate_round at the same K
and N (the same bytes read): the price of robustness.  Device time.

Section `krum`: one Multi-Krum round (f = K // 5, m = K - f) at K = 10 and
K = 32, N of the ResNet18 last conv block, fedavg / fedprox:
consensus.krum_round (csrc/krum.hip) against krum_round_torch on the GPU
(K (K - 1) / 2 difference reductions and a host read of the selection), and
further rows against robust_round (trim = f) and the plain mean of
aggregate_round at the same K and N.  Device time; the torch sequence is
timed by the wall clock, since it reads the selection on the host.

Section `geomed`: one geometric-median round (iters = 16) at K = 10 and
K = 32, the two N of `aggregate`, fedavg / fedprox: consensus.geomed_round
(csrc/geomed.hip) against geomed_round_torch on the GPU (wall: it reads the
kept set on the host), and device-time rows against krum_round (Multi-Krum,
f = K // 5) and the plain mean of aggregate_round.  Two further rows per K
time the same round with iters = 1 and iters = 1024: the differences are
the solver's iterations alone.

Section `cclip`: one centred-clipping round (iters = 3) at the K and N of
`geomed`, fedavg / fedprox, bucket s = 1 and s = 2 (a seeded permutation):
consensus.cclip_round (csrc/cclip.hip) against cclip_round_torch on the GPU
(wall: it reads the kept set on the host), and a device-time row against
geomed_round at the same K, N and iters.  One further row per K times
iters = 3 against iters = 1024.

Section `bulyan`: one Bulyan round at K = 10, f = 1 (fedavg / fedprox) and
K = 32, f = 7 (fedavg), N of the ResNet18 last conv block:
consensus.bulyan_round (csrc/bulyan.hip) against bulyan_round_torch on the GPU
(wall: it reads every pick on the host), and a device-time row against
krum_round (Multi-Krum, the same f).

Method: warm-up, then SAMPLES samples per path taken alternately (fused,
torch, fused, ...), each sample ITERS back-to-back calls between two device
events; the reported figure is the median sample in microseconds per call.
Needs a GPU; there is no CPU fallback for a timing.
"""

import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from fedkit.ops import consensus  # noqa: E402

RHO, L1, L2 = 0.1, 1e-4, 1e-4
WARMUP, ITERS, SAMPLES = 30, 50, 21


def param_lists(dev):
    g = torch.Generator().manual_seed(0)

    def rn(*s):
        return (torch.randn(*s, generator=g) * 0.05).to(dev)

    net2_fc = [rn(1024, 512), rn(1024)]
    conv = lambda: rn(512, 512, 3, 3).contiguous(  # noqa: E731
        memory_format=torch.channels_last)
    resnet_last = [conv(), rn(512), rn(512), conv(), rn(512), rn(512)]
    return {"Net2 fc4 block": net2_fc, "ResNet18 last conv block": resnet_last}


def flat_physical(p):
    if p.dim() == 4 and p.is_contiguous(memory_format=torch.channels_last):
        return p.permute(0, 2, 3, 1).reshape(-1)
    return p.reshape(-1)


def torch_penalty(params, z, y):
    """The closure's expression sequence on the torch path."""
    vec = torch.cat([flat_physical(p) for p in params])
    xdelta = vec - z
    pen = torch.dot(y, xdelta) + 0.5 * RHO * (torch.norm(xdelta, 2) ** 2)
    pen = pen + L1 * torch.norm(vec, 1)
    return pen + L2 * (torch.norm(vec, 2) ** 2)


def fused_penalty(params, z, y):
    return consensus.penalty(params, z=z, y=y, rho=RHO, lambda1=L1,
                             lambda2=L2)


def sample_us(fn):
    s = torch.cuda.Event(enable_timing=True)
    e = torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(ITERS):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / ITERS * 1000.0


def sample_wall_us(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(ITERS):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / ITERS * 1e6


def ab(fn_a, fn_b, sampler=sample_us):
    """Median us/call of two callables, samples taken alternately."""
    for _ in range(WARMUP):
        fn_a()
        fn_b()
    torch.cuda.synchronize()
    a, b = [], []
    for _ in range(SAMPLES):
        a.append(sampler(fn_a))
        b.append(sampler(fn_b))
    return (statistics.median(a), statistics.median(b),
            max(a) - min(a), max(b) - min(b))


AGG_K = 10
AGG_SIZES = {"ResNet18 last conv block": 4720640, "ResNet18 head": 5130}


def torch_round(xs, z, ys, mode, read):
    """The strategies' sequence without the fused round (GPU form)."""
    K = len(xs)
    if mode == "admm":
        contrib = [y + RHO * x for x, y in zip(xs, ys)]
    else:
        contrib = [x.clone() for x in xs]
    znew = torch.zeros_like(contrib[0])
    for c in contrib:
        znew += c
    znew /= (K * RHO) if mode == "admm" else K
    dual = torch.norm(z - znew)
    if mode == "fedavg":
        return dual
    out = [dual.item() if read else dual]
    for k, x in enumerate(xs):
        if mode == "admm":
            sq = consensus.admm_dual_update(ys[k], x, znew, RHO)
        else:
            sq = torch.norm(RHO * (x - znew))
        out.append(sq.item() if read else sq)
    return out


def aggregate_section(dev, row):
    for name, n in AGG_SIZES.items():
        g = torch.Generator().manual_seed(2)
        xs = [(torch.randn(n, generator=g) * 0.05).to(dev)
              for _ in range(AGG_K)]
        z = (torch.randn(n, generator=g) * 0.05).to(dev)
        for mode in consensus.AGGREGATE_MODES:
            # duals start at 0 and are updated by every timed call of either
            # path; with constant x they stay finite (y_k sums to ~0)
            ya = [torch.zeros(n, device=dev) for _ in range(AGG_K)]
            yb = [torch.zeros(n, device=dev) for _ in range(AGG_K)]
            ys = lambda y: y if mode == "admm" else None  # noqa: E731

            def fused(read=False):
                znew, res = consensus.aggregate_round(xs, z, ys(ya), rho=RHO,
                                                      mode=mode)
                return res.tolist() if read else res

            zf, _ = consensus.aggregate_round(xs, z, ys([y.clone() for y in ya]),
                                              rho=RHO, mode=mode)
            print(f"{name} {mode}: znew finite {bool(zf.isfinite().all())}",
                  flush=True)
            row(f"{name}: {mode} round K={AGG_K} (device)", n,
                ab(fused, lambda: torch_round(xs, z, yb, mode, False)))
            if mode != "fedavg":
                row(f"{name}: {mode} round K={AGG_K} (wall, with host reads)",
                    n, ab(lambda: fused(True),
                          lambda: torch_round(xs, z, yb, mode, True),
                          sampler=sample_wall_us))


def bb_section(dev, row):
    K = AGG_K
    rho_used = [RHO * (1 + k / 64) for k in range(K)]
    for name, n in AGG_SIZES.items():
        g = torch.Generator().manual_seed(3)
        rn = lambda: (torch.randn(n, generator=g) * 0.05).to(dev)  # noqa: E731
        xs = [rn() for _ in range(K)]
        z = rn()
        # each path owns its duals and carry vectors and updates them on every
        # timed call; with constant x the duals stay finite (y_k sums to ~0)
        own = lambda: ([torch.zeros(n, device=dev) for _ in range(K)],  # noqa: E731
                       [rn() for _ in range(K)], [rn() for _ in range(K)])
        ya, ha, pa = own()
        yb, hb, pb = own()

        def fused(read=False):
            st = consensus.bb_stats_round(ya, ha, xs, z, pa)
            if read:
                st = st.tolist()
            _, res = consensus.aggregate_round(
                xs, z, ya, rho=RHO, mode="admm", x0s=pa, yhat0s=ha,
                rho_used=rho_used)
            return res.tolist() if read else res

        def sequence(read=False):
            for k in range(K):
                st = consensus.bb_stats(yb[k], hb[k], xs[k], z, pb[k])
                if read:
                    st = st.tolist()
            for k in range(K):
                hb[k] = yb[k] + rho_used[k] * (xs[k] - z)
                pb[k] = xs[k].clone()
            _, res = consensus.aggregate_round(xs, z, yb, rho=RHO,
                                               mode="admm")
            return res.tolist() if read else res

        # same numbers first: one round of each path from the same state
        fused()
        sequence()
        same = all(torch.equal(a, b) for a, b in zip(ya + ha + pa,
                                                      yb + hb + pb))
        print(f"{name} bb: y, yhat0, x0 of the two paths equal: {same}",
              flush=True)
        row(f"{name}: BB round K={K} (device)", n, ab(fused, sequence))
        row(f"{name}: BB round K={K} (wall, with host reads)", n,
            ab(lambda: fused(True), lambda: sequence(True),
               sampler=sample_wall_us))


def robust_section(dev, row):
    for name, n in AGG_SIZES.items():
        g = torch.Generator().manual_seed(4)
        xs = [(torch.randn(n, generator=g) * 0.05).to(dev)
              for _ in range(AGG_K)]
        z = (torch.randn(n, generator=g) * 0.05).to(dev)
        for mode in ("fedavg", "fedprox"):
            for label, trim in (("trim=1", 1), ("median", (AGG_K - 1) // 2)):
                def fused(trim=trim):
                    return consensus.robust_round(xs, z, RHO, mode, trim)

                def sequence(trim=trim):
                    return consensus.robust_round_torch(xs, z, RHO, mode,
                                                        trim)

                same = torch.equal(fused()[0], sequence()[0])
                print(f"{name} robust {mode} {label}: znew of the two paths "
                      f"equal: {same}", flush=True)
                row(f"{name}: robust {mode} {label} K={AGG_K} (device)", n,
                    ab(fused, sequence))
            row(f"{name}: robust {mode} trim=1 vs plain mean K={AGG_K} "
                "(device; columns: robust, mean, mean/robust)", n,
                ab(lambda: consensus.robust_round(xs, z, RHO, mode, 1),
                   lambda: consensus.aggregate_round(xs, z, rho=RHO,
                                                     mode=mode)))


def krum_section(dev, row):
    name, n = "ResNet18 last conv block", AGG_SIZES["ResNet18 last conv block"]
    for K in (10, 32):
        g = torch.Generator().manual_seed(5)
        z = (torch.randn(n, generator=g) * 0.05).to(dev)
        xs = [z + (torch.randn(n, generator=g) * 0.01).to(dev)
              for _ in range(K)]
        f = K // 5
        for mode in ("fedavg", "fedprox"):
            def fused():
                return consensus.krum_round(xs, z, RHO, mode, f)

            def sequence():
                return consensus.krum_round_torch(xs, z, RHO, mode, f)

            (za, _, sa), (zb, _, sb) = fused(), sequence()
            print(f"{name} krum {mode} K={K}: selection equal "
                  f"{torch.equal(sa, sb)}, znew equal {torch.equal(za, zb)}",
                  flush=True)
            row(f"{name}: multi_krum {mode} K={K} f={f} (wall)", n,
                ab(fused, sequence, sampler=sample_wall_us))
            row(f"{name}: multi_krum {mode} vs robust trim={f} K={K} "
                "(device; columns: krum, robust, robust/krum)", n,
                ab(fused,
                   lambda: consensus.robust_round(xs, z, RHO, mode, f)))
            row(f"{name}: multi_krum {mode} vs plain mean K={K} "
                "(device; columns: krum, mean, mean/krum)", n,
                ab(fused, lambda: consensus.aggregate_round(xs, z, rho=RHO,
                                                            mode=mode)))
        row(f"{name}: pairwise_sqdist K={K} vs fp32 A @ A.T of the centred "
            "stack (device)", n,
            ab(lambda: consensus.pairwise_sqdist(xs, z),
               lambda: (lambda A: A @ A.T)(torch.stack(xs) - z)))


def geomed_section(dev, row):
    for name, n in AGG_SIZES.items():
        for K in (10, 32):
            g = torch.Generator().manual_seed(6)
            z = (torch.randn(n, generator=g) * 0.05).to(dev)
            xs = [z + (torch.randn(n, generator=g) * 0.01).to(dev)
                  for _ in range(K)]
            f = K // 5
            for mode in ("fedavg", "fedprox"):
                def fused(iters=16):
                    return consensus.geomed_round(xs, z, RHO, mode, iters)

                def sequence():
                    return consensus.geomed_round_torch(xs, z, RHO, mode)

                (za, _, ca), (zb, _, cb) = fused(), sequence()
                print(f"{name} geomed {mode} K={K}: max |c - c_torch| / max c "
                      f"{float((ca - cb).abs().max() / cb.max()):.3g}, "
                      f"max |znew - znew_torch| "
                      f"{float((za - zb).abs().max()):.3g}", flush=True)
                row(f"{name}: geomed {mode} K={K} iters=16 (wall)", n,
                    ab(fused, sequence, sampler=sample_wall_us))
                row(f"{name}: geomed {mode} vs multi_krum f={f} K={K} "
                    "(device; columns: geomed, krum, krum/geomed)", n,
                    ab(fused,
                       lambda: consensus.krum_round(xs, z, RHO, mode, f)))
                row(f"{name}: geomed {mode} vs plain mean K={K} "
                    "(device; columns: geomed, mean, mean/geomed)", n,
                    ab(fused, lambda: consensus.aggregate_round(
                        xs, z, rho=RHO, mode=mode)))
            # the solver: 15 and 1008 further iterations of the same round
            def fedavg(iters=16):
                return consensus.geomed_round(xs, z, RHO, "fedavg", iters)

            row(f"{name}: geomed fedavg K={K} iters=16 vs iters=1 "
                "(device; columns: 16, 1, 1/16)", n,
                ab(fedavg, lambda: fedavg(1)))
            row(f"{name}: geomed fedavg K={K} iters=16 vs iters=1024 "
                "(device; columns: 16, 1024, 1024/16)", n,
                ab(fedavg, lambda: fedavg(1024)))


def cclip_section(dev, row):
    iters = 3
    for name, n in AGG_SIZES.items():
        for K in (10, 32):
            g = torch.Generator().manual_seed(7)
            z = (torch.randn(n, generator=g) * 0.05).to(dev)
            xs = [z + (torch.randn(n, generator=g) * 0.01).to(dev)
                  for _ in range(K)]
            perm = torch.randperm(K, generator=g)
            for mode in ("fedavg", "fedprox"):
                for s in (1, 2):
                    def fused(iters=iters, s=s):
                        return consensus.cclip_round(xs, z, RHO, mode, iters,
                                                     0.0, s, perm)

                    def sequence(s=s):
                        return consensus.cclip_round_torch(
                            xs, z, RHO, mode, iters, 0.0, s, perm)

                    (za, _, wa), (zb, _, wb) = fused(), sequence()
                    print(f"{name} cclip {mode} K={K} s={s}: max |w - w_torch|"
                          f" / max w {float((wa - wb).abs().max() / wb.max()):.3g}"
                          f", max |znew - znew_torch| "
                          f"{float((za - zb).abs().max()):.3g}", flush=True)
                    row(f"{name}: cclip {mode} K={K} s={s} iters={iters} "
                        "(wall)", n, ab(fused, sequence,
                                        sampler=sample_wall_us))
                    row(f"{name}: cclip {mode} s={s} vs geomed K={K} "
                        f"iters={iters} (device; columns: cclip, geomed, "
                        "geomed/cclip)", n,
                        ab(fused, lambda: consensus.geomed_round(
                            xs, z, RHO, mode, iters)))
            row(f"{name}: cclip fedavg K={K} s=2 iters={iters} vs iters=1024 "
                f"(device; columns: {iters}, 1024, 1024/{iters})", n,
                ab(lambda: consensus.cclip_round(xs, z, RHO, "fedavg", iters,
                                                 0.0, 2, perm),
                   lambda: consensus.cclip_round(xs, z, RHO, "fedavg", 1024,
                                                 0.0, 2, perm)))


def bulyan_section(dev, row):
    name, n = "ResNet18 last conv block", AGG_SIZES["ResNet18 last conv block"]
    for K, f, modes in ((10, 1, ("fedavg", "fedprox")), (32, 7, ("fedavg",))):
        g = torch.Generator().manual_seed(8)
        z = (torch.randn(n, generator=g) * 0.05).to(dev)
        xs = [z + (torch.randn(n, generator=g) * 0.01).to(dev)
              for _ in range(K)]
        for mode in modes:
            def fused():
                return consensus.bulyan_round(xs, z, RHO, mode, f)

            def sequence():
                return consensus.bulyan_round_torch(xs, z, RHO, mode, f)

            (za, _, sa), (zb, _, sb) = fused(), sequence()
            print(f"{name} bulyan {mode} K={K}: selection equal "
                  f"{torch.equal(sa, sb)}, znew equal {torch.equal(za, zb)}",
                  flush=True)
            row(f"{name}: bulyan {mode} K={K} f={f} (wall)", n,
                ab(fused, sequence, sampler=sample_wall_us))
            row(f"{name}: bulyan {mode} vs multi_krum f={f} K={K} "
                "(device; columns: bulyan, krum, krum/bulyan)", n,
                ab(fused, lambda: consensus.krum_round(xs, z, RHO, mode, f)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the table here")
    ap.add_argument("--section", default="all",
                    choices=["all", "penalty", "aggregate", "bb",
                             "robust", "krum", "geomed", "cclip",
                             "bulyan"])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_penalty needs a GPU")
    dev = torch.device("cuda")
    lines = ["| case | N | fused us | torch us | torch/fused | "
             "spread fused/torch us |",
             "|---|---:|---:|---:|---:|---:|"]

    def row(case, n, r):
        fa, tb, sa, sb = r
        lines.append(f"| {case} | {n} | {fa:.1f} | {tb:.1f} | {tb / fa:.2f}x "
                     f"| {sa:.1f} / {sb:.1f} |")
        print(lines[-1], flush=True)

    plists = param_lists(dev) if args.section in ("all", "penalty") else {}
    for name, params in plists.items():
        n = sum(p.numel() for p in params)
        g = torch.Generator().manual_seed(1)
        z = torch.randn(n, generator=g).to(dev) * 0.05
        y = torch.randn(n, generator=g).to(dev) * 0.05
        leaves = [p.requires_grad_() for p in params]

        # same numbers first: value and gradients of the two paths
        for p in leaves:
            p.grad = None
        vf = fused_penalty(leaves, z, y)
        vf.backward()
        gf = [p.grad.clone() for p in leaves]
        for p in leaves:
            p.grad = None
        vt = torch_penalty(leaves, z, y)
        vt.backward()
        gerr = max(float((a - p.grad).abs().max()) for a, p in zip(gf, leaves))
        print(f"{name}: fused {vf.item():.8g} torch {vt.item():.8g} "
              f"max |grad diff| {gerr:.3g}", flush=True)

        def fwd_bwd(fn):
            def run():
                for p in leaves:
                    p.grad = None
                fn(leaves, z, y).backward()
            return run

        def fwd(fn):
            def run():
                with torch.no_grad():
                    fn(leaves, z, y)
            return run

        row(f"{name}: penalty fwd+bwd", n,
            ab(fwd_bwd(fused_penalty), fwd_bwd(torch_penalty)))
        row(f"{name}: penalty fwd (no_grad)", n,
            ab(fwd(fused_penalty), fwd(torch_penalty)))

        yh, x, x0 = (torch.randn(n, generator=g).to(dev) for _ in range(3))

        def six_dots():
            a, b, dx = y - yh, x - z, x - x0
            return [a.dot(a), a.dot(b), b.dot(b),
                    a.dot(dx), b.dot(dx), dx.dot(dx)]

        row(f"{name}: bb_stats (device)", n,
            ab(lambda: consensus.bb_stats(y, yh, x, z, x0), six_dots))
        row(f"{name}: bb_stats (wall, with host read)", n,
            ab(lambda: consensus.bb_stats(y, yh, x, z, x0).tolist(),
               lambda: [float(v) for v in six_dots()],
               sampler=sample_wall_us))

        yy = torch.zeros(n, device=dev)

        def dual_torch():
            ydelta = RHO * (x - z)
            nrm = torch.norm(ydelta)
            yy.add_(ydelta)
            return nrm

        row(f"{name}: admm_dual_update (device)", n,
            ab(lambda: consensus.admm_dual_update(yy, x, z, RHO), dual_torch))

    if args.section in ("all", "aggregate"):
        aggregate_section(dev, row)
    if args.section in ("all", "bb"):
        bb_section(dev, row)
    if args.section in ("all", "robust"):
        robust_section(dev, row)
    if args.section in ("all", "krum"):
        krum_section(dev, row)
    if args.section in ("all", "geomed"):
        geomed_section(dev, row)
    if args.section in ("all", "cclip"):
        cclip_section(dev, row)
    if args.section in ("all", "bulyan"):
        bulyan_section(dev, row)

    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
