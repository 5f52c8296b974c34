#!/usr/bin/env python3
"""Microbenchmark: fused consensus penalty / ADMM statistics vs the torch
expressions they replace, same process, same inputs.

    python tools/bench_penalty.py [--out FILE.md]

Two parameter lists: Net2's largest fc block (fc4: [1024,512] + [1024]) and
ResNet18's last conv block (two channels_last [512,512,3,3] weights + four
[512] BatchNorm vectors).  Random z and y, rho=0.1, lambda1=lambda2=1e-4.

Timed per list, for each of the two paths:
  fwd+bwd   penalty value, then backward into the parameters' .grad
  fwd       value only under no_grad (an LBFGS line-search probe)
and bb_stats against the six-dot form (device time, and wall time including
the host read of the six numbers, which is how the BB update consumes them).

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the table here")
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

    for name, params in param_lists(dev).items():
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

    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
