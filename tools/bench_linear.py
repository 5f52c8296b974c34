#!/usr/bin/env python3
"""Microbenchmark: the bf16 MFMA fc kernels (csrc/linear_mfma.hip) against
the library path FedLinear took for the same layers before them, same
process, same inputs.

    python tools/bench_linear.py [--out FILE.md]

Layers: Net1 fc1 (K = 1600, N = 512) and Net2 fc4 (K = 512, N = 1024), at
batch 128 (the drivers' batch) and 512.  Per layer and batch the three passes
are timed one by one:
  fwd         linear_mfma_fwd         | F.linear(x, w, b) on bf16
  bwd-data    linear_mfma_bwd_data    | gy @ w
  bwd-weight  linear_mfma_bwd_weight  | gy.T @ x and gy.sum(0)
The right-hand side is what autograd runs for F.linear's backward.  `sum` is
the three medians added.

Method: every case is warmed, then SAMPLES samples per path taken alternately
(new, library, new, ...), each sample ITERS back-to-back calls between two
device events; the figure is the median sample in microseconds per call.  The
whole comparison is repeated REPEATS times; the spread of a sum is its
largest minus its smallest value over the repeats.  Needs a GPU; there is no
CPU fallback for a timing.
"""

import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from fedkit import ops  # noqa: E402

LAYERS = {"Net1 fc1": (1600, 512), "Net2 fc4": (512, 1024)}
BATCHES = (128, 512)
WARMUP, ITERS, SAMPLES, REPEATS = 30, 300, 7, 3


def sample_us(fn):
    s = torch.cuda.Event(enable_timing=True)
    e = torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(ITERS):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / ITERS * 1000.0


def ab(fn_a, fn_b):
    """Median us/call of two callables, samples taken alternately."""
    for _ in range(WARMUP):
        fn_a()
        fn_b()
    torch.cuda.synchronize()
    a, b = [], []
    for _ in range(SAMPLES):
        a.append(sample_us(fn_a))
        b.append(sample_us(fn_b))
    return statistics.median(a), statistics.median(b)


def passes(M, K, N):
    """[(name, new, library)] on one set of inputs"""
    ext = ops.require_ext()
    g = torch.Generator().manual_seed(0)
    bf = lambda t: t.to("cuda", torch.bfloat16)  # noqa: E731
    x = bf(torch.randn(M, K, generator=g))
    w = bf(torch.randn(N, K, generator=g) * 0.05)
    gy = bf(torch.randn(M, N, generator=g))
    b = torch.randn(N, generator=g).cuda()
    b16 = b.to(torch.bfloat16)
    return [
        ("fwd", lambda: ext.linear_mfma_fwd(x, w, b),
         lambda: F.linear(x, w, b16)),
        ("bwd-data", lambda: ext.linear_mfma_bwd_data(gy, w),
         lambda: gy @ w),
        ("bwd-weight", lambda: ext.linear_mfma_bwd_weight(gy, x, True),
         lambda: (gy.t() @ x, gy.sum(0))),
    ]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the table here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_linear needs a GPU")
    lines = ["| layer | batch | pass | repeat | mfma us | library us | "
             "library/mfma |", "|---|---:|---|---:|---:|---:|---:|"]
    sums = {}
    for rep in range(REPEATS):
        for layer, (K, N) in LAYERS.items():
            for M in BATCHES:
                tot_a = tot_b = 0.0
                for name, fa, fb in passes(M, K, N):
                    ta, tb = ab(fa, fb)
                    tot_a += ta
                    tot_b += tb
                    lines.append(f"| {layer} | {M} | {name} | {rep} | {ta:.2f} "
                                 f"| {tb:.2f} | {tb / ta:.2f}x |")
                    print(lines[-1], flush=True)
                sums.setdefault((layer, M), []).append((tot_a, tot_b))
    lines += ["", "| layer | batch | sum mfma us (per repeat) | sum library us "
              "(per repeat) | spread mfma / library us | library/mfma "
              "(medians) |", "|---|---:|---|---|---:|---:|"]
    for (layer, M), s in sums.items():
        a, b = [v[0] for v in s], [v[1] for v in s]
        fmt = lambda v: " ".join(f"{t:.2f}" for t in v)  # noqa: E731
        lines.append(
            f"| {layer} | {M} | {fmt(a)} | {fmt(b)} | {max(a) - min(a):.2f} / "
            f"{max(b) - min(b):.2f} | "
            f"{statistics.median(b) / statistics.median(a):.2f}x |")
        print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
