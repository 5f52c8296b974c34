#!/usr/bin/env python3
"""Microbenchmark: info_nce forward + backward, native kernels against the
torch sequence (two norms, two divides, GEMM, softmax, diagonal, log, sum and
their autograd chain), same process, same inputs.

    python tools/bench_infonce.py [--out FILE.md]

D = batch * Rc = 4096 (the CPC driver's defaults), fp32, P = 49, 105, 225,
1024 as (px, py) = (7, 7), (15, 7), (15, 15), (32, 32).  P = 49 runs the
one-workgroup kernel of csrc/losses_extra.hip and is there for the record;
the others run csrc/infonce_tiled.hip.  The torch column is what info_nce
ran above P = 64 before the tiled kernels (ops._NATIVE_ENV = False).

Method: warm-up of both paths, then SAMPLES samples per path taken
alternately (native, torch, native, ...), each sample ITERS back-to-back
forward + backward calls between two device events; the figure is the median
sample in microseconds per call, the spread is max - min of the samples.  The
whole table is then taken again with the torch path first.  Needs a GPU.
"""

import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from fedkit import ops  # noqa: E402
from fedkit.ops.losses import info_nce  # noqa: E402

BATCH, RC = 128, 32
GRIDS = [(7, 7), (15, 7), (15, 15), (32, 32)]
WARMUP, ITERS, SAMPLES = 20, 20, 15


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
    """Median and spread (us/call) of two callables, sampled alternately."""
    for _ in range(WARMUP):
        fn_a()
        fn_b()
    torch.cuda.synchronize()
    a, b = [], []
    for _ in range(SAMPLES):
        a.append(sample_us(fn_a))
        b.append(sample_us(fn_b))
    return (statistics.median(a), max(a) - min(a),
            statistics.median(b), max(b) - min(b))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the table here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_infonce needs a GPU")
    lines = ["| P | D | order | native us | torch us | torch/native | "
             "spread native/torch us |",
             "|---:|---:|---|---:|---:|---:|---:|"]
    for order in ("native first", "torch first"):
        for px, py in GRIDS:
            g = torch.Generator().manual_seed(0)
            z, zhat = (torch.randn(BATCH, RC, px, py, generator=g)
                       .cuda().requires_grad_() for _ in range(2))

            def run(native):
                def fn():
                    old = ops._NATIVE_ENV
                    ops._NATIVE_ENV = native
                    try:
                        z.grad = zhat.grad = None
                        info_nce(z, zhat).backward()
                    finally:
                        ops._NATIVE_ENV = old
                return fn

            if order == "native first":
                na, sa, tb, sb = ab(run(True), run(False))
            else:
                tb, sb, na, sa = ab(run(False), run(True))
            lines.append(f"| {px * py} | {BATCH * RC} | {order} | {na:.1f} | "
                         f"{tb:.1f} | {tb / na:.2f}x | {sa:.1f} / {sb:.1f} |")
            print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
