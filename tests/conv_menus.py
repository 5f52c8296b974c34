"""Conv shape menus shared by the GPU numerics tests (test_ops_gpu.py,
test_bn_gpu.py) and the CPU planner test (test_conv_plan.py), plus the
geometry that turns a menu row into the integer arguments the launch planner
(csrc/conv_plan.h) receives from the host wrappers.  Plain data and integer
arithmetic: importing this needs neither torch nor a GPU."""

FWD, BWD, BANK = 0, 1, 2           # conv_plan's caller argument

RESNET_SHAPES = [
    # (N, C, H, K, R, stride) — the ResNet18 CIFAR conv menu;
    # pad = 1 for R == 3, else 0
    (16, 64, 32, 64, 3, 1),
    (16, 64, 32, 128, 3, 2),
    (16, 128, 16, 128, 3, 1),
    (16, 128, 16, 256, 3, 2),
    (16, 256, 8, 256, 3, 1),
    (16, 256, 8, 512, 3, 2),
    (16, 512, 4, 512, 3, 1),
    (16, 64, 32, 128, 1, 2),   # shortcut projections
    # N=64 so the stride-2 even/odd-plane dw fast path qualifies
    # ((N*Hp*Wp/2) % 64 == 0 — N=16 falls back to the library path)
    (64, 64, 32, 128, 3, 2),
    (64, 128, 16, 256, 3, 2),
    (16, 128, 16, 256, 1, 2),
    (16, 256, 8, 512, 1, 2),
    # bench-size layer4 shapes: Q == 4, so dw takes the library path
    (128, 512, 4, 512, 3, 1),
    (128, 256, 8, 512, 3, 2),
    # smallest shapes that reach the remaining kernel variants (the planner
    # test checks that the menus cover every instantiated kernel)
    (8, 64, 32, 512, 1, 1),    # fwd: 128-row stride-1 plain
    (8, 64, 64, 512, 1, 2),    # fwd: 128-row stride-2 plain
    (8, 512, 32, 64, 3, 1),    # bwd-data: 128-row virtual-pad-1 plain
    (64, 128, 16, 128, 3, 1),  # bwd-data: 128-row virtual-pad-1 split-K
    (4, 64, 8, 64, 1, 1),      # bwd-weight: dw_gemm<64, stride 1>
    (4, 64, 16, 64, 1, 2),     # bwd-weight: dw_gemm<64, stride 2>
]

VAE_CPC_CONVS = [
    # (Cin, Kout, H, ksize, stride, pad, dil) at N = GEN_N — VAE encoder
    # 4x4-s2 chain (simple_models.py:249-255) and the CPC dilated bank / 2x2 /
    # 1x1 convs (simple_models.py:441-460, 478-481, 503-504)
    (3, 12, 32, 4, 2, 1, 1),
    (12, 24, 16, 4, 2, 1, 1),
    (24, 48, 8, 4, 2, 1, 1),
    (48, 96, 4, 4, 2, 1, 1),
    (8, 8, 32, 4, 2, 3, 2),      # CPC dilated bank d=2
    (8, 8, 32, 4, 2, 6, 4),      # d=4
    (8, 8, 32, 4, 2, 24, 16),    # d=16
    (40, 256, 16, 4, 2, 1, 1),   # CPC conv2 (8*5 -> latent/4)
    (256, 256, 6, 2, 1, 1, 1),   # CPC contextgen 2x2 pad 1
    (1024, 256, 4, 1, 1, 0, 1),  # CPC predictor 1x1
]
GEN_N = 16

# conv-epilogue BatchNorm statistics: (xp shape, Kout, R, stride) on a
# PRE-PADDED input; M and the tile regime of each row are in
# profiles/bn_numerics.md.  "window" = ceil(M/128) * Kout/64 in [256, 512),
# where the conv launches 64-row tiles.
BN_CONV_CASES = [
    ((2, 64, 11, 11), 128, 3, 1),     # BM64, M tail 34, two column blocks
    ((2, 64, 19, 19), 64, 3, 2),      # stride 2
    ((3, 64, 9, 9), 64, 1, 2),        # 1x1 projection
    ((4, 8, 35, 35), 512, 3, 1),      # window, M tail 4, Kg = 72 tail tile
    ((32, 64, 34, 34), 64, 3, 1),     # window, ResNet layer1 at batch 32
    ((8, 8, 35, 35), 512, 3, 1),      # BM128, M tail 8
    ((8, 8, 67, 67), 512, 3, 2),      # BM128 stride 2, M tail 8
]

# fused dilated bank, called directly: (N, C, H, R, stride, kt, dils, pads)
# with kt true out channels per tap.  Row 0 is the CPC encoder's bank; the
# others are the smallest that reach the stride-1 and the 128-row kernels
# (128-row needs ceil(M/128) >= 256).
BANK_CASES = [
    (9, 8, 32, 4, 2, 8, (1, 2, 4, 8, 16), (1, 3, 6, 12, 24)),
    (2, 8, 9, 4, 1, 16, (1, 3), (2, 5)),       # 64-row, stride 1, M tail
    (33, 8, 64, 4, 2, 8, (1, 2), (1, 3)),      # 128-row, stride 2
    (33, 8, 31, 4, 1, 16, (1, 3), (2, 5)),     # 128-row, stride 1
]


def _up(n, m):
    return (n + m - 1) // m * m


def fwd_plan_args(N, C, H, K, R, stride, pad, dil=1, ktrue=None, bn=False):
    """conv_plan arguments of the forward conv (C, K already padded to x8 /
    x64; ktrue = dense out channels)."""
    P = (H + 2 * pad - ((R - 1) * dil + 1)) // stride + 1
    dense = ktrue is None or ktrue == K
    return (N * P * P, K, R * R * C, stride, dense, bn, 0, FWD)


def bwd_data_plan_args(N, C, H, K, R, stride, pad, dil=1):
    """conv_plan arguments of dx = conv(gy, rot180(w)): out channels C rounded
    up to the 64-row tile, reduction over R*R*K."""
    P = (H + 2 * pad - ((R - 1) * dil + 1)) // stride + 1
    Cpad = _up(C, 64)
    dense = Cpad == C
    if R == 1 and stride == 2 and pad == 0:
        # 1x1 stride-2 shortcut: dense GEMM at the small resolution
        return (N * P * P, Cpad, K, 1, dense, False, 0, BWD)
    pl = (R - 1) * dil - pad
    vpad_ok = K % 64 == 0 and pl >= 0 and \
        (stride == 1 or (stride == 2 and H >= 16))
    return (N * H * H, Cpad, R * R * K, 1, dense, False,
            stride if vpad_ok else 0, BWD)


def dw_plan_args(N, C, H, K, R, stride, pad, dil=1):
    """dw_plan arguments of the bwd-weight GEMM."""
    P = (H + 2 * pad - ((R - 1) * dil + 1)) // stride + 1
    Hp = H + 2 * pad
    return (N, C, Hp, Hp, K, P, P, R, R, stride, dil)


def resnet_row(row):
    N, C, H, K, R, stride = row
    return dict(N=N, C=C, H=H, K=K, R=R, stride=stride,
                pad=1 if R == 3 else 0)


def gen_row(row):
    """A VAE_CPC_CONVS row as the padded shapes the generic path launches."""
    Cin, Kout, H, ks, stride, pad, dil = row
    return dict(N=GEN_N, C=_up(Cin, 8), H=H, K=_up(Kout, 64), R=ks,
                stride=stride, pad=pad, dil=dil), Kout


def bn_plan_args(case, bn):
    (N, C, Hp, _), Kout, R, stride = case
    return fwd_plan_args(N, C, Hp, Kout, R, stride, 0, bn=bn)


def bank_plan_args(case):
    N, C, H, R, stride, kt, dils, pads = case
    P = (H + 2 * pads[0] - ((R - 1) * dils[0] + 1)) // stride + 1
    return (N * P * P, 64, len(dils) * R * R * C, stride,
            kt * len(dils) == 64, False, 0, BANK)


def menu_conv_plan_args():
    """(label, conv_plan args) of every conv launch the GPU conv tests make
    from these menus."""
    out = []
    for row in RESNET_SHAPES:
        kw = resnet_row(row)
        out.append((("resnet", "fwd") + row, fwd_plan_args(**kw)))
        out.append((("resnet", "dx") + row, bwd_data_plan_args(**kw)))
    for row in VAE_CPC_CONVS:
        kw, ktrue = gen_row(row)
        out.append((("gen", "fwd") + row, fwd_plan_args(ktrue=ktrue, **kw)))
        out.append((("gen", "dx") + row, bwd_data_plan_args(**kw)))
    for case in BN_CONV_CASES:
        out.append((("bn", "stats") + case, bn_plan_args(case, True)))
        out.append((("bn", "plain") + case, bn_plan_args(case, False)))
    for case in BANK_CASES:
        out.append((("bank", "fwd") + case, bank_plan_args(case)))
    return out


# every distinct conv of ResNet18 on 32x32 inputs (the benchmark's workload,
# at batch BENCH_N): (C, H, K, R, stride).  conv1 (C = 3) runs the small-C
# direct kernel forward and needs no dx; only its bwd-weight is planned.
RESNET18_CONVS = [
    (64, 32, 64, 3, 1),                                          # layer1
    (64, 32, 128, 3, 2), (128, 16, 128, 3, 1), (64, 32, 128, 1, 2),
    (128, 16, 256, 3, 2), (256, 8, 256, 3, 1), (128, 16, 256, 1, 2),
    (256, 8, 512, 3, 2), (512, 4, 512, 3, 1), (256, 8, 512, 1, 2),
]
RESNET18_CONV1 = (3, 32, 64, 3, 1)
BENCH_N = 128


def bench_conv_plan_args():
    out = []
    for row in RESNET18_CONVS:
        kw = resnet_row((BENCH_N,) + row)
        out.append((("bench", "fwd") + row, fwd_plan_args(**kw)))
        out.append((("bench", "dx") + row, bwd_data_plan_args(**kw)))
    return out


def bench_dw_plan_args():
    return [(("bench", "dw") + row,
             dw_plan_args(**resnet_row((BENCH_N,) + row)))
            for row in RESNET18_CONVS + [RESNET18_CONV1]]


def menu_dw_plan_args():
    out = []
    for row in RESNET_SHAPES:
        out.append((("resnet", "dw") + row, dw_plan_args(**resnet_row(row))))
    for row in VAE_CPC_CONVS:
        out.append((("gen", "dw") + row, dw_plan_args(**gen_row(row)[0])))
    return out
