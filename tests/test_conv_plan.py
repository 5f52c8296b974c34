"""CPU test of the conv launch planner (csrc/conv_plan.h, bound as
ext.conv_plan / ext.dw_plan): pure integer rules, no GPU.

The expected plans below are literals transcribed from the host code as it
stood before the planner existed (the nested bm64/splits/stages ladders of
conv_core, the dilated bank and the bwd-weight wrapper) — not produced by
the planner.  Tuple layouts:
  conv args (M, Kout, Kg, stride, dense, bnpart, vpad, caller)
  conv plan (BM, stride, mode, stages, vpad, multitap, grid_x, grid_y, splits)
  dw args   (N, C, Hp, Wp, K, P, Q, R, S, stride, dil)
  dw plan   (fast, BMK, NT, stride, rsc_tiles, grid_y, splits,
             mtiles_per_split, two_stage, chunks); the fast path's fields are
             0 on the library path and chunks is 0 on the fast path
"""

import pytest

import conv_menus as cm


def _ext():
    import fedkit.ops
    if not fedkit.ops.has_ext():
        pytest.skip("fedkit._C is not built (python __graft_entry__.py build)")
    return fedkit.ops.ext()


def _check(table, rows, plan):
    assert [a for a, _ in table] == [a for _, a in rows], \
        "the menus changed: re-derive the expected plans by hand"
    for (args, want), (label, _) in zip(table, rows):
        assert tuple(plan(*args)) == want, (label, args)


def test_conv_plans_of_test_menus():
    _check(MENU_CONV, cm.menu_conv_plan_args(), _ext().conv_plan)


def test_conv_plans_of_benchmark_workload():
    _check(BENCH_CONV, cm.bench_conv_plan_args(), _ext().conv_plan)


def test_dw_plans_of_test_menus():
    _check(MENU_DW, cm.menu_dw_plan_args(), _ext().dw_plan)


def test_dw_plans_of_benchmark_workload():
    _check(BENCH_DW, cm.bench_dw_plan_args(), _ext().dw_plan)


@pytest.mark.parametrize("caller,bnpart", [
    (cm.FWD, False), (cm.FWD, True), (cm.BWD, False), (cm.BWD, True),
    (cm.BANK, False)])                  # the bank has no BN epilogue
@pytest.mark.parametrize("wg128", [255, 256, 511, 512])
def test_tile_rows_match_grid_at_thresholds(caller, wg128, bnpart):
    """The boundary behind the BN partials overrun: whichever tile the
    caller's threshold picks at ceil(M/128) * Kout/64 = wg128, grid_x is the
    row count of THAT tile, and the BN slab [grid_y][grid_x][2][64] is sized
    from the same two numbers."""
    plan = _ext().conv_plan
    for Kout in ([64] if caller == cm.BANK else [64, 128, 192]):
        gy = Kout // 64
        if wg128 % gy:
            continue
        t128 = wg128 // gy
        for M in (t128 * 128, t128 * 128 - 127, t128 * 128 - 64,
                  t128 * 128 - 63):
            assert -(-M // 128) * gy == wg128
            BM, _, mode, _, _, _, grid_x, grid_y, splits = plan(
                M, Kout, 576, 1, True, bnpart, 0, caller)
            want_bm = 64 if wg128 < (512 if caller == cm.FWD else 256) \
                else 128
            assert BM == want_bm, (M, Kout)
            assert grid_x == -(-M // BM) and grid_y == gy, (M, Kout)
            if bnpart:      # conv_core allocates grid_y * grid_x slab rows
                assert mode == 1 and splits == 1


def test_menus_cover_every_instantiated_kernel():
    """The GPU conv tests' menus select exactly the kernels the dispatch
    tables instantiate: no variant is built untested, none is missing."""
    ext = _ext()
    conv = {tuple(ext.conv_plan(*a))[:6] for _, a in cm.menu_conv_plan_args()}
    assert conv == {tuple(v[:5]) + (bool(v[5]),) for v in ext.conv_variants()}
    dw = {(p[1], p[3], p[2]) for p in
          (tuple(ext.dw_plan(*a)) for _, a in cm.menu_dw_plan_args()) if p[0]}
    assert dw == {tuple(v) for v in ext.dw_variants()}
    assert len(ext.conv_variants()) == 23 and len(ext.dw_variants()) == 5


MENU_CONV = [
    ((16384, 64, 576, 1, True, False, 0, 0),
     (64, 1, 2, 2, 0, False, 256, 1, 2)),  # resnet fwd 16 64 32 64 3 1
    ((16384, 64, 576, 1, True, False, 1, 1),
     (64, 1, 2, 3, 1, False, 256, 1, 2)),  # resnet dx 16 64 32 64 3 1
    ((4096, 128, 576, 2, True, False, 0, 0),
     (64, 2, 2, 2, 0, False, 64, 2, 2)),  # resnet fwd 16 64 32 128 3 2
    ((16384, 64, 1152, 1, True, False, 2, 1),
     (64, 1, 2, 3, 2, False, 256, 1, 2)),  # resnet dx 16 64 32 128 3 2
    ((4096, 128, 1152, 1, True, False, 0, 0),
     (64, 1, 2, 2, 0, False, 64, 2, 4)),  # resnet fwd 16 128 16 128 3 1
    ((4096, 128, 1152, 1, True, False, 1, 1),
     (64, 1, 2, 3, 1, False, 64, 2, 4)),  # resnet dx 16 128 16 128 3 1
    ((1024, 256, 1152, 2, True, False, 0, 0),
     (64, 2, 2, 2, 0, False, 16, 4, 4)),  # resnet fwd 16 128 16 256 3 2
    ((4096, 128, 2304, 1, True, False, 2, 1),
     (64, 1, 2, 3, 2, False, 64, 2, 4)),  # resnet dx 16 128 16 256 3 2
    ((1024, 256, 2304, 1, True, False, 0, 0),
     (64, 1, 2, 2, 0, False, 16, 4, 8)),  # resnet fwd 16 256 8 256 3 1
    ((1024, 256, 2304, 1, True, False, 1, 1),
     (64, 1, 2, 3, 1, False, 16, 4, 8)),  # resnet dx 16 256 8 256 3 1
    ((256, 512, 2304, 2, True, False, 0, 0),
     (64, 2, 2, 2, 0, False, 4, 8, 8)),  # resnet fwd 16 256 8 512 3 2
    ((1024, 256, 4608, 1, True, False, 0, 1),
     (64, 1, 2, 2, 0, False, 16, 4, 8)),  # resnet dx 16 256 8 512 3 2
    ((256, 512, 4608, 1, True, False, 0, 0),
     (64, 1, 2, 2, 0, False, 4, 8, 8)),  # resnet fwd 16 512 4 512 3 1
    ((256, 512, 4608, 1, True, False, 1, 1),
     (64, 1, 2, 3, 1, False, 4, 8, 8)),  # resnet dx 16 512 4 512 3 1
    ((4096, 128, 64, 2, True, False, 0, 0),
     (64, 2, 0, 2, 0, False, 64, 2, 1)),  # resnet fwd 16 64 32 128 1 2
    ((4096, 64, 128, 1, True, False, 0, 1),
     (64, 1, 0, 2, 0, False, 64, 1, 1)),  # resnet dx 16 64 32 128 1 2
    ((16384, 128, 576, 2, True, False, 0, 0),
     (64, 2, 0, 2, 0, False, 256, 2, 1)),  # resnet fwd 64 64 32 128 3 2
    ((65536, 64, 1152, 1, True, False, 2, 1),
     (128, 1, 0, 2, 2, False, 512, 1, 1)),  # resnet dx 64 64 32 128 3 2
    ((4096, 256, 1152, 2, True, False, 0, 0),
     (64, 2, 2, 2, 0, False, 64, 4, 2)),  # resnet fwd 64 128 16 256 3 2
    ((16384, 128, 2304, 1, True, False, 2, 1),
     (128, 1, 2, 3, 2, False, 128, 2, 2)),  # resnet dx 64 128 16 256 3 2
    ((1024, 256, 128, 2, True, False, 0, 0),
     (64, 2, 0, 2, 0, False, 16, 4, 1)),  # resnet fwd 16 128 16 256 1 2
    ((1024, 128, 256, 1, True, False, 0, 1),
     (64, 1, 0, 2, 0, False, 16, 2, 1)),  # resnet dx 16 128 16 256 1 2
    ((256, 512, 256, 2, True, False, 0, 0),
     (64, 2, 0, 2, 0, False, 4, 8, 1)),  # resnet fwd 16 256 8 512 1 2
    ((256, 256, 512, 1, True, False, 0, 1),
     (64, 1, 2, 2, 0, False, 4, 4, 2)),  # resnet dx 16 256 8 512 1 2
    ((2048, 512, 4608, 1, True, False, 0, 0),
     (64, 1, 2, 2, 0, False, 32, 8, 2)),  # resnet fwd 128 512 4 512 3 1
    ((2048, 512, 4608, 1, True, False, 1, 1),
     (64, 1, 2, 3, 1, False, 32, 8, 2)),  # resnet dx 128 512 4 512 3 1
    ((2048, 512, 2304, 2, True, False, 0, 0),
     (64, 2, 2, 2, 0, False, 32, 8, 2)),  # resnet fwd 128 256 8 512 3 2
    ((8192, 256, 4608, 1, True, False, 0, 1),
     (128, 1, 2, 2, 0, False, 64, 4, 2)),  # resnet dx 128 256 8 512 3 2
    ((8192, 512, 64, 1, True, False, 0, 0),
     (128, 1, 0, 2, 0, False, 64, 8, 1)),  # resnet fwd 8 64 32 512 1 1
    ((8192, 64, 512, 1, True, False, 1, 1),
     (64, 1, 2, 3, 1, False, 128, 1, 2)),  # resnet dx 8 64 32 512 1 1
    ((8192, 512, 64, 2, True, False, 0, 0),
     (128, 2, 0, 2, 0, False, 64, 8, 1)),  # resnet fwd 8 64 64 512 1 2
    ((8192, 64, 512, 1, True, False, 0, 1),
     (64, 1, 2, 2, 0, False, 128, 1, 2)),  # resnet dx 8 64 64 512 1 2
    ((8192, 64, 4608, 1, True, False, 0, 0),
     (64, 1, 2, 2, 0, False, 128, 1, 4)),  # resnet fwd 8 512 32 64 3 1
    ((8192, 512, 576, 1, True, False, 1, 1),
     (128, 1, 0, 2, 1, False, 64, 8, 1)),  # resnet dx 8 512 32 64 3 1
    ((16384, 128, 1152, 1, True, False, 0, 0),
     (64, 1, 0, 2, 0, False, 256, 2, 1)),  # resnet fwd 64 128 16 128 3 1
    ((16384, 128, 1152, 1, True, False, 1, 1),
     (128, 1, 2, 3, 1, False, 128, 2, 2)),  # resnet dx 64 128 16 128 3 1
    ((256, 64, 64, 1, True, False, 0, 0),
     (64, 1, 0, 2, 0, False, 4, 1, 1)),  # resnet fwd 4 64 8 64 1 1
    ((256, 64, 64, 1, True, False, 1, 1),
     (64, 1, 0, 2, 1, False, 4, 1, 1)),  # resnet dx 4 64 8 64 1 1
    ((256, 64, 64, 2, True, False, 0, 0),
     (64, 2, 0, 2, 0, False, 4, 1, 1)),  # resnet fwd 4 64 16 64 1 2
    ((256, 64, 64, 1, True, False, 0, 1),
     (64, 1, 0, 2, 0, False, 4, 1, 1)),  # resnet dx 4 64 16 64 1 2
    ((4096, 64, 128, 2, False, False, 0, 0),
     (64, 2, 0, 2, 0, False, 64, 1, 1)),  # gen fwd 3 12 32 4 2 1 1
    ((16384, 64, 1024, 1, False, False, 2, 1),
     (64, 1, 0, 2, 2, False, 256, 1, 1)),  # gen dx 3 12 32 4 2 1 1
    ((1024, 64, 256, 2, False, False, 0, 0),
     (64, 2, 0, 2, 0, False, 16, 1, 1)),  # gen fwd 12 24 16 4 2 1 1
    ((4096, 64, 1024, 1, False, False, 2, 1),
     (64, 1, 0, 2, 2, False, 64, 1, 1)),  # gen dx 12 24 16 4 2 1 1
    ((256, 64, 384, 2, False, False, 0, 0),
     (64, 2, 0, 2, 0, False, 4, 1, 1)),  # gen fwd 24 48 8 4 2 1 1
    ((1024, 64, 1024, 1, False, False, 0, 1),
     (64, 1, 0, 2, 0, False, 16, 1, 1)),  # gen dx 24 48 8 4 2 1 1
    ((64, 128, 768, 2, False, False, 0, 0),
     (64, 2, 0, 2, 0, False, 1, 2, 1)),  # gen fwd 48 96 4 4 2 1 1
    ((256, 64, 2048, 1, False, False, 0, 1),
     (64, 1, 0, 2, 0, False, 4, 1, 1)),  # gen dx 48 96 4 4 2 1 1
    ((4096, 64, 128, 2, False, False, 0, 0),
     (64, 2, 0, 2, 0, False, 64, 1, 1)),  # gen fwd 8 8 32 4 2 3 2
    ((16384, 64, 1024, 1, False, False, 2, 1),
     (64, 1, 0, 2, 2, False, 256, 1, 1)),  # gen dx 8 8 32 4 2 3 2
    ((4096, 64, 128, 2, False, False, 0, 0),
     (64, 2, 0, 2, 0, False, 64, 1, 1)),  # gen fwd 8 8 32 4 2 6 4
    ((16384, 64, 1024, 1, False, False, 2, 1),
     (64, 1, 0, 2, 2, False, 256, 1, 1)),  # gen dx 8 8 32 4 2 6 4
    ((4096, 64, 128, 2, False, False, 0, 0),
     (64, 2, 0, 2, 0, False, 64, 1, 1)),  # gen fwd 8 8 32 4 2 24 16
    ((16384, 64, 1024, 1, False, False, 2, 1),
     (64, 1, 0, 2, 2, False, 256, 1, 1)),  # gen dx 8 8 32 4 2 24 16
    ((1024, 256, 640, 2, True, False, 0, 0),
     (64, 2, 2, 2, 0, False, 16, 4, 2)),  # gen fwd 40 256 16 4 2 1 1
    ((4096, 64, 4096, 1, False, False, 2, 1),
     (64, 1, 0, 2, 2, False, 64, 1, 1)),  # gen dx 40 256 16 4 2 1 1
    ((784, 256, 1024, 1, True, False, 0, 0),
     (64, 1, 2, 2, 0, False, 13, 4, 4)),  # gen fwd 256 256 6 2 1 1 1
    ((576, 256, 1024, 1, True, False, 1, 1),
     (64, 1, 2, 3, 1, False, 9, 4, 4)),  # gen dx 256 256 6 2 1 1 1
    ((256, 256, 1024, 1, True, False, 0, 0),
     (64, 1, 2, 2, 0, False, 4, 4, 4)),  # gen fwd 1024 256 4 1 1 0 1
    ((256, 1024, 256, 1, True, False, 1, 1),
     (64, 1, 0, 2, 1, False, 4, 16, 1)),  # gen dx 1024 256 4 1 1 0 1
    ((162, 128, 576, 1, True, True, 0, 0),
     (64, 1, 1, 3, 0, False, 3, 2, 1)),  # bn stats (2, 64, 11, 11) 128 3 1
    ((162, 128, 576, 1, True, False, 0, 0),
     (64, 1, 2, 2, 0, False, 3, 2, 2)),  # bn plain (2, 64, 11, 11) 128 3 1
    ((162, 64, 576, 2, True, True, 0, 0),
     (64, 2, 1, 3, 0, False, 3, 1, 1)),  # bn stats (2, 64, 19, 19) 64 3 2
    ((162, 64, 576, 2, True, False, 0, 0),
     (64, 2, 2, 2, 0, False, 3, 1, 2)),  # bn plain (2, 64, 19, 19) 64 3 2
    ((75, 64, 64, 2, True, True, 0, 0),
     (64, 2, 1, 3, 0, False, 2, 1, 1)),  # bn stats (3, 64, 9, 9) 64 1 2
    ((75, 64, 64, 2, True, False, 0, 0),
     (64, 2, 0, 2, 0, False, 2, 1, 1)),  # bn plain (3, 64, 9, 9) 64 1 2
    ((4356, 512, 72, 1, True, True, 0, 0),
     (64, 1, 1, 3, 0, False, 69, 8, 1)),  # bn stats (4, 8, 35, 35) 512 3 1
    ((4356, 512, 72, 1, True, False, 0, 0),
     (64, 1, 0, 2, 0, False, 69, 8, 1)),  # bn plain (4, 8, 35, 35) 512 3 1
    ((32768, 64, 576, 1, True, True, 0, 0),
     (64, 1, 1, 3, 0, False, 512, 1, 1)),  # bn stats (32, 64, 34, 34) 64 3 1
    ((32768, 64, 576, 1, True, False, 0, 0),
     (64, 1, 0, 2, 0, False, 512, 1, 1)),  # bn plain (32, 64, 34, 34) 64 3 1
    ((8712, 512, 72, 1, True, True, 0, 0),
     (128, 1, 1, 3, 0, False, 69, 8, 1)),  # bn stats (8, 8, 35, 35) 512 3 1
    ((8712, 512, 72, 1, True, False, 0, 0),
     (128, 1, 0, 2, 0, False, 69, 8, 1)),  # bn plain (8, 8, 35, 35) 512 3 1
    ((8712, 512, 72, 2, True, True, 0, 0),
     (128, 2, 1, 3, 0, False, 69, 8, 1)),  # bn stats (8, 8, 67, 67) 512 3 2
    ((8712, 512, 72, 2, True, False, 0, 0),
     (128, 2, 0, 2, 0, False, 69, 8, 1)),  # bn plain (8, 8, 67, 67) 512 3 2
    ((2304, 64, 640, 2, False, False, 0, 2),
     (64, 2, 0, 3, 0, True, 36, 1, 1)),  # bank fwd 9 8 32 4 2 8 (1, 2, 4, 8, 16) (1, 3, 6, 12, 24)
    ((200, 64, 256, 1, False, False, 0, 2),
     (64, 1, 0, 3, 0, True, 4, 1, 1)),  # bank fwd 2 8 9 4 1 16 (1, 3) (2, 5)
    ((33792, 64, 256, 2, False, False, 0, 2),
     (128, 2, 0, 3, 0, True, 264, 1, 1)),  # bank fwd 33 8 64 4 2 8 (1, 2) (1, 3)
    ((33792, 64, 256, 1, False, False, 0, 2),
     (128, 1, 0, 3, 0, True, 264, 1, 1)),  # bank fwd 33 8 31 4 1 16 (1, 3) (2, 5)
]

BENCH_CONV = [
    ((131072, 64, 576, 1, True, False, 0, 0),
     (128, 1, 0, 2, 0, False, 1024, 1, 1)),  # bench fwd 64 32 64 3 1
    ((131072, 64, 576, 1, True, False, 1, 1),
     (128, 1, 0, 2, 1, False, 1024, 1, 1)),  # bench dx 64 32 64 3 1
    ((32768, 128, 576, 2, True, False, 0, 0),
     (128, 2, 0, 2, 0, False, 256, 2, 1)),  # bench fwd 64 32 128 3 2
    ((131072, 64, 1152, 1, True, False, 2, 1),
     (128, 1, 0, 2, 2, False, 1024, 1, 1)),  # bench dx 64 32 128 3 2
    ((32768, 128, 1152, 1, True, False, 0, 0),
     (128, 1, 0, 2, 0, False, 256, 2, 1)),  # bench fwd 128 16 128 3 1
    ((32768, 128, 1152, 1, True, False, 1, 1),
     (128, 1, 0, 2, 1, False, 256, 2, 1)),  # bench dx 128 16 128 3 1
    ((32768, 128, 64, 2, True, False, 0, 0),
     (128, 2, 0, 2, 0, False, 256, 2, 1)),  # bench fwd 64 32 128 1 2
    ((32768, 64, 128, 1, True, False, 0, 1),
     (128, 1, 0, 2, 0, False, 256, 1, 1)),  # bench dx 64 32 128 1 2
    ((8192, 256, 1152, 2, True, False, 0, 0),
     (64, 2, 0, 2, 0, False, 128, 4, 1)),  # bench fwd 128 16 256 3 2
    ((32768, 128, 2304, 1, True, False, 2, 1),
     (128, 1, 0, 2, 2, False, 256, 2, 1)),  # bench dx 128 16 256 3 2
    ((8192, 256, 2304, 1, True, False, 0, 0),
     (64, 1, 0, 2, 0, False, 128, 4, 1)),  # bench fwd 256 8 256 3 1
    ((8192, 256, 2304, 1, True, False, 1, 1),
     (128, 1, 2, 3, 1, False, 64, 4, 2)),  # bench dx 256 8 256 3 1
    ((8192, 256, 128, 2, True, False, 0, 0),
     (64, 2, 0, 2, 0, False, 128, 4, 1)),  # bench fwd 128 16 256 1 2
    ((8192, 128, 256, 1, True, False, 0, 1),
     (64, 1, 0, 2, 0, False, 128, 2, 1)),  # bench dx 128 16 256 1 2
    ((2048, 512, 2304, 2, True, False, 0, 0),
     (64, 2, 2, 2, 0, False, 32, 8, 2)),  # bench fwd 256 8 512 3 2
    ((8192, 256, 4608, 1, True, False, 0, 1),
     (128, 1, 2, 2, 0, False, 64, 4, 2)),  # bench dx 256 8 512 3 2
    ((2048, 512, 4608, 1, True, False, 0, 0),
     (64, 1, 2, 2, 0, False, 32, 8, 2)),  # bench fwd 512 4 512 3 1
    ((2048, 512, 4608, 1, True, False, 1, 1),
     (64, 1, 2, 3, 1, False, 32, 8, 2)),  # bench dx 512 4 512 3 1
    ((2048, 512, 256, 2, True, False, 0, 0),
     (64, 2, 0, 2, 0, False, 32, 8, 1)),  # bench fwd 256 8 512 1 2
    ((2048, 256, 512, 1, True, False, 0, 1),
     (64, 1, 2, 2, 0, False, 32, 4, 2)),  # bench dx 256 8 512 1 2
]

MENU_DW = [
    ((16, 64, 34, 34, 64, 32, 32, 3, 3, 1, 1),
     (True, 64, 2, 1, 5, 1, 128, 2, True, 0)),  # resnet dw 16 64 32 64 3 1
    ((16, 64, 34, 34, 128, 16, 16, 3, 3, 2, 1),
     (False, 0, 0, 2, 0, 0, 0, 0, False, 2)),  # resnet dw 16 64 32 128 3 2
    ((16, 128, 18, 18, 128, 16, 16, 3, 3, 1, 1),
     (True, 128, 1, 1, 18, 1, 32, 2, True, 0)),  # resnet dw 16 128 16 128 3 1
    ((16, 128, 18, 18, 256, 8, 8, 3, 3, 2, 1),
     (False, 0, 0, 2, 0, 0, 0, 0, False, 1)),  # resnet dw 16 128 16 256 3 2
    ((16, 256, 10, 10, 256, 8, 8, 3, 3, 1, 1),
     (True, 128, 1, 1, 36, 2, 8, 2, False, 0)),  # resnet dw 16 256 8 256 3 1
    ((16, 256, 10, 10, 512, 4, 4, 3, 3, 2, 1),
     (False, 0, 0, 2, 0, 0, 0, 0, False, 1)),  # resnet dw 16 256 8 512 3 2
    ((16, 512, 6, 6, 512, 4, 4, 3, 3, 1, 1),
     (False, 0, 0, 1, 0, 0, 0, 0, False, 1)),  # resnet dw 16 512 4 512 3 1
    ((16, 64, 32, 32, 128, 16, 16, 1, 1, 2, 1),
     (True, 128, 1, 2, 1, 1, 64, 1, True, 0)),  # resnet dw 16 64 32 128 1 2
    ((64, 64, 34, 34, 128, 16, 16, 3, 3, 2, 1),
     (True, 128, 1, 2, 9, 1, 64, 4, True, 0)),  # resnet dw 64 64 32 128 3 2
    ((64, 128, 18, 18, 256, 8, 8, 3, 3, 2, 1),
     (True, 128, 1, 2, 18, 2, 16, 4, True, 0)),  # resnet dw 64 128 16 256 3 2
    ((16, 128, 16, 16, 256, 8, 8, 1, 1, 2, 1),
     (True, 128, 1, 2, 2, 2, 16, 1, True, 0)),  # resnet dw 16 128 16 256 1 2
    ((16, 256, 8, 8, 512, 4, 4, 1, 1, 2, 1),
     (False, 0, 0, 2, 0, 0, 0, 0, False, 1)),  # resnet dw 16 256 8 512 1 2
    ((128, 512, 6, 6, 512, 4, 4, 3, 3, 1, 1),
     (False, 0, 0, 1, 0, 0, 0, 0, False, 1)),  # resnet dw 128 512 4 512 3 1
    ((128, 256, 10, 10, 512, 4, 4, 3, 3, 2, 1),
     (False, 0, 0, 2, 0, 0, 0, 0, False, 1)),  # resnet dw 128 256 8 512 3 2
    ((8, 64, 32, 32, 512, 32, 32, 1, 1, 1, 1),
     (True, 128, 1, 1, 1, 4, 64, 2, True, 0)),  # resnet dw 8 64 32 512 1 1
    ((8, 64, 64, 64, 512, 32, 32, 1, 1, 2, 1),
     (True, 128, 1, 2, 1, 4, 64, 2, True, 0)),  # resnet dw 8 64 64 512 1 2
    ((8, 512, 34, 34, 64, 32, 32, 3, 3, 1, 1),
     (False, 0, 0, 1, 0, 0, 0, 0, False, 4)),  # resnet dw 8 512 32 64 3 1
    ((64, 128, 18, 18, 128, 16, 16, 3, 3, 1, 1),
     (True, 128, 1, 1, 18, 1, 32, 8, True, 0)),  # resnet dw 64 128 16 128 3 1
    ((4, 64, 8, 8, 64, 8, 8, 1, 1, 1, 1),
     (True, 64, 1, 1, 1, 1, 4, 1, False, 0)),  # resnet dw 4 64 8 64 1 1
    ((4, 64, 16, 16, 64, 8, 8, 1, 1, 2, 1),
     (True, 64, 1, 2, 1, 1, 4, 1, False, 0)),  # resnet dw 4 64 16 64 1 2
    ((16, 8, 34, 34, 64, 16, 16, 4, 4, 2, 1),
     (False, 0, 0, 2, 0, 0, 0, 0, False, 2)),  # gen dw 3 12 32 4 2 1 1
    ((16, 16, 18, 18, 64, 8, 8, 4, 4, 2, 1),
     (False, 0, 0, 2, 0, 0, 0, 0, False, 1)),  # gen dw 12 24 16 4 2 1 1
    ((16, 24, 10, 10, 64, 4, 4, 4, 4, 2, 1),
     (False, 0, 0, 2, 0, 0, 0, 0, False, 1)),  # gen dw 24 48 8 4 2 1 1
    ((16, 48, 6, 6, 128, 2, 2, 4, 4, 2, 1),
     (False, 0, 0, 2, 0, 0, 0, 0, False, 1)),  # gen dw 48 96 4 4 2 1 1
    ((16, 8, 38, 38, 64, 16, 16, 4, 4, 2, 2),
     (False, 0, 0, 2, 0, 0, 0, 0, False, 2)),  # gen dw 8 8 32 4 2 3 2
    ((16, 8, 44, 44, 64, 16, 16, 4, 4, 2, 4),
     (False, 0, 0, 2, 0, 0, 0, 0, False, 2)),  # gen dw 8 8 32 4 2 6 4
    ((16, 8, 80, 80, 64, 16, 16, 4, 4, 2, 16),
     (False, 0, 0, 2, 0, 0, 0, 0, False, 2)),  # gen dw 8 8 32 4 2 24 16
    ((16, 40, 18, 18, 256, 8, 8, 4, 4, 2, 1),
     (False, 0, 0, 2, 0, 0, 0, 0, False, 1)),  # gen dw 40 256 16 4 2 1 1
    ((16, 256, 8, 8, 256, 7, 7, 2, 2, 1, 1),
     (False, 0, 0, 1, 0, 0, 0, 0, False, 1)),  # gen dw 256 256 6 2 1 1 1
    ((16, 1024, 4, 4, 256, 4, 4, 1, 1, 1, 1),
     (False, 0, 0, 1, 0, 0, 0, 0, False, 1)),  # gen dw 1024 256 4 1 1 0 1
]

BENCH_DW = [
    ((128, 64, 34, 34, 64, 32, 32, 3, 3, 1, 1),
     (True, 64, 2, 1, 5, 1, 128, 16, True, 0)),  # bench dw 64 32 64 3 1
    ((128, 64, 34, 34, 128, 16, 16, 3, 3, 2, 1),
     (True, 128, 1, 2, 9, 1, 64, 8, True, 0)),  # bench dw 64 32 128 3 2
    ((128, 128, 18, 18, 128, 16, 16, 3, 3, 1, 1),
     (True, 128, 1, 1, 18, 1, 32, 16, True, 0)),  # bench dw 128 16 128 3 1
    ((128, 64, 32, 32, 128, 16, 16, 1, 1, 2, 1),
     (True, 128, 1, 2, 1, 1, 64, 8, True, 0)),  # bench dw 64 32 128 1 2
    ((128, 128, 18, 18, 256, 8, 8, 3, 3, 2, 1),
     (True, 128, 1, 2, 18, 2, 16, 8, True, 0)),  # bench dw 128 16 256 3 2
    ((128, 256, 10, 10, 256, 8, 8, 3, 3, 1, 1),
     (True, 128, 1, 1, 36, 2, 8, 16, False, 0)),  # bench dw 256 8 256 3 1
    ((128, 128, 16, 16, 256, 8, 8, 1, 1, 2, 1),
     (True, 128, 1, 2, 2, 2, 64, 2, True, 0)),  # bench dw 128 16 256 1 2
    ((128, 256, 10, 10, 512, 4, 4, 3, 3, 2, 1),
     (False, 0, 0, 2, 0, 0, 0, 0, False, 1)),  # bench dw 256 8 512 3 2
    ((128, 512, 6, 6, 512, 4, 4, 3, 3, 1, 1),
     (False, 0, 0, 1, 0, 0, 0, 0, False, 1)),  # bench dw 512 4 512 3 1
    ((128, 256, 8, 8, 512, 4, 4, 1, 1, 2, 1),
     (False, 0, 0, 2, 0, 0, 0, 0, False, 1)),  # bench dw 256 8 512 1 2
    ((128, 3, 34, 34, 64, 32, 32, 3, 3, 1, 1),
     (False, 0, 0, 1, 0, 0, 0, 0, False, 64)),  # bench dw 3 32 64 3 1
]

