// Launch planning for the MFMA conv kernels (conv2d_mfma.hip): the only copy
// of every tile / split / variant rule, as plain integer arithmetic.  No ATen
// and no HIP in here, so the rules are bound to Python and tested without a
// GPU (tests/test_conv_plan.py).  The host wrappers turn a plan into a launch
// through one table per kernel family; a plan without a table entry is an
// error, never a silent default.
#pragma once

namespace fedkit_plan {

constexpr int kBN = 64;   // out-channel tile
constexpr int kBK = 64;   // reduction tile

// Who launches the conv.  The caller decides where the 64-row tile takes over
// from the 128-row one, in workgroups of the 128-row grid:
//   kFwd   < 512: forward shapes measured BM64 faster below 512 workgroups
//                 (C128-s2 fwd 20.5 -> 15.2 us);
//   kBwd   < 256: BOTH bwd-data forms regressed under the forward rule (vpad
//                 layer3 dx 32.4 -> 49.8 us, materialized s2-C256 52.4 ->
//                 64.0), so they switch only when the 128-row grid cannot
//                 fill the 256 CUs;
//   kBank  < 256, never splits, always the 3-stage pipeline.
enum ConvCaller { kFwd = 0, kBwd = 1, kBank = 2 };

struct ConvPlan {
  int BM;          // 64 | 128 rows of M per workgroup
  int stride;      // kernel STRIDE (1 | 2)
  int mode;        // 0 plain store, 1 + BN partials, 2 split-K fp32 partials
  int stages;      // LDS pipeline depth (2 | 3)
  int vpad;        // 0 materialized input, 1 | 2 virtual pad (source stride)
  bool multitap;   // dilated bank
  int grid_x;      // ceil(M / BM)
  int grid_y;      // Kout / 64
  int splits;      // grid.z (1 unless mode 2)
};

// M = N*P*Q, Kout % 64 == 0, Kg = R*S*C.  dense: every out channel is stored
// (Ktrue == Kout).  bnpart: the BN-statistics epilogue is wanted; its slab is
// [grid_y][grid_x][2][64] floats.
inline ConvPlan plan_conv(long long M, int Kout, int Kg, int stride,
                          bool dense, bool bnpart, int vpad,
                          ConvCaller caller) {
  ConvPlan p{};
  p.stride = stride;
  p.vpad = vpad;
  p.multitap = caller == kBank;
  p.grid_y = Kout / kBN;
  const long long wg128 = ((M + 127) / 128) * p.grid_y;
  p.BM = wg128 < (caller == kFwd ? 512 : 256) ? 64 : 128;
  p.grid_x = (int)((M + p.BM - 1) / p.BM);
  // split-K when the (M, Kout) grid alone cannot fill the 256 CUs and the
  // Kg loop is deep enough to slice (layer4-class shapes)
  p.splits = 1;
  const int gridxy = p.grid_x * p.grid_y;
  const int nkt = (Kg + kBK - 1) / kBK;
  if (caller != kBank && !bnpart && dense && gridxy <= 256)
    while (p.splits < 8 && gridxy * p.splits < 512 &&
           nkt / (p.splits * 2) >= 4)
      p.splits *= 2;
  p.mode = p.splits > 1 ? 2 : bnpart ? 1 : 0;
  // 2 stages (48 KB LDS at BM=128 -> 3 wg/CU) measured faster or tied on
  // every plain MODE-0 / split-K shape (layer1 25.2 -> 22.6 us): the extra
  // resident waves hide more latency than the deeper pipeline.  The BN
  // epilogue, virtual-pad split-K and the bank keep the 3-stage pipeline.
  p.stages = (p.multitap || p.mode == 1 || (vpad && p.mode == 2)) ? 3 : 2;
  return p;
}

// bwd-weight.  fast: the transpose-then-implicit-GEMM MFMA path
// (dw_gemm_kernel); otherwise im2col + a library GEMM whose reduction dim is
// cut into `chunks` batches.
struct DwPlan {
  bool fast;
  int BMK;               // kout tile (128 ~1.7x faster than 64)
  int NT;                // rsc tile = 64 * NT
  int stride;            // kernel STRIDE (1 | 2)
  int rsc_tiles;         // grid.x
  int grid_y;            // K / BMK
  int splits;            // grid.z: independent fp32 partial slabs over m
  int mtiles_per_split;
  bool two_stage;        // column sum through an [8][L] slab first
  int chunks;            // library path only
};

// gy [N][K][P][Q], padded input [N][C][Hp][Wp], filter R x S.
inline DwPlan plan_dw(int N, int C, int Hp, int Wp, int K, int P, int Q,
                      int R, int S, int stride, int dil) {
  DwPlan d{};
  const long long M = (long long)N * P * Q;
  const long long RSC = (long long)R * S * C;
  const long long NHW = (long long)N * Hp * Wp;
  // an 8-m chunk must stay inside one q row (Q % 8 == 0; Q == 4 was measured
  // slower than the library path twice) and m must split by shifts
  const bool pow2 = P > 0 && Q > 0 && (P & (P - 1)) == 0 && (Q & (Q - 1)) == 0;
  const bool common = dil == 1 && pow2 && Q % 8 == 0 && K % 64 == 0 &&
      RSC % 64 == 0 && C % 64 == 0 && M % 64 == 0;
  // stride 1 reads one transposed plane, stride 2 even/odd-column planes
  d.fast = (stride == 1 && common && NHW % 64 == 0) ||
      (stride == 2 && common && Wp % 2 == 0 && (NHW / 2) % 64 == 0);
  d.stride = stride;
  if (d.fast) {
    d.BMK = K % 128 == 0 ? 128 : 64;
    // K = 64 caps the kout tile; widen the rsc tile instead
    const bool nt2 = d.BMK == 64 && stride == 1 && RSC >= 128;
    d.NT = nt2 ? 2 : 1;
    d.rsc_tiles = nt2 ? (int)((RSC + 127) / 128) : (int)(RSC / 64);
    d.grid_y = K / d.BMK;
    const long long mtiles = M / 64;
    const long long tiles_xy = (long long)d.rsc_tiles * d.grid_y;
    const int maxsplit = nt2 ? 128 : 64;
    d.splits = 1;
    while (d.splits < maxsplit && tiles_xy * d.splits < 512 &&
           (long long)d.splits * 2 <= mtiles)
      d.splits *= 2;
    d.mtiles_per_split = (int)((mtiles + d.splits - 1) / d.splits);
    d.two_stage = d.splits > 8;
    return d;
  }
  // Tensile picks no split-K for the tall-skinny dy^T @ col GEMM: batch the
  // reduction dim into chunks of >= 2048 rows
  d.chunks = 1;
  while (d.chunks < 64 && (M / (d.chunks * 2)) >= 2048 &&
         M % (d.chunks * 2) == 0)
    d.chunks *= 2;
  return d;
}

// Every kernel a plan can select, and nothing else.  The dispatch tables and
// the variant lists bound to Python both expand these.
//   X(BM, STRIDE, MODE, STAGES, MT, VPAD)
#define FEDKIT_CONV_VARIANTS(X)                                         \
  X(64, 1, 0, 2, false, 0) X(128, 1, 0, 2, false, 0)   /* plain */      \
  X(64, 2, 0, 2, false, 0) X(128, 2, 0, 2, false, 0)                    \
  X(64, 1, 2, 2, false, 0) X(128, 1, 2, 2, false, 0)   /* split-K */    \
  X(64, 2, 2, 2, false, 0)                                              \
  X(64, 1, 1, 3, false, 0) X(128, 1, 1, 3, false, 0)   /* BN stats */   \
  X(64, 2, 1, 3, false, 0) X(128, 2, 1, 3, false, 0)                    \
  X(64, 1, 0, 2, false, 1) X(128, 1, 0, 2, false, 1)   /* vpad */       \
  X(64, 1, 0, 2, false, 2) X(128, 1, 0, 2, false, 2)                    \
  X(64, 1, 2, 3, false, 1) X(128, 1, 2, 3, false, 1)                    \
  X(64, 1, 2, 3, false, 2) X(128, 1, 2, 3, false, 2)                    \
  X(64, 1, 0, 3, true, 0) X(128, 1, 0, 3, true, 0)     /* bank */       \
  X(64, 2, 0, 3, true, 0) X(128, 2, 0, 3, true, 0)
//   X(BMK, STRIDE, NT)
#define FEDKIT_DW_VARIANTS(X) \
  X(128, 1, 1) X(128, 2, 1) X(64, 1, 1) X(64, 2, 1) X(64, 1, 2)

}  // namespace fedkit_plan
