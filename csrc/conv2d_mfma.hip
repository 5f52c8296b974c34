// NHWC implicit-GEMM convolution on MFMA matrix cores (gfx950 / CDNA4).
// The single hottest kernel family of the framework (SURVEY.md §2a rows 1-2:
// all ResNet conv3x3 s1/s2 and 1x1 shortcut convs, fwd + bwd-data).
//
// GEMM view:  y[M=N*P*Q, Kout] = A[M, Kg=R*S*C] * B[Kg, Kout]
//   A(m, k)   = xpad[n, p*stride + r, q*stride + s, c]   (im2col, implicit;
//               input is PRE-PADDED so there are no boundary branches and
//               global_load_lds (direct HBM->LDS DMA, 16 B/lane) can stage A)
//   B(k, kout)= w[kout, r, s, c]  — [Kout][R*S*C] rows are k-contiguous, so
//               B stages as a plain 2D tile copy.
//
// Structure (guide §5 anatomy, 2-phase double-buffered):
//   tile BM x BN=64 x BK=64, 256 threads = 4 waves (2x2), wave tile
//   (BM/2) x 32, mfma_f32_16x16x32_bf16 accumulating fp32;
//   LDS: double-buffered A[BM][64] + B[64][64] bf16 in ONE __shared__ block;
//   XOR swizzle on the 16-B k-chunk (chunk ^= row & 7) applied on the glds
//   SOURCE address and the ds_read address (guide T2 / rule 21) to kill the
//   16-way ds_read_b128 bank conflict of 128-B rows;
//   K-loop: STAGE(next) || ds_read+MFMA(cur) || vmcnt(0)+barrier.
//
// bwd-data reuses this kernel: dx = conv_s1(dilate_pad(dy), rot180(w)^T)
// (host-side transform kernels below).  bwd-weight transposes both operands
// once and runs an implicit-GEMM MFMA kernel (dw_gemm_kernel); shapes it
// does not cover take im2col + a library GEMM.
//
// Every tile / split / variant choice is made by conv_plan.h (plain
// integers, tested without a GPU); the host wrappers here only turn a plan
// into a launch through one table per kernel family.
//
// Constraints (host-checked): C % 8 == 0, Kout % 64 == 0, bf16 tensors (a
// Kg = R*S*C tail tile is zero-filled).  conv1 of ResNet (C=3) uses the
// dedicated direct kernel in conv_small.hip.

#include "fedkit_common.h"
#include "conv_plan.h"

namespace {

using namespace fedkit_plan;

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __hip_bfloat16 bf16;

#define GLDS16(gptr, lptr) \
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(gptr), \
                                   (__attribute__((address_space(3))) void*)(lptr), 16, 0, 0)

constexpr int BN = kBN;  // out-channel tile
constexpr int BK = kBK;  // im2col-k tile

// 16-B zero page for the Kg tail: when Kg % 64 != 0 (Net-family 5x5 and
// valid-3x3 shapes: Kg = 200 / 72 / 288) the last K-tile's out-of-range
// 8-element chunks DMA from here instead of reading past the filter row.
// Kg is always a multiple of 8 (C padded to x8), so chunks never straddle.
__device__ __bf16 g_kzero[8] = {};

// Multi-tap descriptor (CPC dilated bank, SURVEY §2a: "fuse dilation bank
// (5 convs, same input) into one multi-tap kernel").  The GEMM K dim is
// the concatenation of each tap's R*S*C block (kg_per each, % 64 == 0);
// the combined weight is block-diagonal over (tap out-channels, tap kg
// range), so one MFMA pass computes all taps' outputs.  off[t] is the
// origin shift (shared_pad - pad_t) into the once-padded input.
struct TapDesc {
  int n;        // taps
  int kg_per;   // R*S*C per tap (multiple of BK)
  int dil[8];
  int off[8];
};

// Virtual-pad descriptor (bwd-data fast path): instead of materializing
// dilate_pad(gy) — one extra kernel plus a full write+read of a y-sized
// buffer per conv, 7%+ of round-1 GPU time — the A stage reads gy
// DIRECTLY, bounds-checking each 16-B chunk (8 channels of ONE pixel,
// C % 64 == 0 on every bwd-data shape) and substituting the zero page
// outside.  The checks are per-SLOT scalars (4 per stage), not per-lane.
//   hs, ws: source (gy) spatial dims
//   pl:     top/left dilate-pad amount ((R-1)*dil - pad)
//   vstr:   zero-insertion stride (the forward conv's stride)
struct VPadDesc {
  int hs, ws, pl, vstr;
};

// LDS byte offset of element (row, k) of a [rows][64] bf16 tile with the
// chunk-XOR swizzle (16-B chunk index ^ (row & 7)).
__device__ __forceinline__ int lds_off(int row, int k) {
  int chunk = (k >> 3) ^ (row & 7);
  return row * 128 + chunk * 16 + (k & 7) * 2;
}

// (A register-staging variant was measured 2x SLOWER than glds staging
// and removed — see profiles/r01_kernel_stats_final.md dead ends.)
// MODE 0: plain store.  MODE 1 (BN stats): the epilogue also emits this
// workgroup's per-channel (sum, sumsq) partial row into aux
// ([Kout/64][mtiles][2][64] fp32, finalized by
// bn_conv_colsum_finalize_kernel).  MODE 2 (split-K): grid.z slices the
// Kg loop and the epilogue writes fp32 partials aux[z][M][Kout] —
// for shapes whose (M, Kout) grid alone cannot fill 256 CUs
// (layer4: 2048x512 -> 256 workgroups, measured 37 us at 12% MFMA).
// STAGES: 3 = double-lookahead pipeline (72 KB LDS at BM=128 -> 2 wg/CU);
// 2 = single-lookahead (48 KB -> 3 wg/CU: PMC shows 43% wave-wait at
// occupancy 2 with zero LDS conflicts, so more resident waves may hide
// more latency than the deeper pipeline) — picked per form by plan_conv.
// VPAD: 0 = pre-materialized input; 1 = virtual pad, stride-1 source
// (per-slot int compares, affine address); 2 = virtual pad over a
// stride-2 zero-inserted source (bwd-data of stride-2 convs): the A
// stage reads the RAW gy — besides killing the dilate_pad launch and
// buffer, it skips the 3/4-zeros A traffic the materialized dilated
// image pays.  Parity/bounds per slot via 2 precomputed parity bits and
// 4 stage-scalar class offsets (no 64-bit muls in the loop).
template <int BM, int STRIDE, int MODE, int STAGES, bool MT, int VPAD>
__global__ __launch_bounds__(256)
void conv_fwd_kernel(const bf16* __restrict__ xp,  // [N][Hp][Wp][C] padded
                     const bf16* __restrict__ w,   // [Kout][R*S*C]
                     bf16* __restrict__ y,         // [M][Ktrue]
                     int N, int Hp, int Wp, int C, int Kout,
                     int R, int S, int P, int Q, int Kg, int dil,
                     int Ktrue /* <= Kout: K rows beyond are zero-padding
                                  (VAE/CPC channel counts), skipped on
                                  store so y needs no unpad pass */,
                     float* __restrict__ aux, TapDesc td, VPadDesc vp) {
  constexpr int AB = BM * BK * 2;          // A tile bytes
  constexpr int BB = BN * BK * 2;          // B tile bytes
  __shared__ char smem[STAGES * (AB + BB)];

  const int tid = threadIdx.x;
  const int wave = tid >> 6;
  const int lane = tid & 63;
  const long long M = (long long)N * P * Q;

  // XCD-aware block swizzle (guide T1, bijective form): the dispatcher
  // places block b on XCD b%8; remap so each XCD owns a CONTIGUOUS chunk of
  // the (bm, bn) space and neighbor tiles share its private L2.
  int bm, bn;
  {
    const int nwg = gridDim.x * gridDim.y;
    const int orig = blockIdx.y * gridDim.x + blockIdx.x;
    const int q8 = nwg / 8, r8 = nwg % 8;
    const int xcd = orig % 8, idx = orig / 8;
    const int swz = (xcd < r8 ? xcd * (q8 + 1)
                              : r8 * (q8 + 1) + (xcd - r8) * q8) + idx;
    bm = swz % gridDim.x;                  // M tile
    bn = swz / gridDim.x;                  // Kout tile
  }

  // ---- staging geometry: each thread owns (BM*BK)/(256*8) A-slots and
  //      (BN*BK)/(256*8) B-slots of 8 bf16 (16 B) each, fixed across the
  //      K loop; only the (r,s,c) decomposition changes per K-tile.
  constexpr int A_SLOTS = (BM * BK) / (256 * 8);   // 4 (BM=128) or 2 (BM=64)
  constexpr int B_SLOTS = (BN * BK) / (256 * 8);   // 2

  // A slot d = pass*256 + tid -> LDS row = d/8, stored chunk = d%8,
  // source element (row, k8 = (d%8) ^ (row&7)).
  long long a_rowbase[A_SLOTS];   // &xp[n][p*STRIDE][q*STRIDE][0] offset
  int a_k8[A_SLOTS];
  int a_p[A_SLOTS], a_q[A_SLOTS];          // VPAD: virtual-coord row origin
#pragma unroll
  for (int i = 0; i < A_SLOTS; ++i) {
    int d = i * 256 + tid;
    int row = d >> 3;
    long long m = (long long)bm * BM + row;
    if (m >= M) m = M - 1;                 // clamp (store side is guarded)
    int q = (int)(m % Q);
    int p = (int)((m / Q) % P);
    int n = (int)(m / ((long long)P * Q));
    if (VPAD == 1) {
      // base points at gy pixel (p - pl, q - pl); the stage adds a
      // SCALAR tap offset and the per-slot work is just int compares
      // against stage-scalar bounds — no muls in the loop
      a_rowbase[i] =
          (((long long)n * vp.hs + (p - vp.pl)) * vp.ws + (q - vp.pl)) * C;
      a_p[i] = p - vp.pl;
      a_q[i] = q - vp.pl;
    } else if (VPAD == 2) {
      // virtual coords hv = (p - pl) + r*dil map to source row hv/2 when
      // hv is even; base uses the FLOOR halves, the stage adds a class
      // offset selected by this slot's parity bits (a_p/a_q carry the
      // full virtual origin for parity + bounds)
      int vpp = p - vp.pl, vqq = q - vp.pl;
      a_rowbase[i] =
          (((long long)n * vp.hs + (vpp >> 1)) * vp.ws + (vqq >> 1)) * C;
      a_p[i] = vpp;
      a_q[i] = vqq;
    } else {
      a_rowbase[i] = (((long long)n * Hp + p * STRIDE) * Wp + q * STRIDE) * C;
      a_p[i] = a_q[i] = 0;
    }
    a_k8[i] = (d & 7) ^ (row & 7);
  }
  long long b_rowbase[B_SLOTS];
  int b_k8[B_SLOTS];
#pragma unroll
  for (int i = 0; i < B_SLOTS; ++i) {
    int d = i * 256 + tid;
    int row = d >> 3;                      // out channel within tile
    b_rowbase[i] = ((long long)bn * BN + row) * Kg;
    b_k8[i] = (d & 7) ^ (row & 7);
  }

  auto bufA = [&](int b) -> char* { return smem + b * (AB + BB); };
  auto bufB = [&](int b) -> char* { return smem + b * (AB + BB) + AB; };

  const bool c64 = !MT && (C % 64) == 0;
  auto stage = [&](int buf, int kt) {
    // A tile: per-slot source (r,s,c) from k_global; 16-B LDS-DMA.
    // LDS dest for a glds is wave-uniform base + lane*16: slot d = pass*256
    // + wave*64 + lane matches d = pass*256 + tid exactly.
    // When C % 64 == 0 (every flagship shape) a whole 64-k tile lies in ONE
    // (r,s) filter tap, so the kg -> (r,s,c) split is SCALAR per stage —
    // the per-lane divisions by runtime C/S otherwise cost a magic-number
    // sequence per slot right in the hot loop.
    long long tap_off = 0;
    int c0 = 0;
    int vh = 0, vw = 0;                    // VPAD: tap offset (dil applied)
    // VPAD == 2 stage scalars: class tap offsets + bounds per parity bit
    int t00 = 0, t01 = 0, t10 = 0, t11 = 0;
    int rlo0 = 0, rhi0 = 0, rlo1 = 0, rhi1 = 0;
    int clo0 = 0, chi0 = 0, clo1 = 0, chi1 = 0;
    if (c64) {
      int rs = (kt * BK) / C;
      c0 = kt * BK - rs * C;
      int s = rs % S;
      int r = rs / S;
      if (VPAD == 1) {
        vh = r * dil;
        vw = s * dil;
        tap_off = ((long long)vh * vp.ws + vw) * C;
      } else if (VPAD == 2) {
        vh = r * dil;
        vw = s * dil;
        int rt0 = (vh + 0) >> 1, rt1 = (vh + 1) >> 1;
        int ct0 = (vw + 0) >> 1, ct1 = (vw + 1) >> 1;
        t00 = (rt0 * vp.ws + ct0) * C + c0;
        t01 = (rt0 * vp.ws + ct1) * C + c0;
        t10 = (rt1 * vp.ws + ct0) * C + c0;
        t11 = (rt1 * vp.ws + ct1) * C + c0;
        rlo0 = -rt0; rhi0 = vp.hs - rt0;
        rlo1 = -rt1; rhi1 = vp.hs - rt1;
        clo0 = -ct0; chi0 = vp.ws - ct0;
        clo1 = -ct1; chi1 = vp.ws - ct1;
      } else {
        tap_off = ((long long)r * dil * Wp + s * dil) * C;
      }
    }
    // multi-tap: the whole 64-k tile lies in ONE tap (kg_per % 64 == 0),
    // so the tap lookup is SCALAR per stage
    int mt_dil = 0, mt_off = 0, mt_base = 0;
    if (MT) {
      int tap = (kt * BK) / td.kg_per;
      mt_dil = td.dil[tap];
      mt_off = td.off[tap];
      mt_base = tap * td.kg_per;
    }
#pragma unroll
    for (int i = 0; i < A_SLOTS; ++i) {
      const bf16* src;
      if (VPAD == 1) {
        // per-slot: 4 int compares vs stage-scalar bounds, then select.
        // C % 64 == 0 on every bwd-data shape, so (r,s) is stage-scalar
        // and the address is precomputed-base + scalar tap_off.
        int hv = a_p[i] + vh, wv = a_q[i] + vw;
        bool ok = hv >= 0 && wv >= 0 && hv < vp.hs && wv < vp.ws;
        src = ok ? xp + a_rowbase[i] + tap_off + c0 + a_k8[i] * 8
                 : (const bf16*)g_kzero;
      } else if (VPAD == 2) {
        // parity + bounds per slot, class tap offset by 2 parity bits
        int pa = a_p[i] & 1, qa = a_q[i] & 1;
        int ah = a_p[i] >> 1, aq = a_q[i] >> 1;
        bool ok = (((a_p[i] ^ vh) | (a_q[i] ^ vw)) & 1) == 0 &&
                  ah >= (pa ? rlo1 : rlo0) && ah < (pa ? rhi1 : rhi0) &&
                  aq >= (qa ? clo1 : clo0) && aq < (qa ? chi1 : chi0);
        int off = pa ? (qa ? t11 : t10) : (qa ? t01 : t00);
        src = ok ? xp + a_rowbase[i] + off + a_k8[i] * 8
                 : (const bf16*)g_kzero;
      } else if (c64) {
        // C % 64 == 0 implies Kg % 64 == 0: no tail possible
        src = xp + a_rowbase[i] + tap_off + c0 + a_k8[i] * 8;
      } else {
        int kg = kt * BK + a_k8[i] * 8;
        if (kg >= Kg) {
          src = (const bf16*)g_kzero;        // Kg-tail zero fill
        } else if (MT) {
          int inner = kg - mt_base;
          int c = inner % C;
          int rs = inner / C;
          int s = rs % S;
          int r = rs / S;
          src = xp + a_rowbase[i] +
                ((long long)(r * mt_dil + mt_off) * Wp + s * mt_dil + mt_off)
                    * C + c;
        } else {
          int c = kg % C;
          int rs = kg / C;
          int s = rs % S;
          int r = rs / S;
          src = xp + a_rowbase[i] + ((long long)r * dil * Wp + s * dil) * C + c;
        }
      }
      GLDS16(src, bufA(buf) + (i * 4 + wave) * 1024);
    }
#pragma unroll
    for (int i = 0; i < B_SLOTS; ++i) {
      int kg = kt * BK + b_k8[i] * 8;
      const bf16* src = kg < Kg ? w + b_rowbase[i] + kg
                                : (const bf16*)g_kzero;
      GLDS16(src, bufB(buf) + (i * 4 + wave) * 1024);
    }
  };

  // ---- wave -> output sub-tile: 2x2 waves, wave tile (BM/2) x 32
  constexpr int MR = BM / 2 / 16;          // A frags per wave (4 or 2)
  constexpr int NR = 2;                    // B frags per wave
  const int wm = (wave >> 1) * (BM / 2);   // wave row offset
  const int wn = (wave & 1) * 32;          // wave col offset

  f32x4 acc[MR][NR] = {};

  const int frag_row = lane & 15;          // fragment row/col within 16
  const int frag_k = (lane >> 4) * 8;      // 8 contiguous k per lane

  const int nkt_all = (Kg + BK - 1) / BK;   // tail tile zero-filled
  int kt0 = 0, nkt = nkt_all;
  if (MODE == 2) {
    int kps = (nkt + gridDim.z - 1) / gridDim.z;
    kt0 = blockIdx.z * kps;
    nkt = min(kps, nkt_all - kt0);
  }
  // 3-stage software pipeline: tiles kt and kt+1 are in flight on entry to
  // iteration kt; kt+2 is issued right after the barrier.  The wait is a
  // MANUAL vmcnt(LPS) (LPS = this thread's GLDS ops per stage) so only tile
  // kt's DMA is drained — __syncthreads() would emit vmcnt(0) and kill the
  // overlap (guide: LDS-DMA is a pending LDS write on the VM counter).  The
  // single raw s_barrier does double duty: every wave's tile-kt loads have
  // landed, and every wave is done reading buffer (kt+2)%3 (used by kt-1).
  constexpr int LPS = A_SLOTS + B_SLOTS;
  if (nkt > 0) stage(0, kt0);
  if (STAGES == 3 && nkt > 1) stage(1, kt0 + 1);

  for (int kt = 0; kt < nkt; ++kt) {
    if (STAGES == 3) {
      // double lookahead: tile kt+1 stays in flight across the wait
      if (kt + 1 < nkt)
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(LPS) : "memory");
      else
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      if (kt + 2 < nkt) stage((kt + 2) % 3, kt0 + kt + 2);
    } else {
      // single lookahead: drain kt, fence the buffer kt+1 overwrites
      // (consumed in compute kt-1), issue kt+1, compute kt
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      if (kt + 1 < nkt) stage((kt + 1) % 2, kt0 + kt + 1);
    }
    const char* A = bufA(kt % STAGES);
    const char* B = bufB(kt % STAGES);
#pragma unroll
    for (int kk = 0; kk < BK; kk += 32) {
      bf16x8 a[MR], b[NR];
#pragma unroll
      for (int mfrag = 0; mfrag < MR; ++mfrag)
        a[mfrag] = *(const bf16x8*)(A + lds_off(wm + mfrag * 16 + frag_row,
                                                kk + frag_k));
#pragma unroll
      for (int nfrag = 0; nfrag < NR; ++nfrag)
        b[nfrag] = *(const bf16x8*)(B + lds_off(wn + nfrag * 16 + frag_row,
                                                kk + frag_k));
#pragma unroll
      for (int mfrag = 0; mfrag < MR; ++mfrag)
#pragma unroll
        for (int nfrag = 0; nfrag < NR; ++nfrag)
          acc[mfrag][nfrag] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              a[mfrag], b[nfrag], acc[mfrag][nfrag], 0, 0, 0);
    }
  }

  // ---- epilogue: D fragment lane l holds col = l&15, rows (l>>4)*4 + v;
  // stores go at Ktrue stride and skip the zero-padded out channels
  const int col = bn * BN + wn + frag_row;
  float bs[NR] = {}, bq[NR] = {};          // per-lane BN partials (2 cols)
#pragma unroll
  for (int mfrag = 0; mfrag < MR; ++mfrag) {
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      long long m = (long long)bm * BM + wm + mfrag * 16 + (lane >> 4) * 4 + v;
      if (m < M) {
        if (MODE == 2) {
          float* out = aux + ((long long)blockIdx.z * M + m) * Kout + col;
#pragma unroll
          for (int nfrag = 0; nfrag < NR; ++nfrag)
            out[nfrag * 16] = acc[mfrag][nfrag][v];
          continue;
        }
#pragma unroll
        for (int nfrag = 0; nfrag < NR; ++nfrag)
          if (col + nfrag * 16 < Ktrue) {
            bf16 h = __float2bfloat16(acc[mfrag][nfrag][v]);
            y[m * Ktrue + col + nfrag * 16] = h;
            if (MODE == 1) {
              float f = __bfloat162float(h);   // stats over the ROUNDED y
              bs[nfrag] += f;
              bq[nfrag] += f * f;
            }
          }
      }
    }
  }
  if (MODE == 1) {
    // channel totals: xor-reduce the 4 lane-groups sharing a column, then
    // combine the wave pairs (wn 0: waves 0,2; wn 32: waves 1,3) via LDS
#pragma unroll
    for (int f = 0; f < NR; ++f) {
#pragma unroll
      for (int off = 16; off < 64; off <<= 1) {
        bs[f] += __shfl_xor(bs[f], off, 64);
        bq[f] += __shfl_xor(bq[f], off, 64);
      }
    }
    float* red = (float*)smem;               // [4 waves][16 fr][4]
    __syncthreads();                         // pipeline LDS reads done
    if (lane < 16) {
      float* r = red + (wave * 16 + frag_row) * 4;
      r[0] = bs[0];
      r[1] = bq[0];
      r[2] = bs[1];
      r[3] = bq[1];
    }
    __syncthreads();
    // one thread per channel writes the workgroup's partial row
    if (tid < 64) {
      int grp = tid >> 5;                    // 0: wn=0 (waves 0,2), 1: wn=32
      int nf = (tid >> 4) & 1;
      int fr = tid & 15;
      float s = red[((grp + 0) * 16 + fr) * 4 + 2 * nf]
              + red[((grp + 2) * 16 + fr) * 4 + 2 * nf];
      float q = red[((grp + 0) * 16 + fr) * 4 + 2 * nf + 1]
              + red[((grp + 2) * 16 + fr) * 4 + 2 * nf + 1];
      // layout [Kout/64 = bn][mtiles = gridDim.x][2][64]
      float* out = aux +
          (((long long)bn * gridDim.x + bm) * 2) * 64;
      out[tid] = s;
      out[64 + tid] = q;
    }
  }
}

// ------------------------------------------------------- bwd-weight (dw)
// dw[kout][rsc] = sum_m dy[m][kout] * im2col(xp)[m][rsc] — a GEMM whose
// reduction dim (m = N*P*Q) is the MAJOR axis of both operands, so MFMA
// fragments (8 reduction-contiguous bf16 per lane) cannot be loaded from the
// natural layouts.  Instead of gathering scalars (latency-bound) or
// materializing im2col + a library split-K GEMM (extra HBM round-trips),
// both operands are TRANSPOSED ONCE with an LDS-tiled transpose:
//
//   dyT [K][M]          <- dy  [M][K]      (transpose_mk_batch_kernel)
//   xpT [C][N][Hp][Wp]  <- xp  [N][Hp][Wp][C]   (same launch, M' = N*Hp*Wp)
//
// and the GEMM reads its B operand IMPLICITLY from xpT: for a fixed
// (r, s, c) row, 8 consecutive m are 8 consecutive q, which in xpT is 16
// contiguous bytes (stride 1, Q % 8 == 0) — so both tiles stage with the
// same glds 16 B/lane + XOR-swizzle + 3-stage pipeline as the forward
// kernel.  Output: fp32 partials [SPLITS][K][RSC] (one m-slice per split),
// column-summed to bf16 by colsum_to_bf16_kernel.
//
// Qualifying shapes: plan_dw's `fast` (Q % 8 == 0, P/Q powers of two,
// K, C, M multiples of 64; stride 2 through even/odd-column planes) —
// 15 of the 17 ResNet18 convs.  Everything else takes the im2col +
// split-K library-GEMM path below.

// LDS-tiled 64x64 bf16 transpose: out[k][m] = in[m][k].  Both global phases
// are 16 B/lane coalesced; the store-phase LDS gather reads 8 scalars whose
// rows step by 8, so the swizzle folds in (row>>3)&7 as well as row&7 —
// plain chunk^(row&7) would leave all 64 lanes on one 4-bank group.
__device__ __forceinline__ int tr_off(int row, int k) {
  int chunk = (k >> 3) ^ (row & 7) ^ ((row >> 3) & 7);
  return row * 128 + chunk * 16 + (k & 7) * 2;
}

// load phase of a 64x64 tile: LDS row = input row, 8 contiguous columns per
// lane; src(row) points at the row's first column
template <typename Src>
__device__ __forceinline__ void tr_load64(char* smem, int tid, Src src) {
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    int d = i * 256 + tid;
    int row = d >> 3, c = d & 7;
    *(bf16x8*)(smem + tr_off(row, c * 8)) = *(const bf16x8*)(src(row) + c * 8);
  }
}

// store phase: output row = input column, 8 input rows gathered per lane;
// dst(row) points at the output row's first element
template <typename Dst>
__device__ __forceinline__ void tr_store64(const char* smem, int tid, Dst dst) {
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    int d = i * 256 + tid;
    int row = d >> 3, c = d & 7;
    bf16x8 v;
#pragma unroll
    for (int j = 0; j < 8; ++j)
      v[j] = *(const bf16*)(smem + tr_off(c * 8 + j, row));
    *(bf16x8*)(dst(row) + c * 8) = v;
  }
}

// Batched transpose: the 2-3 operand transposes of ONE dw call (dyT +
// xpT[+ xpT2]) issued as a SINGLE launch — each costs ~6 us of which most
// is launch/ramp latency at these sizes (~32 transpose launches/step,
// ~190 us, round-2 profile).  1-D grid linearizes all jobs' 64x64 tiles.
// mscale/moff subsample the input rows (out[k][m'] = in[m'*mscale+moff][k])
// — used to build the even/odd-column planes for the stride-2 dw path.
struct TransJob {
  const bf16* in;           // [M*mscale][K]
  bf16* out;                // [K][M]
  long long M;
  int K;
  long long mscale, moff;
  long long tile0;          // first linear tile of this job
};

__global__ __launch_bounds__(256)
void transpose_mk_batch_kernel(TransJob j0, TransJob j1, TransJob j2,
                               int njobs, long long total_tiles) {
  __shared__ char smem[64 * 128];
  const int tid = threadIdx.x;
  long long t = blockIdx.x;
  if (t >= total_tiles) return;
  TransJob j = j0;
  if (njobs > 2 && t >= j2.tile0) j = j2;
  else if (njobs > 1 && t >= j1.tile0) j = j1;
  long long rel = t - j.tile0;
  const long long mtiles = j.M / 64;
  const long long mt = (rel % mtiles) * 64;
  const int kt = (int)(rel / mtiles) * 64;
  tr_load64(smem, tid, [&](int row) {
    return j.in + ((mt + row) * j.mscale + j.moff) * j.K + kt;
  });
  __syncthreads();
  tr_store64(smem, tid, [&](int kr) {
    return j.out + (long long)(kt + kr) * j.M + mt;
  });
}

// Vectorized bwd-data weight rotation: wrot[c][R-1-r][S-1-s][k] =
// w[k][r][s][c] — i.e. the 64x64 LDS transpose above with the OUTPUT row
// index permuted ((r,s,c) -> (c, R-1-r, S-1-s)).  The scalar rot_weight
// fallback below measured 9 GB/s (2-B scattered stores, 144 wavefronts);
// this runs at transpose speed.  Host-gated on K % 64 == 0, R*S*C % 64 == 0.
__global__ __launch_bounds__(256)
void rot_weight64_kernel(const bf16* __restrict__ w,   // [K][R*S*C]
                         bf16* __restrict__ wr,        // [R*S*C][K] permuted
                         int K, int R, int S, int C) {
  __shared__ char smem[64 * 128];
  const int tid = threadIdx.x;
  const int kt = blockIdx.x * 64;          // k tile (input rows)
  const int jt = blockIdx.y * 64;          // rsc tile (input cols)
  const int RSC = R * S * C;
  tr_load64(smem, tid, [&](int row) {
    return w + (long long)(kt + row) * RSC + jt;
  });
  __syncthreads();
  tr_store64(smem, tid, [&](int jr) {
    int rsc = jt + jr;
    int cc = rsc % C;
    int rs = rsc / C;
    int s = rs % S;
    int r = rs / S;
    long long o = ((long long)cc * R + (R - 1 - r)) * S + (S - 1 - s);
    return wr + o * K + kt;
  });
}

// dw GEMM on the transposed operands: D[kout][rsc] += A[kout][m] B[rsc][m]
// with A = dyT (plain 2-D) and B = implicit transposed im2col of xpT.
// Same 256-thread / 4-wave / 3-stage-glds structure as conv_fwd_kernel;
// BMK (kout tile) = 128 where K allows — the 64x64 tile has half the MFMA
// work per LDS read and measured ~1.7x slower — else 64; grid.z splits the
// m range into independent fp32 partials.
// B stages via LDS-DMA straight from the (only 2-B aligned) xpT rows.
// Measured on gfx950: unaligned global_load_lds is CORRECT (all numerics
// tests pass) and 34-40 % faster than register staging + ds_write (layer3
// dw 64.6 -> 38.8 us).
// STRIDE=2 reads from TWO half-width transposed planes (even/odd input
// columns): 8 consecutive output q stay contiguous within the plane of
// the filter column's parity, so the same glds staging applies; Wp is the
// PLANE width and xpT2 the odd plane.
// NT=2 doubles the rsc tile (two B tiles share one A stage: 8 MFMAs per
// 6 LDS reads instead of 4 per 4) — used for layer1 (K=64 caps the kout
// tile at 64 and its 48.8 us was the largest single kernel).
// (Two Q == 4 variants and a register-staged B were measured slower and
// removed — NOTES.md, "Measured dead ends".)
template <int BMK, int STRIDE, int NT>
__global__ __launch_bounds__(256)
void dw_gemm_kernel(const bf16* __restrict__ dyT,  // [K][M]
                    const bf16* __restrict__ xpT,  // [C][N][Hp][Wp(lane)]
                    const bf16* __restrict__ xpT2, // odd plane (STRIDE=2)
                    float* __restrict__ part,      // [SPLITS][K][RSC]
                    int K, int C, int N, int Hp, int Wp, int S,
                    long long M, int RSC, int mtiles_per_split,
                    int qshift /* log2 Q */, int qmask,
                    int pshift /* log2 (P*Q) */, int pmask) {
  constexpr int BNT = BN * NT;             // rsc tile rows
  constexpr int AB = BMK * BK * 2;         // A tile bytes
  constexpr int BB = BNT * BK * 2;         // B tile bytes
  __shared__ char smem[3 * (AB + BB)];

  const int tid = threadIdx.x;
  const int wave = tid >> 6;
  const int lane = tid & 63;
  const int rrow0 = blockIdx.x * BNT;      // rsc tile base
  const int krow0 = blockIdx.y * BMK;      // kout tile base
  const long long m0 =
      (long long)blockIdx.z * mtiles_per_split * BK;
  const int nkt = (int)std::min<long long>(mtiles_per_split,
                                           (M - m0 + BK - 1) / BK);

  // fixed staging slots (A_SLOTS A + 2 B per thread), fwd-kernel scheme:
  // slot d = i*256 + tid -> LDS row d>>3, swizzled m-chunk (d&7)^(row&7)
  constexpr int A_SLOTS = (BMK * BK) / (256 * 8);  // 2 or 4
  long long a_base[A_SLOTS];
  int a_k8[A_SLOTS];
#pragma unroll
  for (int i = 0; i < A_SLOTS; ++i) {
    int d = i * 256 + tid;
    int row = d >> 3;
    a_k8[i] = (d & 7) ^ (row & 7);
    a_base[i] = (long long)(krow0 + row) * M;
  }
  constexpr int BS = 2 * NT;               // B slots per thread
  long long b_base[BS];                    // plane (c, r-row, s-col) offset
  const bf16* b_plane[BS];
  int b_k8[BS];
#pragma unroll
  for (int i = 0; i < BS; ++i) {
    int d = i * 256 + tid;
    int row = d >> 3;
    b_k8[i] = (d & 7) ^ (row & 7);
    int rsc = rrow0 + row;
    if (rsc >= RSC) rsc = RSC - 1;         // tail tile: junk rows, stores guarded
    int c = rsc % C;
    int rs = rsc / C;
    int s = rs % S;
    int r = rs / S;
    if (STRIDE == 2) {
      b_plane[i] = (s & 1) ? xpT2 : xpT;
      b_base[i] = ((long long)c * N * Hp + r) * Wp + (s >> 1);
    } else {
      b_plane[i] = xpT;
      b_base[i] = ((long long)c * N * Hp + r) * Wp + s;
    }
  }

  auto bufA = [&](int b) -> char* { return smem + b * (AB + BB); };
  auto bufB = [&](int b) -> char* { return smem + b * (AB + BB) + AB; };

  // A (dyT rows, always 16-B aligned) and B (xpT rows shifted by the filter
  // column s, so only 2-B aligned) both stage via glds
  auto stage = [&](int buf, int kt) {
    const long long mt = m0 + (long long)kt * BK;
#pragma unroll
    for (int i = 0; i < A_SLOTS; ++i) {
      const bf16* src = dyT + a_base[i] + mt + a_k8[i] * 8;
      GLDS16(src, bufA(buf) + (i * 4 + wave) * 1024);
    }
#pragma unroll
    for (int i = 0; i < BS; ++i) {
      long long mm = mt + b_k8[i] * 8;     // 8 consecutive m = 8 consecutive q
      int q = (int)(mm & qmask);
      int p = (int)((mm >> qshift) & pmask);
      int n = (int)(mm >> pshift);
      const bf16* src =
          b_plane[i] + b_base[i] + ((long long)n * Hp + p * STRIDE) * Wp + q;
      GLDS16(src, bufB(buf) + (i * 4 + wave) * 1024);
    }
  };

  constexpr int MR = BMK / 2 / 16;         // kout frags per wave (2 or 4)
  constexpr int NRW = 2 * NT;              // rsc frags per wave
  const int frag_row = lane & 15;
  const int frag_k = (lane >> 4) * 8;
  f32x4 acc[MR][NRW] = {};                 // wave tile (BMK/2) x (BNT/2)
  const int wk = (wave >> 1) * (BMK / 2);
  const int wr = (wave & 1) * (BNT / 2);

  if (nkt > 0) {
    stage(0, 0);
    if (nkt > 1) stage(1, 1);
    for (int kt = 0; kt < nkt; ++kt) {
      // drain stage kt's glds ops (A_SLOTS + BS); stage kt+1's stay in flight
      if (kt + 1 < nkt)
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(A_SLOTS + BS) : "memory");
      else
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      if (kt + 2 < nkt) stage((kt + 2) % 3, kt + 2);
      const char* A = bufA(kt % 3);
      const char* B = bufB(kt % 3);
#pragma unroll
      for (int kk = 0; kk < BK; kk += 32) {
        bf16x8 a[MR], b[NRW];
#pragma unroll
        for (int f = 0; f < MR; ++f)
          a[f] = *(const bf16x8*)(A + lds_off(wk + f * 16 + frag_row,
                                              kk + frag_k));
#pragma unroll
        for (int f = 0; f < NRW; ++f)
          b[f] = *(const bf16x8*)(B + lds_off(wr + f * 16 + frag_row,
                                              kk + frag_k));
#pragma unroll
        for (int fa = 0; fa < MR; ++fa)
#pragma unroll
          for (int fb = 0; fb < NRW; ++fb)
            acc[fa][fb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                a[fa], b[fb], acc[fa][fb], 0, 0, 0);
      }
    }
  }

  // ---- epilogue: D[kout][rsc] fragments -> this split's fp32 partial slab
  float* out = part + (long long)blockIdx.z * K * RSC;
  const int col = rrow0 + wr + frag_row;
#pragma unroll
  for (int fa = 0; fa < MR; ++fa) {
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      int k = krow0 + wk + fa * 16 + (lane >> 4) * 4 + v;
#pragma unroll
      for (int fb = 0; fb < NRW; ++fb)
        if (NT == 1 || col + fb * 16 < RSC)
          out[(long long)k * RSC + col + fb * 16] = acc[fa][fb][v];
    }
  }
}

// column-sum the [SPLITS][L] fp32 partials into bf16 (thread per column,
// rows are contiguous so warps read coalesced)
__global__ void colsum_to_bf16_kernel(const float* __restrict__ part,
                                      int splits, long long L,
                                      bf16* __restrict__ out) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
       i < L; i += (long long)gridDim.x * blockDim.x) {
    float s = 0.f;
    for (int b = 0; b < splits; ++b) s += part[(long long)b * L + i];
    out[i] = __float2bfloat16(s);
  }
}

// first-stage column reduction [SPLITS][L] -> [G][L]: with L as small as
// 36 K (layer1 dw) a single-stage colsum has too few threads to cover the
// read latency (measured 0.57 TB/s); grid.y = G groups raise parallelism
// G-fold and the [G][L] slab is finished by colsum_to_bf16_kernel.
__global__ void colsum_stage_kernel(const float* __restrict__ part,
                                    int rows_per_group, long long L,
                                    float* __restrict__ out) {
  const float* src = part + (long long)blockIdx.y * rows_per_group * L;
  float* dst = out + (long long)blockIdx.y * L;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
       i < L; i += (long long)gridDim.x * blockDim.x) {
    float s = 0.f;
    for (int b = 0; b < rows_per_group; ++b) s += src[(long long)b * L + i];
    dst[i] = s;
  }
}

// ---------------------------------------------------------------- transforms

// OUTPUT-indexed zero-pad/dilate NHWC, 16 B/lane (8 bf16 = one C-chunk;
// VEC=1 scalar fallback for C % 8 != 0, e.g. conv1's C=3):
// out[n][h*str+pt][w*str+pl][c] = in[n][h][w][c], everything else 0.
// str=1 is plain padding.  Writes the whole output (no separate zero fill).
template <int VEC>
__global__ void dilate_pad_out_kernel(const bf16* __restrict__ in,
                                      bf16* __restrict__ out, int N, int H,
                                      int W, int Cv /* C/VEC */, int Hp,
                                      int Wp, int pt, int pl, int str) {
  using V = __attribute__((ext_vector_type(VEC))) __bf16;
  const V* inv = reinterpret_cast<const V*>(in);
  V* outv = reinterpret_cast<V*>(out);
  long long total = (long long)N * Hp * Wp * Cv;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
       i < total; i += (long long)gridDim.x * blockDim.x) {
    int cv = (int)(i % Cv);
    long long t = i / Cv;
    int wp = (int)(t % Wp);
    t /= Wp;
    int hp = (int)(t % Hp);
    int n = (int)(t / Hp);
    int hs = hp - pt, ws = wp - pl;
    V v = {};
    if (hs >= 0 && ws >= 0 && hs % str == 0 && ws % str == 0) {
      int h = hs / str, w = ws / str;
      if (h < H && w < W)
        v = inv[(((long long)n * H + h) * W + w) * Cv + cv];
    }
    outv[i] = v;
  }
}

// weight rotation for bwd-data: wrot[c][r][s][k] = w[k][R-1-r][S-1-s][c]
template <typename T>
__global__ void rot_weight_kernel(const T* __restrict__ w, T* __restrict__ wr,
                                  int K, int R, int S, int C) {
  long long total = (long long)K * R * S * C;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
       i < total; i += (long long)gridDim.x * blockDim.x) {
    int c = (int)(i % C);
    long long t = i / C;
    int s = (int)(t % S);
    t /= S;
    int r = (int)(t % R);
    int k = (int)(t / R);
    wr[((((long long)c * R + (R - 1 - r)) * S + (S - 1 - s)) * K) + k] = w[i];
  }
}

// im2col from the PADDED input (for bwd-weight GEMM), 16 B/lane vectors
// (the 8-chunk never crosses a (r,s) boundary since C % 8 == 0; VEC=1
// scalar fallback for small C):
// col[m][r*S*C + s*C + c] = xp[n][p*stride+r][q*stride+s][c], m=(n,p,q)
template <int VEC>
__global__ void im2col_kernel(const bf16* __restrict__ xp,
                              bf16* __restrict__ col, int N, int Hp, int Wp,
                              int C, int R, int S, int P, int Q, int stride,
                              int dil) {
  using V = __attribute__((ext_vector_type(VEC))) __bf16;
  const V* xv = reinterpret_cast<const V*>(xp);
  V* cv = reinterpret_cast<V*>(col);
  long long M = (long long)N * P * Q;
  long long Kv = (long long)R * S * C / VEC;
  long long total = M * Kv;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
       i < total; i += (long long)gridDim.x * blockDim.x) {
    long long m = i / Kv;
    int k8 = (int)(i % Kv);
    int c8 = k8 % (C / VEC);
    int rs = k8 / (C / VEC);
    int s = rs % S;
    int r = rs / S;
    int q = (int)(m % Q);
    int p = (int)((m / Q) % P);
    int n = (int)(m / ((long long)P * Q));
    cv[i] = xv[((((long long)n * Hp + p * stride + r * dil) * Wp +
                 (q * stride + s * dil)) * C) / VEC + c8];
  }
}

// 3-D-grid dilate/pad for C % 8 == 0: block.x covers Wp*Cv (Cv = C/8 is a
// power of two -> shifts), grid.y = Hp, grid.z = N — no per-element integer
// division (the flat-index form's div/mod by runtime Wp/Hp/Cv cost more
// than the memory traffic at these sizes).
__global__ void dilate_pad_out3d_kernel(const bf16* __restrict__ in,
                                        bf16* __restrict__ out, int H, int W,
                                        int cvshift, int Wp, int pt, int pl,
                                        int str) {
  typedef __attribute__((ext_vector_type(8))) __bf16 v8;
  const int Cv = 1 << cvshift;
  const int hp = blockIdx.y, n = blockIdx.z;
  const int hs = hp - pt;
  const bool hok = hs >= 0 && hs % str == 0 && hs / str < H;
  const int h = hs / str;
  const v8* inv = reinterpret_cast<const v8*>(in);
  v8* outv = reinterpret_cast<v8*>(out);
  long long orow = ((long long)n * gridDim.y + hp) * Wp << cvshift;
  long long irow = ((long long)n * H + h) * W << cvshift;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < (Wp << cvshift);
       i += gridDim.x * blockDim.x) {
    int wp = i >> cvshift;
    int cv = i - (wp << cvshift);
    int ws = wp - pl;
    v8 v = {};
    if (hok && ws >= 0 && ws % str == 0 && ws / str < W)
      v = inv[irow + ((long long)(ws / str) << cvshift) + cv];
    outv[orow + i] = v;
  }
}

// str = 1 is plain zero padding
at::Tensor dilate_pad_nhwc(const at::Tensor& x, int pt, int pb, int pl,
                           int pr, int str) {
  int N = x.size(0), C = x.size(1), H = x.size(2), W = x.size(3);
  int Hp = (H - 1) * str + 1 + pt + pb, Wp = (W - 1) * str + 1 + pl + pr;
  auto xp = at::empty({N, C, Hp, Wp},
                      x.options().memory_format(at::MemoryFormat::ChannelsLast));
  auto stream = fedkit_stream();
  if (C % 8 == 0 && ((C / 8) & (C / 8 - 1)) == 0) {
    int cvshift = __builtin_ctz((unsigned)(C / 8));
    int wc = Wp << cvshift;
    hipLaunchKernelGGL(dilate_pad_out3d_kernel,
                       dim3((wc + 255) / 256, Hp, N), dim3(256), 0, stream,
                       (const bf16*)x.data_ptr(), (bf16*)xp.data_ptr(), H, W,
                       cvshift, Wp, pt, pl, str);
  } else if (C % 8 == 0) {
    long long total = (long long)N * Hp * Wp * C / 8;
    hipLaunchKernelGGL(dilate_pad_out_kernel<8>, dim3(grid_1d(total, 256)),
                       dim3(256), 0, stream, (const bf16*)x.data_ptr(),
                       (bf16*)xp.data_ptr(), N, H, W, C / 8, Hp, Wp, pt, pl,
                       str);
  } else {
    long long total = (long long)N * Hp * Wp * C;
    hipLaunchKernelGGL(dilate_pad_out_kernel<1>, dim3(grid_1d(total, 256)),
                       dim3(256), 0, stream, (const bf16*)x.data_ptr(),
                       (bf16*)xp.data_ptr(), N, H, W, C, Hp, Wp, pt, pl, str);
  }
  return xp;
}

at::Tensor pad_nhwc(const at::Tensor& x, int pad) {
  return pad > 0 ? dilate_pad_nhwc(x, pad, pad, pad, pad, 1) : x;
}

void check_conv_inputs(const at::Tensor& x, const at::Tensor& w) {
  TORCH_CHECK(x.scalar_type() == at::kBFloat16 &&
              w.scalar_type() == at::kBFloat16,
              "conv MFMA kernel is bf16-only (the MI355X fast path)");
  TORCH_CHECK(x.is_contiguous(at::MemoryFormat::ChannelsLast),
              "conv input must be channels_last");
  TORCH_CHECK(w.is_contiguous(at::MemoryFormat::ChannelsLast),
              "conv weight must be channels_last");
}

// ---- plan -> kernel: one table per kernel family, expanded from the variant
// lists in conv_plan.h (so exactly the listed kernels are instantiated)
using ConvKernel = decltype(&conv_fwd_kernel<64, 1, 0, 2, false, 0>);
struct ConvVariant {
  int BM, stride, mode, stages;
  bool mt;
  int vpad;
  ConvKernel kern;
};
#define X(bm, st, mode, stages, mt, vpad) \
  {bm, st, mode, stages, mt, vpad,        \
   conv_fwd_kernel<bm, st, mode, stages, mt, vpad>},
const ConvVariant kConvVariants[] = {FEDKIT_CONV_VARIANTS(X)};
#undef X

using DwKernel = decltype(&dw_gemm_kernel<64, 1, 1>);
struct DwVariant {
  int BMK, stride, NT;
  DwKernel kern;
};
#define X(bmk, st, nt) {bmk, st, nt, dw_gemm_kernel<bmk, st, nt>},
const DwVariant kDwVariants[] = {FEDKIT_DW_VARIANTS(X)};
#undef X

struct ConvDims {
  int N, Hp, Wp, C, Kout, R, S, P, Q, Kg, dil, Ktrue;
};

void launch_conv(const ConvPlan& p, const ConvDims& d, const at::Tensor& xp,
                 const at::Tensor& w, at::Tensor& y, float* aux,
                 const TapDesc& td, const VPadDesc& vp) {
  ConvKernel kern = nullptr;
  for (const ConvVariant& v : kConvVariants)
    if (v.BM == p.BM && v.stride == p.stride && v.mode == p.mode &&
        v.stages == p.stages && v.mt == p.multitap && v.vpad == p.vpad)
      kern = v.kern;
  TORCH_CHECK(kern, "no conv_fwd_kernel for plan BM=", p.BM, " stride=",
              p.stride, " mode=", p.mode, " stages=", p.stages, " multitap=",
              p.multitap, " vpad=", p.vpad);
  hipLaunchKernelGGL(kern, dim3(p.grid_x, p.grid_y, p.splits), dim3(256), 0,
                     fedkit_stream(), (const bf16*)xp.data_ptr(),
                     (const bf16*)w.data_ptr(), (bf16*)y.data_ptr(), d.N,
                     d.Hp, d.Wp, d.C, d.Kout, d.R, d.S, d.P, d.Q, d.Kg, d.dil,
                     d.Ktrue, aux, td, vp);
}

// launch on the PRE-PADDED input; pad already folded into Hp/Wp.
// Ktrue < Kout means the trailing weight rows are channel zero-padding
// (VAE/CPC shapes): y is allocated and stored dense at Ktrue channels.
// vpad != nullptr: xp is the RAW gy (bwd-data) and the kernel performs the
// dilate+pad virtually in the A stage (requires C % 64 == 0, stride 1).
// bnpart != nullptr: run the MODE-1 epilogue and hand back its BatchNorm
// partials slab [Kout/64][gridDim.x][2][64] through *bnpart.  The slab is
// allocated HERE, from the plan's grid, because the epilogue indexes it by
// gridDim.x: no caller holds a tile rule.
at::Tensor conv_core(const at::Tensor& xp, const at::Tensor& w_krs_c,
                     int stride, int P, int Q, ConvCaller caller, int dil = 1,
                     int Ktrue = -1, at::Tensor* bnpart = nullptr,
                     const VPadDesc* vpad = nullptr) {
  int N = xp.size(0), C = xp.size(1), Hp = xp.size(2), Wp = xp.size(3);
  int Kout = w_krs_c.size(0), R = w_krs_c.size(2), S = w_krs_c.size(3);
  int Kg = R * S * C;
  if (Ktrue < 0) Ktrue = Kout;
  TORCH_CHECK(C % 8 == 0, "conv kernel needs C % 8 == 0, got ", C);
  // Kg % 64 != 0 is allowed: the kernel zero-fills the tail K-tile from a
  // device zero page (Net-family 5x5 / valid-3x3 shapes)
  TORCH_CHECK(Kout % BN == 0, "conv kernel needs Kout % 64 == 0, got ", Kout);
  TORCH_CHECK(stride == 1 || stride == 2, "conv kernel supports stride 1/2");
  TORCH_CHECK(!bnpart || (Ktrue == Kout && !vpad),
              "conv BN-stats epilogue needs dense Kout and no virtual pad");
  TORCH_CHECK(!vpad || (C % 64 == 0 && stride == 1),
              "vpad path needs C % 64 == 0, stride-1 conv");
  long long M = (long long)N * P * Q;
  const ConvPlan p = plan_conv(M, Kout, Kg, stride, Ktrue == Kout,
                               bnpart != nullptr, vpad ? vpad->vstr : 0,
                               caller);
  auto y = at::empty({N, Ktrue, P, Q},
                     xp.options().memory_format(at::MemoryFormat::ChannelsLast));
  at::Tensor part;
  float* aux = nullptr;
  if (bnpart) {
    *bnpart = at::empty({(long long)p.grid_y, (long long)p.grid_x, 2, BN},
                        xp.options().dtype(at::kFloat));
    aux = bnpart->data_ptr<float>();
  }
  if (p.splits > 1) {
    part = at::empty({p.splits, M, (long long)Kout},
                     xp.options().dtype(at::kFloat));
    aux = part.data_ptr<float>();
  }
  launch_conv(p, {N, Hp, Wp, C, Kout, R, S, P, Q, Kg, dil, Ktrue}, xp,
              w_krs_c, y, aux, TapDesc{}, vpad ? *vpad : VPadDesc{});
  if (p.splits > 1) {
    long long Ly = M * Kout;
    hipLaunchKernelGGL(colsum_to_bf16_kernel, dim3(grid_1d(Ly, 256)),
                       dim3(256), 0, fedkit_stream(), part.data_ptr<float>(),
                       p.splits, Ly, (bf16*)y.data_ptr());
  }
  return y;
}

}  // namespace

// the instantiated kernels, from the dispatch tables (coverage test)
std::vector<std::vector<long>> fedkit_conv_variants() {
  std::vector<std::vector<long>> out;
  for (const ConvVariant& v : kConvVariants)
    out.push_back({v.BM, v.stride, v.mode, v.stages, v.vpad, v.mt});
  return out;
}

std::vector<std::vector<long>> fedkit_dw_variants() {
  std::vector<std::vector<long>> out;
  for (const DwVariant& v : kDwVariants)
    out.push_back({v.BMK, v.stride, v.NT});
  return out;
}

// Fused multi-dilation conv bank (CPC EncoderCNN, simple_models.py:441-460):
// n_tap convs share one input and one launch.  x [N,C,H,W] NHWC bf16;
// w2d [64, n_tap*R*R*C] bf16 contiguous BLOCK-DIAGONAL combined weight
// (rows t*Kt .. per tap t nonzero only in its kg block, Kt true out
// channels per tap); dils/pads per tap; all taps must produce the same
// P x Q.  Returns [N, ktrue, P, P] channels_last (the torch.cat result).
at::Tensor fedkit_conv2d_dilated_bank(const at::Tensor& x,
                                      const at::Tensor& w2d,
                                      std::vector<long> dils,
                                      std::vector<long> pads, long stride,
                                      long R, long ktrue) {
  TORCH_CHECK(x.scalar_type() == at::kBFloat16 &&
              w2d.scalar_type() == at::kBFloat16, "bank is bf16-only");
  TORCH_CHECK(x.is_contiguous(at::MemoryFormat::ChannelsLast),
              "bank input must be channels_last");
  TORCH_CHECK(w2d.is_contiguous() && w2d.size(0) == 64,
              "bank weight must be [64, n*R*R*C] contiguous");
  int n = (int)dils.size();
  TORCH_CHECK(n >= 1 && n <= 8 && (int)pads.size() == n, "1..8 taps");
  int N = x.size(0), C = x.size(1), H = x.size(2);
  TORCH_CHECK(C % 8 == 0, "bank needs C % 8 == 0");
  int kg_per = (int)(R * R * C);
  TORCH_CHECK(kg_per % BK == 0, "bank needs R*R*C % 64 == 0 per tap");
  TORCH_CHECK(w2d.size(1) == (long)n * kg_per, "bank weight Kg mismatch");
  int shared_pad = 0;
  for (long p : pads) shared_pad = std::max(shared_pad, (int)p);
  TapDesc td = {};
  td.n = n;
  td.kg_per = kg_per;
  int P = -1;
  for (int t = 0; t < n; ++t) {
    td.dil[t] = (int)dils[t];
    td.off[t] = shared_pad - (int)pads[t];
    int Reff = ((int)R - 1) * (int)dils[t] + 1;
    int Pt = (H + 2 * (int)pads[t] - Reff) / (int)stride + 1;
    TORCH_CHECK(P < 0 || Pt == P, "bank taps disagree on output size");
    P = Pt;
  }
  at::Tensor xp = pad_nhwc(x, shared_pad);
  int Hp = xp.size(2), Wp = xp.size(3);
  long long M = (long long)N * P * P;
  auto y = at::empty({N, ktrue, P, P},
                     x.options().memory_format(at::MemoryFormat::ChannelsLast));
  int Kg = n * kg_per;
  const ConvPlan p = plan_conv(M, 64, Kg, (int)stride, ktrue == 64, false, 0,
                               kBank);
  launch_conv(p, {N, Hp, Wp, C, 64, (int)R, (int)R, P, P, Kg, 1, (int)ktrue},
              xp, w2d, y, nullptr, td, VPadDesc{});
  return y;
}


at::Tensor fedkit_conv_small_fwd(const at::Tensor& x, const at::Tensor& w,
                                 long stride, long padding);  // conv_small.hip

// public dilate+pad (transposed-conv input dilation):
// out[n][h*str+pt][w*str+pl][c] = x[n][h][w][c], everything else zero
at::Tensor fedkit_dilate_pad(const at::Tensor& x, long pt, long pb, long pl,
                             long pr, long str) {
  TORCH_CHECK(x.is_contiguous(at::MemoryFormat::ChannelsLast),
              "dilate_pad expects channels_last");
  return dilate_pad_nhwc(x, (int)pt, (int)pb, (int)pl, (int)pr, (int)str);
}

at::Tensor fedkit_conv2d_pad_input(const at::Tensor& x, long padding) {
  TORCH_CHECK(x.is_contiguous(at::MemoryFormat::ChannelsLast),
              "pad_input expects channels_last");
  return pad_nhwc(x, (int)padding);
}

// forward on a PRE-PADDED input (the autograd wrapper saves xp so backward
// never re-pads): P = (Hp - Reff)/stride + 1 with Reff = (R-1)*dil + 1.
// ktrue < Kout marks trailing zero-padded out channels (generic VAE/CPC
// path); y comes back dense at ktrue channels.
at::Tensor fedkit_conv2d_fwd_prepadded(const at::Tensor& xp,
                                       const at::Tensor& w, long stride,
                                       long dil, long ktrue) {
  check_conv_inputs(xp, w);
  int Hp = xp.size(2), Wp = xp.size(3);
  int R = w.size(2), S = w.size(3);
  int Reff = (R - 1) * (int)dil + 1, Seff = (S - 1) * (int)dil + 1;
  int P = (Hp - Reff) / (int)stride + 1;
  int Q = (Wp - Seff) / (int)stride + 1;
  return conv_core(xp, w, (int)stride, P, Q, kFwd, (int)dil, (int)ktrue);
}

// prepadded forward that ALSO emits the BatchNorm stage-1 partials
// ([Kout/64][mtiles][2][64] fp32, mtiles = the tile rows conv_core
// launched) from the epilogue registers — feeds
// fedkit_bn_fwd's conv_part fast path (one launch and one full read of y
// fewer per conv+BN pair).
std::vector<at::Tensor> fedkit_conv2d_fwd_prepadded_bnstats(
    const at::Tensor& xp, const at::Tensor& w, long stride) {
  check_conv_inputs(xp, w);
  int Hp = xp.size(2), Wp = xp.size(3);
  int R = w.size(2), S = w.size(3);
  int P = (Hp - R) / (int)stride + 1;
  int Q = (Wp - S) / (int)stride + 1;
  // conv_core sizes the slab to the grid its plan launches
  at::Tensor part;
  auto y = conv_core(xp, w, (int)stride, P, Q, kFwd, 1, -1, &part);
  return {y, part};
}

at::Tensor fedkit_conv2d_fwd(const at::Tensor& x, const at::Tensor& w,
                             long stride, long padding, long dil,
                             long ktrue) {
  check_conv_inputs(x, w);
  int C = x.size(1), H = x.size(2), W = x.size(3);
  int R = w.size(2);
  if (C % 8 != 0) {  // e.g. ResNet conv1 (C=3): direct small-C kernel
    TORCH_CHECK(dil == 1 && ktrue < 0,
                "small-C conv path has no dilation/ktrue support");
    return fedkit_conv_small_fwd(x, w, stride, padding);
  }
  int Reff = (R - 1) * (int)dil + 1;
  int P = (H + 2 * (int)padding - Reff) / (int)stride + 1;
  int Q = (W + 2 * (int)padding - Reff) / (int)stride + 1;
  at::Tensor xp = pad_nhwc(x, (int)padding);
  return conv_core(xp, w, (int)stride, P, Q, kFwd, (int)dil, (int)ktrue);
}

// dx = conv_dil(dilate_str(gy), rot180(w)); gy must carry the same
// (possibly zero-padded) K channels as w; ctrue < C slices the channel
// padding off dx at the store.
at::Tensor fedkit_conv2d_bwd_data(const at::Tensor& gy, const at::Tensor& w,
                                  long stride, long padding, long H, long W,
                                  long dil, long ctrue) {
  check_conv_inputs(gy, w);
  int K = w.size(0), C = w.size(1), R = w.size(2), S = w.size(3);
  TORCH_CHECK(K % 8 == 0, "bwd-data needs Kout % 8 == 0");
  // rotate weights: wrot[c][r][s][k].  The dx GEMM's out-channel count is
  // C, which the generic (VAE/CPC) path only pads to a multiple of 8 —
  // round the wrot rows up to the 64-row tile with zeros and store dx
  // dense at ctrue via the kernel's Ktrue guard.
  int Cpad = (C + 63) / 64 * 64;
  // (empty + zero_: at::zeros drops the memory_format in options)
  auto wrot = at::empty({Cpad, K, R, S},
                        w.options().memory_format(at::MemoryFormat::ChannelsLast));
  if (Cpad != C) wrot.zero_();
  {
    auto stream = fedkit_stream();
    long long total = (long long)K * R * S * C;
    int RSC = R * S * C;
    if (K % 64 == 0 && RSC % 64 == 0)
      hipLaunchKernelGGL(rot_weight64_kernel, dim3(K / 64, RSC / 64),
                         dim3(256), 0, stream, (const bf16*)w.data_ptr(),
                         (bf16*)wrot.data_ptr(), K, R, S, C);
    else
      hipLaunchKernelGGL((rot_weight_kernel<bf16>), dim3(grid_1d(total, 256)),
                         dim3(256), 0, stream, (const bf16*)w.data_ptr(),
                         (bf16*)wrot.data_ptr(), K, R, S, C);
  }
  if (ctrue < 0) ctrue = C;
  if (R == 1 && S == 1 && stride == 2 && padding == 0) {
    // 1x1 stride-2 shortcut dx: only every other pixel is nonzero, so the
    // dilate-then-conv form runs the GEMM at 4x the useful M.  Instead:
    // dense GEMM at the SMALL resolution, then one zero-interleave pass
    // (dx[2p][2q] = sum_k gy[p][q][k] w[k][c]).
    int P = gy.size(2), Q = gy.size(3);
    auto dxs = conv_core(gy, wrot, 1, P, Q, kBwd, 1, (int)ctrue);
    int pb = (int)H - ((P - 1) * 2 + 1);
    int pr = (int)W - ((Q - 1) * 2 + 1);
    return dilate_pad_nhwc(dxs, 0, pb, 0, pr, 2);
  }
  // dilate+pad gy: pl = (R-1)*dil - pad, pr = pl + a with
  // a = (H + 2p - Reff) % stride, Reff = (R-1)*dil + 1.
  // Fast path: the pad/dilation happens VIRTUALLY in the conv kernel's A
  // stage (zero-page substitution per out-of-range chunk) — no gyp buffer,
  // no dilate_pad launch, no extra y-sized HBM round trip.
  int Reff = (R - 1) * (int)dil + 1;
  int pl = (Reff - 1) - (int)padding;
  static const bool no_vpad = []() {
    const char* e = getenv("FEDKIT_NO_VPAD");
    return e && atoi(e) == 1;
  }();
  int K64 = gy.size(1);
  // stride 1: affine gy address + per-slot int compares (first cut with
  // per-slot 64-bit muls measured SLOWER than the materialized dilate;
  // this form measured layer1 dx 42.4 -> 29.1 us).
  // stride 2: parity-class form — skips the 3/4-zeros A traffic of the
  // zero-inserted image; wins at large spatial (60.1 -> 49.8 us at H=32)
  // but LOSES at H=8 (52.4 -> 61.4, latency-bound small grid), so gated
  // on the dx spatial size (gpurun_out/ab3_*.log).
  bool vpad_ok = !no_vpad && K64 % 64 == 0 && pl >= 0 &&
      (stride == 1 || (stride == 2 && H >= 16));
  if (vpad_ok) {
    VPadDesc vp{(int)gy.size(2), (int)gy.size(3), pl, (int)stride};
    return conv_core(gy, wrot, 1, (int)H, (int)W, kBwd, (int)dil, (int)ctrue,
                     nullptr, &vp);
  }
  int a = (int)((H + 2 * padding - Reff) % stride);
  at::Tensor gyp = dilate_pad_nhwc(gy, pl, pl + a, pl, pl + a, (int)stride);
  return conv_core(gyp, wrot, 1, (int)H, (int)W, kBwd, (int)dil, (int)ctrue);
}

// bwd-weight from the PRE-PADDED input saved by the forward
at::Tensor fedkit_conv2d_bwd_weight_prepadded(const at::Tensor& gy,
                                              const at::Tensor& xp,
                                              long stride, long R_in,
                                              long S_in, long dil) {
  check_conv_inputs(gy, xp);
  int N = xp.size(0), C = xp.size(1), Hp = xp.size(2), Wp = xp.size(3);
  int K = gy.size(1), P = gy.size(2), Q = gy.size(3);
  int R = (int)R_in, S = (int)S_in;
  long long M = (long long)N * P * Q;
  long long RSC = (long long)R * S * C;
  const DwPlan d = plan_dw(N, C, Hp, Wp, K, P, Q, R, S, (int)stride, (int)dil);

  // transpose-then-implicit-GEMM MFMA path (no col buffer, no library GEMM):
  // see the dw block comment above the kernels.  Stride 1 uses one
  // transposed plane; stride 2 uses EVEN/ODD-column planes (each filter
  // column's parity is fixed, so 8 consecutive q remain contiguous in its
  // plane) — together 15/17 ResNet18 convs.
  if (d.fast) {
    auto stream = fedkit_stream();
    long long NHW = (long long)N * Hp * Wp;
    auto dyT = at::empty({(long long)K, M}, gy.options());
    at::Tensor xpT, xpT2;
    int Wlane = Wp;
    // all operand transposes of this dw call in ONE launch
    TransJob jd = {(const bf16*)gy.data_ptr(), (bf16*)dyT.data_ptr(),
                   M, K, 1LL, 0LL, 0LL};
    TransJob jx = {}, jx2 = {};
    int njobs;
    long long tiles = (M / 64) * (K / 64);
    if (stride == 1) {
      xpT = at::empty({(long long)C, NHW}, xp.options());
      jx = {(const bf16*)xp.data_ptr(), (bf16*)xpT.data_ptr(),
            NHW, C, 1LL, 0LL, tiles};
      tiles += (NHW / 64) * (C / 64);
      njobs = 2;
    } else {
      Wlane = Wp / 2;
      long long NHW2 = NHW / 2;
      xpT = at::empty({(long long)C, NHW2}, xp.options());
      xpT2 = at::empty({(long long)C, NHW2}, xp.options());
      jx = {(const bf16*)xp.data_ptr(), (bf16*)xpT.data_ptr(),
            NHW2, C, 2LL, 0LL, tiles};
      tiles += (NHW2 / 64) * (C / 64);
      jx2 = {(const bf16*)xp.data_ptr(), (bf16*)xpT2.data_ptr(),
             NHW2, C, 2LL, 1LL, tiles};
      tiles += (NHW2 / 64) * (C / 64);
      njobs = 3;
    }
    hipLaunchKernelGGL(transpose_mk_batch_kernel, dim3((unsigned)tiles),
                       dim3(256), 0, stream, jd, jx, jx2, njobs, tiles);
    int qshift = __builtin_ctz((unsigned)Q);
    int pshift = qshift + __builtin_ctz((unsigned)P);
    auto part = at::empty({d.splits, (long long)K, RSC},
                          xp.options().dtype(at::kFloat));
    auto dw = at::empty({K, C, R, S},
                        xp.options().memory_format(at::MemoryFormat::ChannelsLast));
    DwKernel kern = nullptr;
    for (const DwVariant& v : kDwVariants)
      if (v.BMK == d.BMK && v.stride == d.stride && v.NT == d.NT)
        kern = v.kern;
    TORCH_CHECK(kern, "no dw_gemm_kernel for plan BMK=", d.BMK, " stride=",
                d.stride, " NT=", d.NT);
    hipLaunchKernelGGL(kern, dim3(d.rsc_tiles, d.grid_y, d.splits), dim3(256),
                       0, stream, (const bf16*)dyT.data_ptr(),
                       (const bf16*)xpT.data_ptr(),
                       stride == 2 ? (const bf16*)xpT2.data_ptr() : nullptr,
                       part.data_ptr<float>(), K, C, N, Hp, Wlane, S, M,
                       (int)RSC, d.mtiles_per_split, qshift, Q - 1, pshift,
                       P - 1);
    long long L = (long long)K * RSC;
    if (d.two_stage) {
      auto part2 = at::empty({8, L}, xp.options().dtype(at::kFloat));
      hipLaunchKernelGGL(colsum_stage_kernel,
                         dim3(grid_1d(L, 256, 512), 8), dim3(256), 0, stream,
                         part.data_ptr<float>(), d.splits / 8, L,
                         part2.data_ptr<float>());
      hipLaunchKernelGGL(colsum_to_bf16_kernel, dim3(grid_1d(L, 256)),
                         dim3(256), 0, stream, part2.data_ptr<float>(), 8, L,
                         (bf16*)dw.data_ptr());
    } else {
      hipLaunchKernelGGL(colsum_to_bf16_kernel, dim3(grid_1d(L, 256)),
                         dim3(256), 0, stream, part.data_ptr<float>(),
                         d.splits, L, (bf16*)dw.data_ptr());
    }
    return dw;
  }

  at::Tensor col;
  if (R == 1 && S == 1 && stride == 1) {
    col = xp.permute({0, 2, 3, 1}).reshape({M, C});  // NHWC view, no copy
  } else {
    col = at::empty({M, (long long)R * S * C},
                    xp.options().memory_format(at::MemoryFormat::Contiguous));
    auto stream = fedkit_stream();
    if (C % 8 == 0) {
      long long total = M * R * S * C / 8;
      hipLaunchKernelGGL(im2col_kernel<8>, dim3(grid_1d(total, 512)),
                         dim3(256), 0, stream, (const bf16*)xp.data_ptr(),
                         (bf16*)col.data_ptr(), N, xp.size(2), xp.size(3), C,
                         R, S, P, Q, (int)stride, (int)dil);
    } else {
      long long total = M * R * S * C;
      hipLaunchKernelGGL(im2col_kernel<1>, dim3(grid_1d(total, 512)),
                         dim3(256), 0, stream, (const bf16*)xp.data_ptr(),
                         (bf16*)col.data_ptr(), N, xp.size(2), xp.size(3), C,
                         R, S, P, Q, (int)stride, (int)dil);
    }
  }
  // dw = dy^T @ col is a tall-skinny reduction GEMM ([K<=512, RSC<=4608]
  // output, reduction dim up to 131072).  Tensile picks no split-K for that
  // shape, so split it ourselves: batch the reduction dim into chunks, bmm
  // into fp32 partials, sum — a plain library GEMM per chunk.
  auto dy2d = gy.permute({0, 2, 3, 1}).reshape({M, K});
  const int chunks = d.chunks;
  at::Tensor dw;
  if (chunks > 1) {
    auto dyb = dy2d.reshape({chunks, M / chunks, K});
    auto colb = col.reshape({chunks, M / chunks, RSC});
    auto partial = at::bmm(dyb.transpose(1, 2), colb);  // [chunks, K, Kg2]
    dw = partial.sum(0, false, at::kFloat).to(at::kBFloat16);
  } else {
    dw = at::matmul(dy2d.t(), col);
  }
  return dw.reshape({K, R, S, C}).permute({0, 3, 1, 2})
      .contiguous(at::MemoryFormat::ChannelsLast);
}

at::Tensor fedkit_conv2d_bwd_weight(const at::Tensor& gy, const at::Tensor& x,
                                    long stride, long padding, long R_in,
                                    long S_in, long dil) {
  at::Tensor xp = pad_nhwc(x, (int)padding);
  return fedkit_conv2d_bwd_weight_prepadded(gy, xp, stride, R_in, S_in, dil);
}
