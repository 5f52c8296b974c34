// Fused consensus penalty and ADMM update kernels (FedProx / consensus ADMM).
//
// The closure-side penalty of the reference (consensus_multi.py:209-218,
// fedprox_multi.py:183-190, plus the L1/L2 regulariser of
// federated_multi.py:183-187) is, per minibatch closure call,
//   y.(x-z) + (rho/2)||x-z||^2 + lambda1 ||x||_1 + lambda2 ||x||^2
// over the trainable block x.  As stock torch ops that is a cat of the
// block, ~10 elementwise/reduction launches forward and the autograd replay
// backward.  Here the forward is ONE streaming reduction that reads the
// parameter tensors in place through by-value segment tables (<= 48
// tensors per launch, csrc/multi_tensor.h) and the
// backward is ONE elementwise pass writing the closed-form gradient
//   go * (y + rho (x-z) + lambda1 sign(x) + 2 lambda2 x)
// in the same physical (storage) element order the packed z / y use.
//
// The aggregation side gets the same treatment: admm_dual_update fuses
// y += rho (x-z) with the primal-residual norm, bb_stats forms the six
// Barzilai-Borwein inner products in one pass over five vectors
// (bb_stats_round: for all local clients in one launch).
//
// Every reduction is deterministic: fixed grid (a function of the length
// only), per-workgroup partials in a slab, one finalize kernel that sums
// the slab in a fixed order.  No floating-point atomics — the bit-exact
// kill-and-resume and nccl==local tests run through penalty_fwd.
//
// Memory access: 16-byte loads/stores are used per pointer only when that
// pointer is 16-byte aligned (parameter tensors come from separate
// allocations, so their offsets into the flat vectors are arbitrary);
// otherwise that side falls back to four dword accesses.  Units that
// straddle a tensor boundary or the tail take a per-element scalar path.

#include "agg_common.h"
#include "multi_tensor.h"

#include <cmath>
#include <type_traits>

namespace {

using namespace fedkit_agg;
using fedkit_mt::DeviceGuard;
using fedkit_mt::for_each_unit;
using fedkit_mt::SegTable;

template <bool HZ, bool HY>
__device__ __forceinline__ float pen_term(float x, float z, float y,
                                          float hrho, float l1, float l2) {
  float s = l1 * fabsf(x) + l2 * x * x;
  if (HZ) {
    float dlt = x - z;
    s += hrho * dlt * dlt;
    if (HY) s += y * dlt;
  }
  return s;
}

template <bool HZ, bool HY>
__device__ __forceinline__ float pen_grad(float x, float z, float y,
                                          float rho, float l1, float l2x2,
                                          float go) {
  float sgn = (float)(x > 0.f) - (float)(x < 0.f);   // sign(0) = 0
  float g = l1 * sgn + l2x2 * x;
  if (HZ) {
    g += rho * (x - z);
    if (HY) g += y;
  }
  return go * g;
}

// part[blockIdx.x] = this workgroup's share of the penalty over the chunk.
// z / y already point at the chunk's slice of the flat vectors.
template <bool HZ, bool HY>
__global__ void __launch_bounds__(kBlock)
penalty_fwd_kernel(SegTable<1> d, const float* __restrict__ z,
                   const float* __restrict__ y, float hrho, float l1,
                   float l2, long long total, float* __restrict__ part) {
  __shared__ float red[4];
  float acc = 0.f;
  for_each_unit<4>(
      d, total,
      [&](int t, long long j, long long i0) {
        f4 xv = load4(d.at<const float>(0, t) + j);
        f4 zv = {}, yv = {};
        if (HZ) zv = load4(z + i0);
        if (HY) yv = load4(y + i0);
#pragma unroll
        for (int k = 0; k < 4; ++k)
          acc += pen_term<HZ, HY>(xv[k], zv[k], yv[k], hrho, l1, l2);
      },
      [&](int t, long long j, long long i) {
        acc += pen_term<HZ, HY>(d.at<const float>(0, t)[j], HZ ? z[i] : 0.f,
                                HY ? y[i] : 0.f, hrho, l1, l2);
      });
  float s = block_sum(acc, red);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// g[i] = go * dPenalty/dx_i over the chunk; g / z / y point at the chunk's
// slice of the flat vectors, go is a device scalar.
template <bool HZ, bool HY>
__global__ void __launch_bounds__(kBlock)
penalty_bwd_kernel(SegTable<1> d, const float* __restrict__ z,
                   const float* __restrict__ y, float rho, float l1,
                   float l2x2, const float* __restrict__ go_ptr,
                   long long total, float* __restrict__ g) {
  const float go = *go_ptr;
  for_each_unit<4>(
      d, total,
      [&](int t, long long j, long long i0) {
        f4 xv = load4(d.at<const float>(0, t) + j);
        f4 zv = {}, yv = {}, gv;
        if (HZ) zv = load4(z + i0);
        if (HY) yv = load4(y + i0);
#pragma unroll
        for (int k = 0; k < 4; ++k)
          gv[k] = pen_grad<HZ, HY>(xv[k], zv[k], yv[k], rho, l1, l2x2, go);
        store4(g + i0, gv);
      },
      [&](int t, long long j, long long i) {
        g[i] = pen_grad<HZ, HY>(d.at<const float>(0, t)[j], HZ ? z[i] : 0.f,
                                HY ? y[i] : 0.f, rho, l1, l2x2, go);
      });
}

// rho (x - z), rounded: it is added to y as torch's `y.add_(rho * (x - z))`
// adds it, not fused into the add, so that this kernel, aggregate_kernel
// and the torch sequence leave the same bits in y.
__device__ __forceinline__ float dual_step(float rho, float x, float z) {
#pragma clang fp contract(off)
  return rho * (x - z);
}

__device__ __forceinline__ float add_rounded(float a, float b) {
#pragma clang fp contract(off)
  return a + b;
}

// y += rho (x - z);  part[blockIdx.x] = partial sum of (rho (x - z))^2
FEDKIT_AGG_KERNEL __launch_bounds__(kBlock)
admm_dual_update_kernel(float* __restrict__ y, const float* __restrict__ x,
                        const float* __restrict__ z, float rho, long long n,
                        float* __restrict__ part) {
  __shared__ float red[4];
  float acc = 0.f;
  const long long units = (n + 3) >> 2;
  for (long long u = blockIdx.x * (long long)kBlock + threadIdx.x; u < units;
       u += (long long)gridDim.x * kBlock) {
    long long i0 = u << 2;
    if (i0 + 4 <= n) {
      f4 xv = load4(x + i0), zv = load4(z + i0), yv = load4(y + i0);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float yd = dual_step(rho, xv[k], zv[k]);
        yv[k] = add_rounded(yv[k], yd);
        acc += yd * yd;
      }
      store4(y + i0, yv);
    } else {
      for (long long i = i0; i < n; ++i) {
        float yd = dual_step(rho, x[i], z[i]);
        y[i] = add_rounded(y[i], yd);
        acc += yd * yd;
      }
    }
  }
  float s = block_sum(acc, red);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// One element's six products, each folded into its sum by one fused
// multiply-add.  The fma is written out: left to contraction, the compiler
// fused some of these and rounded the product of others, differently from
// one kernel to the next, and bb_stats_round_kernel's rows have to be
// bb_stats_kernel's bit for bit.
__device__ __forceinline__ void bb_accum(float* acc, float y, float yh,
                                         float x, float z, float x0) {
  float a = y - yh, b = x - z, dx = x - x0;
  acc[0] = __builtin_fmaf(a, a, acc[0]);
  acc[1] = __builtin_fmaf(a, b, acc[1]);
  acc[2] = __builtin_fmaf(b, b, acc[2]);
  acc[3] = __builtin_fmaf(a, dx, acc[3]);
  acc[4] = __builtin_fmaf(b, dx, acc[4]);
  acc[5] = __builtin_fmaf(dx, dx, acc[5]);
}

// part[blockIdx.x][0..5] = partial (a.a, a.b, b.b, a.dx, b.dx, dx.dx)
FEDKIT_AGG_KERNEL __launch_bounds__(kBlock)
bb_stats_kernel(const float* __restrict__ y, const float* __restrict__ yh,
                const float* __restrict__ x, const float* __restrict__ z,
                const float* __restrict__ x0, long long n,
                float* __restrict__ part) {
  __shared__ float red[4];
  float acc[6] = {};
  const long long units = (n + 3) >> 2;
  for (long long u = blockIdx.x * (long long)kBlock + threadIdx.x; u < units;
       u += (long long)gridDim.x * kBlock) {
    long long i0 = u << 2;
    if (i0 + 4 <= n) {
      f4 yv = load4(y + i0), hv = load4(yh + i0), xv = load4(x + i0),
         zv = load4(z + i0), pv = load4(x0 + i0);
#pragma unroll
      for (int k = 0; k < 4; ++k)
        bb_accum(acc, yv[k], hv[k], xv[k], zv[k], pv[k]);
    } else {
      for (long long i = i0; i < n; ++i)
        bb_accum(acc, y[i], yh[i], x[i], z[i], x0[i]);
    }
  }
#pragma unroll
  for (int c = 0; c < 6; ++c) {
    float s = block_sum(acc[c], red);
    if (threadIdx.x == 0) part[(long long)blockIdx.x * 6 + c] = s;
  }
}

// ---- BB statistics of all K local clients in one launch ----
//
// bb_stats_kernel once per client reads z K times and costs K launches and K
// host reads.  Here blockIdx.y picks a bucket of kBBBucket clients out of a
// table in the kernarg segment; a thread loads its z unit once and serves
// the bucket's clients from it: four 16-byte loads and six accumulators per
// client.  z is read ceil(K / kBBBucket) times.
//
// Row k is bitwise bb_stats of client k, which keeps the BB rho chain (and
// so z and y) the same whichever path formed the statistics: per client this
// is bb_stats_kernel's partition (same grid over the units, same unit of a
// thread, same in-loop tail), the same bb_accum with its explicit fmas, the
// same block_sum, and a finalize whose row order depends on the number of
// workgroups only.
//
// Bucket size, from the compiler's kernel-resource-usage report for gfx950
// (256 threads, 16 B LDS, no scratch in any of them):
//   clients/bucket  VGPRs  waves/SIMD  z reads at K = 10
//         2           43       7              5
//         4           57       7              3
//         8           83       5              2
// 4 is used: it costs no occupancy against 2 and reads z 3 times at the
// drivers' default K = 10 where bb_stats read it 10 times.  8 saves one more
// read of z there, but gives up two waves per SIMD and leaves 6 of its 16
// client slots idle.  (bb_stats_kernel: 35 VGPRs, 8 waves.)
constexpr int kBBBucket = 4;

struct BBTable {                  // by value in the kernarg segment, 1 KB
  const float* y[kMaxClients];
  const float* yh[kMaxClients];
  const float* x[kMaxClients];
  const float* x0[kMaxClients];
};

// part[blockIdx.x][k][0..5] = workgroup partial of client k's six products
FEDKIT_AGG_KERNEL __launch_bounds__(kBlock)
bb_stats_round_kernel(BBTable t, const float* __restrict__ z, int K,
                      long long n, float* __restrict__ part) {
  __shared__ float red[4];
  const int k0 = blockIdx.y * kBBBucket;   // wave-uniform: scalar table reads
  const float *py[kBBBucket], *ph[kBBBucket], *px[kBBBucket], *pp[kBBBucket];
#pragma unroll
  for (int j = 0; j < kBBBucket; ++j) {
    const int k = min(k0 + j, K - 1);      // slots past K are never read
    py[j] = t.y[k]; ph[j] = t.yh[k]; px[j] = t.x[k]; pp[j] = t.x0[k];
  }
  float acc[kBBBucket][6] = {};
  const long long units = (n + 3) >> 2;
  for (long long u = blockIdx.x * (long long)kBlock + threadIdx.x; u < units;
       u += (long long)gridDim.x * kBlock) {
    long long i0 = u << 2;
    if (i0 + 4 <= n) {
      const f4 zv = load4(z + i0);
#pragma unroll
      for (int j = 0; j < kBBBucket; ++j)
        if (k0 + j < K) {
          f4 yv = load4(py[j] + i0), hv = load4(ph[j] + i0),
             xv = load4(px[j] + i0), pv = load4(pp[j] + i0);
#pragma unroll
          for (int e = 0; e < 4; ++e)
            bb_accum(acc[j], yv[e], hv[e], xv[e], zv[e], pv[e]);
        }
    } else {
      for (long long i = i0; i < n; ++i) {
        const float zs = z[i];
#pragma unroll
        for (int j = 0; j < kBBBucket; ++j)
          if (k0 + j < K)
            bb_accum(acc[j], py[j][i], ph[j][i], px[j][i], zs, pp[j][i]);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < kBBBucket; ++j)
    if (k0 + j < K) {
      float* row = part + ((long long)blockIdx.x * K + k0 + j) * 6;
#pragma unroll
      for (int c = 0; c < 6; ++c) {
        float s = block_sum(acc[j][c], red);
        if (threadIdx.x == 0) row[c] = s;
      }
    }
}

// ---- aggregation round: z-update, dual update and residuals in one pass ----
//
// One LocalComm round over K client vectors x_k (and duals y_k for ADMM):
//   fedavg   znew = (0 + x_0 + ... + x_{K-1}) * inv          inv = 1/K
//   fedprox  same znew;  r_k = sum (rho (x_k - znew))^2
//   admm     znew = (0 + c_0 + ...) * inv, c_k = y_k + rho x_k, inv = 1/(K rho)
//            y_k += rho (x_k - znew);  r_k as above
// and r_z = sum (z - znew)^2 in every mode.  Every operand is read once and
// znew / y_k are written once: a thread's unit (4 consecutive floats) keeps
// its K client values on chip between the sum and the residual / dual step.
//
// Bit-compatibility with the torch sequence the strategies ran before (K
// in-place adds into a zero vector, `/= scalar`, `rho * (x - znew)`, `add_`):
// contraction is off in this code, every product is rounded before it is
// added, the sum starts from +0.0f and runs in client order, and the
// division is a multiply by a reciprocal formed on the host.  Found on
// gfx950: torch's GPU division of a float tensor by a host scalar s is
// `t * inv` bit for bit, not the correctly rounded quotient (which differs
// in 20% of the elements at s = 10 and 33% at s = 3), and inv is
// (float)(1.0 / s) with s and the division in double: 1.0f / (float)s is a
// different float at, e.g., s = 17 * 0.1 and misses torch's znew by 1-2 ulp.
//
// Variants: the held values live in registers up to K = 16 in both modes,
// template-unrolled in buckets of 4 clients (K is a run-time argument; a
// bucket costs at most 12 (fedprox) or 24 (admm) VGPRs it does not use).
// Above 16 clients a thread parks them in a private LDS column
// ([rows][BLOCK] float4, 128 KB: one workgroup per CU); a thread reads back
// only what it wrote, so the slab needs no barrier, and consecutive lanes
// touch consecutive 16-byte slots, so it has no bank conflicts.  The
// cut-over is at 16 because registers are the better store up to there: the
// largest register variant, 16 clients with duals, still runs 2 waves per
// SIMD (8 per CU, each with 33 16-byte loads in flight per lane) against the
// slab's 4 (fedprox, 256 threads) or 2 (admm, 128 threads) waves per CU,
// and the drivers' default K = 10 runs 5 (fedprox) or 3 (admm) waves per
// SIMD.  Past 16 the admm registers (2 x 4 x K) would drop it to one wave.
// The per-variant figures are in the table at fedkit_aggregate_round.
// FedAvg forms no per-client residual and holds nothing.  The n % 4 tail
// elements are done after the unit loop, one thread each, so the loop body
// has no tail branch.
//
// BB carry (admm only): adaptive rho also wants, from the operands this
// kernel already holds on chip,
//   x0_k = x_k        yhat0_k = y_k + rho_used[k] (x_k - z)
// with y_k before the dual step and the old z.  A compile-time CARRY adds
// them as one (kCarryX0, round 0) or two (kCarryFull) more 16-byte stores per
// client and no load.  rho_used is the rho the BB chain had at client k's
// turn; it travels by value and is indexed by the unrolled client index
// only, so it stays in scalar registers.  Without carry the kernel takes an
// empty argument in the table's place and is the code it was.

constexpr int kAggRegMax = 16;   // clients held in registers; above: LDS
enum { kFedAvg = 0, kFedProx = 1, kAdmm = 2 };
// ints, not an unnamed enum: CARRY is part of aggregate_kernel's signature
// (CarryArg<CARRY>), and an unnamed type in a kernel's mangled name is
// numbered differently by the host and the device compilation
constexpr int kCarryNone = 0, kCarryX0 = 1, kCarryFull = 2;

struct CarryTable {               // by value in the kernarg segment, 640 B
  float* x0[kMaxClients];
  float* yh[kMaxClients];
  float rho_used[kMaxClients];
};
struct NoCarry {};
template <int CARRY>
using CarryArg = std::conditional_t<CARRY == kCarryNone, NoCarry, CarryTable>;

// A unit of 4 floats at i0; lanes at or past n read as 0 and are not stored.
// Zero lanes add exact zeros to every sum below.
__device__ __forceinline__ f4 load_unit(const float* p, long long i0,
                                        long long n) {
  if (i0 + 4 <= n) return load4(p + i0);
  f4 v = {};
#pragma unroll
  for (int e = 0; e < 4; ++e)
    if (i0 + e < n) v[e] = p[i0 + e];
  return v;
}

__device__ __forceinline__ void store_unit(float* p, long long i0, long long n,
                                           f4 v) {
  if (i0 + 4 <= n) {
    store4(p + i0, v);
    return;
  }
#pragma unroll
  for (int e = 0; e < 4; ++e)
    if (i0 + e < n) p[i0 + e] = v[e];
}

// znew = (0 + x_0 + ...) * inv;  part[blockIdx.x] = partial sum (z - znew)^2
FEDKIT_AGG_KERNEL __launch_bounds__(kBlock)
aggregate_fedavg_kernel(ClientTable t, const float* __restrict__ z,
                        float* __restrict__ znew, float inv, int K,
                        long long n, float* __restrict__ part) {
#pragma clang fp contract(off)
  __shared__ float red[4];
  float acc = 0.f;
  const long long units = (n + 3) >> 2;
  for (long long u = blockIdx.x * (long long)kBlock + threadIdx.x; u < units;
       u += (long long)gridDim.x * kBlock) {
    const long long i0 = u << 2;
    f4 s = {};
#pragma unroll 4
    for (int k = 0; k < K; ++k) s += load_unit(t.x[k], i0, n);
    f4 zn = s * inv;
    f4 d = load_unit(z, i0, n) - zn;
    store_unit(znew, i0, n, zn);
    acc += d[0] * d[0];
    acc += d[1] * d[1];
    acc += d[2] * d[2];
    acc += d[3] * d[3];
  }
  float r = block_sum(acc, red);
  if (threadIdx.x == 0) part[blockIdx.x] = r;
}

// FedProx / ADMM round for K <= KL clients.  LDS = false: held values in
// registers (hx, hy).  LDS = true: in the thread's column of `slab`.
// part[blockIdx.x][0] = partial sum (z - znew)^2, [1 + k] = partial r_k.
// CARRY: also write cr.x0[k] (kCarryX0) and cr.yh[k] (kCarryFull).
template <int MODE, int KL, bool LDS, int BLOCK, int CARRY>
FEDKIT_AGG_KERNEL __launch_bounds__(BLOCK)
aggregate_kernel(ClientTable t, const float* __restrict__ z,
                 float* __restrict__ znew, float rho, float inv, int K,
                 long long n, float* __restrict__ part, CarryArg<CARRY> cr) {
#pragma clang fp contract(off)
  constexpr bool DUAL = MODE == kAdmm;
  static_assert(DUAL || CARRY == kCarryNone, "the BB carry is an admm step");
  constexpr int ROWS = DUAL ? 2 * KL : KL;
  __shared__ f4 slab[LDS ? ROWS * BLOCK : 1];
  __shared__ float red[4];
  f4 hx[LDS ? 1 : KL], hy[(LDS || !DUAL) ? 1 : KL];
  const int tid = threadIdx.x;
  // slot of client k in this thread's slab column: x rows, then y rows
  const int col = tid;
#define AGG_PUT(regs, row, k, v)                       \
  do {                                                 \
    if constexpr (LDS) slab[((row) + (k)) * BLOCK + col] = (v); \
    else regs[k] = (v);                                \
  } while (0)
#define AGG_GET(regs, row, k) \
  (LDS ? slab[((row) + (k)) * BLOCK + col] : regs[LDS ? 0 : (k)])
  float accz = 0.f, acck[KL] = {};
  const long long units = n >> 2;   // whole units; the tail follows the loop
  for (long long u = blockIdx.x * (long long)BLOCK + tid; u < units;
       u += (long long)gridDim.x * BLOCK) {
    const long long i0 = u << 2;
    // Slab variant with carry: 128 pointers and 32 rho values are more than
    // the SGPR file; held live across this loop they made the compiler
    // reserve a private segment.  An offset it cannot see through has it
    // read the carry table's entries per unit instead (scalar loads that
    // hit the scalar cache), and no variant has a private segment.
    int ko = 0;
    if constexpr (LDS && CARRY != kCarryNone) asm volatile("" : "+s"(ko));
    // all loads of the unit are issued before the first use
#pragma unroll
    for (int k = 0; k < KL; ++k)
      if (k < K) {
        AGG_PUT(hx, 0, k, load4(t.x[k] + i0));
        if constexpr (DUAL) AGG_PUT(hy, KL, k, load4(t.y[k] + i0));
      }
    const f4 zv = load4(z + i0);
    f4 s = {};
#pragma unroll
    for (int k = 0; k < KL; ++k)
      if (k < K) {
        f4 c = AGG_GET(hx, 0, k);
        if constexpr (DUAL) c = AGG_GET(hy, KL, k) + rho * c;
        s += c;
      }
    const f4 zn = s * inv;
    store4(znew + i0, zn);
    const f4 d = zv - zn;
    accz += d[0] * d[0];
    accz += d[1] * d[1];
    accz += d[2] * d[2];
    accz += d[3] * d[3];
#pragma unroll
    for (int k = 0; k < KL; ++k)
      if (k < K) {
        const f4 yd = rho * (AGG_GET(hx, 0, k) - zn);
        if constexpr (CARRY != kCarryNone)
          store4(cr.x0[k + ko] + i0, AGG_GET(hx, 0, k));
        if constexpr (CARRY == kCarryFull)
          store4(cr.yh[k + ko] + i0,
                 AGG_GET(hy, KL, k) +
                     cr.rho_used[k + ko] * (AGG_GET(hx, 0, k) - zv));
        if constexpr (DUAL) store4(t.y[k] + i0, AGG_GET(hy, KL, k) + yd);
        acck[k] += yd[0] * yd[0];
        acck[k] += yd[1] * yd[1];
        acck[k] += yd[2] * yd[2];
        acck[k] += yd[3] * yd[3];
      }
  }
  // the n % 4 tail elements: one thread each, same arithmetic per element
  const long long it = (units << 2) + tid;
  if (blockIdx.x == 0 && it < n) {
    float xs[KL], s = 0.f;
#pragma unroll
    for (int k = 0; k < KL; ++k)
      if (k < K) {
        xs[k] = t.x[k][it];
        s += DUAL ? t.y[k][it] + rho * xs[k] : xs[k];
      }
    const float zo = z[it], zn = s * inv, d = zo - zn;
    znew[it] = zn;
    accz += d * d;
#pragma unroll
    for (int k = 0; k < KL; ++k)
      if (k < K) {
        const float yd = rho * (xs[k] - zn);
        if constexpr (CARRY != kCarryNone) cr.x0[k][it] = xs[k];
        if constexpr (CARRY == kCarryFull)
          cr.yh[k][it] = t.y[k][it] + cr.rho_used[k] * (xs[k] - zo);
        if constexpr (DUAL) t.y[k][it] += yd;
        acck[k] += yd * yd;
      }
  }
  float* row = part + (long long)blockIdx.x * (1 + K);
  float r = block_sum<BLOCK / kWave>(accz, red);
  if (tid == 0) row[0] = r;
#pragma unroll
  for (int k = 0; k < KL; ++k)
    if (k < K) {
      r = block_sum<BLOCK / kWave>(acck[k], red);
      if (tid == 0) row[1 + k] = r;
    }
#undef AGG_PUT
#undef AGG_GET
}

struct AggArgs {                  // what every round variant is launched with
  ClientTable t;
  const float* z;
  float* znew;
  float rho, inv;
  int K;
  long long n;
  int nb;
  float* part;
  hipStream_t stream;
};

template <int MODE, int KL, bool LDS, int BLOCK, int CARRY>
void launch_aggregate(const AggArgs& a, const CarryArg<CARRY>& cr) {
  hipLaunchKernelGGL((aggregate_kernel<MODE, KL, LDS, BLOCK, CARRY>),
                     dim3(a.nb), dim3(BLOCK), 0, a.stream, a.t, a.z, a.znew,
                     a.rho, a.inv, a.K, a.n, a.part, cr);
}

// the register variant that fits K, or the LDS slab above kAggRegMax
template <int MODE, int CARRY>
void launch_round(const AggArgs& a, const CarryArg<CARRY>& cr) {
  constexpr int kSlabBlock = MODE == kAdmm ? 128 : kBlock;
  if (a.K <= 4) launch_aggregate<MODE, 4, false, kBlock, CARRY>(a, cr);
  else if (a.K <= 8) launch_aggregate<MODE, 8, false, kBlock, CARRY>(a, cr);
  else if (a.K <= 12) launch_aggregate<MODE, 12, false, kBlock, CARRY>(a, cr);
  else if (a.K <= kAggRegMax)
    launch_aggregate<MODE, 16, false, kBlock, CARRY>(a, cr);
  else launch_aggregate<MODE, 32, true, kSlabBlock, CARRY>(a, cr);
}

// [p, p + numel) of two operands intersect
bool overlaps(const at::Tensor& a, const at::Tensor& b) {
  const char* a0 = static_cast<const char*>(a.data_ptr());
  const char* b0 = static_cast<const char*>(b.data_ptr());
  return a0 < b0 + b.nbytes() && b0 < a0 + a.nbytes();
}

const float* flat_ptr(const c10::optional<at::Tensor>& v, long long n,
                      const at::Tensor& like, const char* name) {
  if (!v.has_value()) return nullptr;
  fedkit_mt::check_flat("consensus penalty", name, *v, like, n);
  return v->data_ptr<float>();
}

void check_vec(const at::Tensor& v, const at::Tensor& like, const char* op) {
  fedkit_mt::check_flat(op, "every operand", v, like, like.numel());
}

}  // namespace

// 0-dim device fp32: [y.(x-z)] + (rho/2)||x-z||^2 + l1 ||x||_1 + l2 ||x||^2
at::Tensor fedkit_penalty_fwd(std::vector<at::Tensor> params,
                              c10::optional<at::Tensor> z,
                              c10::optional<at::Tensor> y, double rho,
                              double lambda1, double lambda2) {
  TORCH_CHECK(z.has_value() || !y.has_value(),
              "consensus penalty: y needs z");
  const auto cs = fedkit_mt::build_chunks<1>("consensus penalty", {&params},
                                             {at::kFloat});
  const auto& chunks = cs.chunks;
  const long long n = cs.total;
  const DeviceGuard guard(params[0].device());
  const float* zp = flat_ptr(z, n, params[0], "z");
  const float* yp = flat_ptr(y, n, params[0], "y");
  auto opts = params[0].options();
  if (chunks.empty()) return at::zeros({}, opts);
  auto out = at::empty({1}, opts);
  auto stream = fedkit_stream();
  auto part = at::empty({(long long)chunks.size() * kRedGrid}, opts);
  float* pp = part.data_ptr<float>();
  const float hrho = 0.5f * (float)rho, l1 = (float)lambda1,
              l2 = (float)lambda2;
  int np = 0;
  for (const auto& c : chunks) {
    int nb = grid_1d((c.total + 3) >> 2, kBlock, kRedGrid);
    if (yp) {
      hipLaunchKernelGGL((penalty_fwd_kernel<true, true>), dim3(nb),
                         dim3(kBlock), 0, stream, c.d, zp + c.base,
                         yp + c.base, hrho, l1, l2, c.total, pp + np);
    } else if (zp) {
      hipLaunchKernelGGL((penalty_fwd_kernel<true, false>), dim3(nb),
                         dim3(kBlock), 0, stream, c.d, zp + c.base,
                         (const float*)nullptr, hrho, l1, l2, c.total,
                         pp + np);
    } else {
      hipLaunchKernelGGL((penalty_fwd_kernel<false, false>), dim3(nb),
                         dim3(kBlock), 0, stream, c.d, (const float*)nullptr,
                         (const float*)nullptr, hrho, l1, l2, c.total,
                         pp + np);
    }
    np += nb;
  }
  fedkit_colsum_finalize(pp, np, 1, out.data_ptr<float>(), stream);
  return out.reshape({});
}

// flat fp32 [N] gradient in physical order, scaled by the device scalar go
at::Tensor fedkit_penalty_bwd(std::vector<at::Tensor> params,
                              c10::optional<at::Tensor> z,
                              c10::optional<at::Tensor> y, double rho,
                              double lambda1, double lambda2,
                              const at::Tensor& grad_out) {
  TORCH_CHECK(z.has_value() || !y.has_value(),
              "consensus penalty: y needs z");
  const auto cs = fedkit_mt::build_chunks<1>("consensus penalty", {&params},
                                             {at::kFloat});
  const auto& chunks = cs.chunks;
  const long long n = cs.total;
  fedkit_mt::check_flat("consensus penalty", "grad_out", grad_out, params[0],
                        1);
  const DeviceGuard guard(params[0].device());
  const float* zp = flat_ptr(z, n, params[0], "z");
  const float* yp = flat_ptr(y, n, params[0], "y");
  auto g = at::empty({n}, params[0].options());
  float* gp = g.data_ptr<float>();
  const float* go = grad_out.data_ptr<float>();
  auto stream = fedkit_stream();
  const float r = (float)rho, l1 = (float)lambda1,
              l2x2 = 2.f * (float)lambda2;
  for (const auto& c : chunks) {
    int nb = grid_1d((c.total + 3) >> 2, kBlock);
    if (yp) {
      hipLaunchKernelGGL((penalty_bwd_kernel<true, true>), dim3(nb),
                         dim3(kBlock), 0, stream, c.d, zp + c.base,
                         yp + c.base, r, l1, l2x2, go, c.total, gp + c.base);
    } else if (zp) {
      hipLaunchKernelGGL((penalty_bwd_kernel<true, false>), dim3(nb),
                         dim3(kBlock), 0, stream, c.d, zp + c.base,
                         (const float*)nullptr, r, l1, l2x2, go, c.total,
                         gp + c.base);
    } else {
      hipLaunchKernelGGL((penalty_bwd_kernel<false, false>), dim3(nb),
                         dim3(kBlock), 0, stream, c.d, (const float*)nullptr,
                         (const float*)nullptr, r, l1, l2x2, go, c.total,
                         gp + c.base);
    }
  }
  return g;
}

// y += rho (x - z) in place; returns the device scalar sum (rho (x-z))^2
at::Tensor fedkit_admm_dual_update(at::Tensor y, const at::Tensor& x,
                                   const at::Tensor& z, double rho) {
  check_vec(y, y, "admm_dual_update");
  check_vec(x, y, "admm_dual_update");
  check_vec(z, y, "admm_dual_update");
  const DeviceGuard guard(y.device());
  long long n = y.numel();
  if (n == 0) return at::zeros({}, y.options());
  auto out = at::empty({1}, y.options());
  auto stream = fedkit_stream();
  int nb = grid_1d((n + 3) >> 2, kBlock, kRedGrid);
  auto part = at::empty({nb}, y.options());
  hipLaunchKernelGGL(admm_dual_update_kernel, dim3(nb), dim3(kBlock), 0,
                     stream, y.data_ptr<float>(), x.data_ptr<float>(),
                     z.data_ptr<float>(), (float)rho, n,
                     part.data_ptr<float>());
  fedkit_colsum_finalize(part.data_ptr<float>(), nb, 1,
                         out.data_ptr<float>(), stream);
  return out.reshape({});
}

// device fp32 [6] = (a.a, a.b, b.b, a.dx, b.dx, dx.dx) with a = y - yhat0,
// b = x - z, dx = x - x0
at::Tensor fedkit_bb_stats(const at::Tensor& y, const at::Tensor& yhat0,
                           const at::Tensor& x, const at::Tensor& z,
                           const at::Tensor& x0) {
  check_vec(y, y, "bb_stats");
  check_vec(yhat0, y, "bb_stats");
  check_vec(x, y, "bb_stats");
  check_vec(z, y, "bb_stats");
  check_vec(x0, y, "bb_stats");
  const DeviceGuard guard(y.device());
  long long n = y.numel();
  if (n == 0) return at::zeros({6}, y.options());
  auto out = at::empty({6}, y.options());
  auto stream = fedkit_stream();
  int nb = grid_1d((n + 3) >> 2, kBlock, kRedGrid);
  auto part = at::empty({nb, 6}, y.options());
  hipLaunchKernelGGL(bb_stats_kernel, dim3(nb), dim3(kBlock), 0, stream,
                     y.data_ptr<float>(), yhat0.data_ptr<float>(),
                     x.data_ptr<float>(), z.data_ptr<float>(),
                     x0.data_ptr<float>(), n, part.data_ptr<float>());
  fedkit_colsum_finalize(part.data_ptr<float>(), nb, 6,
                         out.data_ptr<float>(), stream);
  return out;
}

// device fp32 [K, 6]: row k = fedkit_bb_stats(ys[k], yhat0s[k], xs[k], z,
// x0s[k]) bit for bit, for all K <= 32 clients in one launch + the finalize
at::Tensor fedkit_bb_stats_round(std::vector<at::Tensor> ys,
                                 std::vector<at::Tensor> yhat0s,
                                 std::vector<at::Tensor> xs,
                                 const at::Tensor& z,
                                 std::vector<at::Tensor> x0s) {
  const char* op = "bb_stats_round";
  const int K = (int)xs.size();
  TORCH_CHECK(xs.size() >= 1 && xs.size() <= (size_t)kMaxClients, op,
              ": 1..", kMaxClients, " clients, got ", xs.size());
  TORCH_CHECK(ys.size() == xs.size() && yhat0s.size() == xs.size() &&
              x0s.size() == xs.size(), op, ": ", xs.size(), " clients but ",
              ys.size(), " y, ", yhat0s.size(), " yhat0, ", x0s.size(),
              " x0");
  const long long n = z.numel();
  fedkit_mt::check_flat(op, "z", z, z, n);
  BBTable t = {};
  for (int k = 0; k < K; ++k) {
    fedkit_mt::check_flat(op, "every y_k", ys[k], z, n);
    fedkit_mt::check_flat(op, "every yhat0_k", yhat0s[k], z, n);
    fedkit_mt::check_flat(op, "every x_k", xs[k], z, n);
    fedkit_mt::check_flat(op, "every x0_k", x0s[k], z, n);
    t.y[k] = ys[k].data_ptr<float>();
    t.yh[k] = yhat0s[k].data_ptr<float>();
    t.x[k] = xs[k].data_ptr<float>();
    t.x0[k] = x0s[k].data_ptr<float>();
  }
  const DeviceGuard guard(z.device());
  if (n == 0) return at::zeros({K, 6}, z.options());
  auto out = at::empty({K, 6}, z.options());
  auto stream = fedkit_stream();
  // bb_stats' grid: the partition of a client's sum must not depend on K
  const int nb = grid_1d((n + 3) >> 2, kBlock, kRedGrid);
  auto part = at::empty({nb, 6 * K}, z.options());
  hipLaunchKernelGGL(bb_stats_round_kernel,
                     dim3(nb, (K + kBBBucket - 1) / kBBBucket), dim3(kBlock),
                     0, stream, t, z.data_ptr<float>(), K, n,
                     part.data_ptr<float>());
  fedkit_colsum_finalize(part.data_ptr<float>(), nb, 6 * K,
                         out.data_ptr<float>(), stream);
  return out;
}

// One LocalComm aggregation round (see aggregate_kernel).  Returns
// {znew, res}: znew a fresh fp32 [N]; res device fp32, res[0] =
// sum (z - znew)^2 and, in fedprox / admm mode, res[1 + k] =
// sum (rho (x_k - znew))^2.  admm updates ys[k] += rho (xs[k] - znew) in
// place.  mode: 0 fedavg, 1 fedprox, 2 admm.
//
// BB carry (admm): with x0s the round also writes x0s[k] = xs[k]; with
// x0s, yhat0s and rho_used (K finite values) also yhat0s[k] = ys[k] +
// rho_used[k] (xs[k] - z), from ys[k] as it came in and the old z.  The
// outputs may not overlap any operand or each other.
//
// Compiler's kernel-resource-usage figures for gfx950 (no variant uses
// scratch; 512 VGPRs per SIMD lane):
//   variant             threads  VGPRs  LDS bytes  waves/SIMD
//   fedavg, any K         256      38        16        8
//   fedprox K <=  4 reg   256      40        16        8
//   fedprox K <=  8 reg   256      60        16        8
//   fedprox K <= 12 reg   256      81        16        5
//   fedprox K <= 16 reg   256     104        16        4
//   fedprox K <= 32 LDS   256     122    131088        1 (one workgroup/CU)
//   admm    K <=  4 reg   256      63        16        8
//   admm    K <=  8 reg   256     100        16        4
//   admm    K <= 12 reg   256     136        16        3
//   admm    K <= 16 reg   256     188        16        2
//   admm    K <= 32 LDS   128     138    131088        2 waves per CU
// and of the admm variants with the BB carry (VGPRs x0-only / full; LDS
// bytes and waves as in the row above them, except K <= 4 full: 7 waves):
//   admm    K <=  4 reg   256    63 /  64
//   admm    K <=  8 reg   256   107 / 108
//   admm    K <= 12 reg   256   137 / 138
//   admm    K <= 16 reg   256   188 / 190
//   admm    K <= 32 LDS   128   137 / 141
std::vector<at::Tensor> fedkit_aggregate_round(
    std::vector<at::Tensor> xs, const at::Tensor& z,
    std::vector<at::Tensor> ys, double rho, int64_t mode,
    std::vector<at::Tensor> x0s, std::vector<at::Tensor> yhat0s,
    std::vector<double> rho_used) {
  const char* op = "aggregate_round";
  TORCH_CHECK(mode == kFedAvg || mode == kFedProx || mode == kAdmm, op,
              ": unknown mode ", mode);
  const int K = (int)xs.size();
  TORCH_CHECK(xs.size() >= 1 && xs.size() <= (size_t)kMaxClients, op,
              ": 1..", kMaxClients, " clients, got ", xs.size());
  if (mode == kAdmm) {
    TORCH_CHECK(ys.size() == xs.size(), op, ": ", ys.size(), " duals for ",
                xs.size(), " clients");
    TORCH_CHECK(rho > 0.0 && std::isfinite(rho), op,
                ": admm needs a finite rho > 0, got ", rho);
  } else {
    TORCH_CHECK(ys.empty(), op, ": duals are an admm operand");
    TORCH_CHECK(mode == kFedAvg || std::isfinite(rho), op,
                ": fedprox needs a finite rho, got ", rho);
    TORCH_CHECK(x0s.empty() && yhat0s.empty() && rho_used.empty(), op,
                ": the BB carry (x0s, yhat0s, rho_used) is an admm operand");
  }
  const int carry = !yhat0s.empty() || !rho_used.empty() ? kCarryFull
                    : !x0s.empty()                       ? kCarryX0
                                                         : kCarryNone;
  if (carry != kCarryNone)
    TORCH_CHECK(x0s.size() == xs.size(), op, ": ", x0s.size(), " x0 for ",
                xs.size(), " clients");
  if (carry == kCarryFull) {
    TORCH_CHECK(yhat0s.size() == xs.size() && rho_used.size() == xs.size(),
                op, ": the full carry needs ", xs.size(),
                " yhat0 and rho_used, got ", yhat0s.size(), " and ",
                rho_used.size());
    for (double r : rho_used)
      TORCH_CHECK(std::isfinite(r), op, ": rho_used must be finite, got ", r);
  }
  const long long n = z.numel();
  fedkit_mt::check_flat(op, "z", z, z, n);
  ClientTable t = {};
  for (int k = 0; k < K; ++k) {
    fedkit_mt::check_flat(op, "every x_k", xs[k], z, n);
    t.x[k] = xs[k].data_ptr<float>();
  }
  for (size_t k = 0; k < ys.size(); ++k) {
    fedkit_mt::check_flat(op, "every y_k", ys[k], z, n);
    t.y[k] = ys[k].data_ptr<float>();
    // y_k is written while the other operands are still being read
    TORCH_CHECK(n == 0 || t.y[k] != z.data_ptr<float>(), op,
                ": y_k aliases z");
    for (int j = 0; j < K; ++j)
      TORCH_CHECK(n == 0 || (t.y[k] != t.x[j] && (j >= (int)k ||
                                                  t.y[k] != t.y[j])),
                  op, ": y_", k, " aliases another operand");
  }
  CarryTable cr = {};
  std::vector<const at::Tensor*> outs;   // carry outputs checked so far
  for (size_t i = 0; i < x0s.size() + yhat0s.size(); ++i) {
    const bool is_x0 = i < x0s.size();
    const size_t k = is_x0 ? i : i - x0s.size();
    const at::Tensor& o = is_x0 ? x0s[k] : yhat0s[k];
    fedkit_mt::check_flat(op, is_x0 ? "every x0_k" : "every yhat0_k", o, z, n);
    (is_x0 ? cr.x0 : cr.yh)[k] = o.data_ptr<float>();
    // written while every operand is still being read
    bool clash = n > 0 && overlaps(o, z);
    for (int j = 0; j < K && n > 0; ++j)
      clash = clash || overlaps(o, xs[j]) || overlaps(o, ys[j]);
    for (const at::Tensor* p : outs) clash = clash || (n > 0 && overlaps(o, *p));
    TORCH_CHECK(!clash, op, ": ", is_x0 ? "x0_" : "yhat0_", k,
                " overlaps another operand");
    outs.push_back(&o);
  }
  for (size_t k = 0; k < rho_used.size(); ++k)
    cr.rho_used[k] = (float)rho_used[k];
  const DeviceGuard guard(z.device());
  const int cols = mode == kFedAvg ? 1 : 1 + K;
  auto znew = at::empty({n}, z.options());
  if (n == 0) return {znew, at::zeros({cols}, z.options())};
  auto res = at::empty({cols}, z.options());
  auto stream = fedkit_stream();
  const bool lds = mode != kFedAvg && K > kAggRegMax;
  const int block = (lds && mode == kAdmm) ? 128 : kBlock;
  const int nb = grid_1d((n + 3) >> 2, block, kRedGrid);
  auto part = at::empty({nb, cols}, z.options());
  float* pp = part.data_ptr<float>();
  // the reciprocal torch forms for `znew /= K` and `znew /= (K * rho)`:
  // in double from the double scalar, then rounded to fp32
  const float inv =
      (float)(1.0 / (mode == kAdmm ? (double)K * rho : (double)K));
  const AggArgs a = {t, z.data_ptr<float>(), znew.data_ptr<float>(),
                     (float)rho, inv, K, n, nb, pp, stream};
  if (mode == kFedAvg) {
    hipLaunchKernelGGL(aggregate_fedavg_kernel, dim3(nb), dim3(kBlock), 0,
                       stream, t, a.z, a.znew, inv, K, n, pp);
  } else if (mode == kFedProx) {
    launch_round<kFedProx, kCarryNone>(a, NoCarry{});
  } else if (carry == kCarryNone) {
    launch_round<kAdmm, kCarryNone>(a, NoCarry{});
  } else if (carry == kCarryX0) {
    launch_round<kAdmm, kCarryX0>(a, cr);
  } else {
    launch_round<kAdmm, kCarryFull>(a, cr);
  }
  fedkit_colsum_finalize(pp, nb, cols, res.data_ptr<float>(), stream);
  return {znew, res};
}
