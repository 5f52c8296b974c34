// bf16 MFMA GEMM kernels for the fully connected layers above FedLinear's
// 256k-weight gate (Net1 fc1 [512,1600], Net2 fc4 [1024,512]); linear.hip
// keeps the latency-bound heads below it.
//
// One kernel template serves the three passes.  It computes
//   out[i][j] = sum_r A(i, r) B(j, r),        i < I, j < J, r < R
// with v_mfma_f32_16x16x32_bf16 and fp32 accumulation, and each operand is
// either reduction-contiguous in memory ([I][R]) or reduction-major ([R][I]):
//   forward     y  = x w^T + b   A = x  [M][K]          B = w [N][K]
//   bwd-data    gx = gy w        A = gy [M][N]          B = w [N][K] (major)
//   bwd-weight  gw = gy^T x      A = gy [M][N] (major)  B = x [M][K] (major)
// Nothing is transposed in global memory.
//
// Work split (linear_plan.h): 64 x 64 output tiles, 256 threads = 2 x 2
// waves of 32 x 32 (2 x 2 MFMA fragments), reduction tiles of 64.  Forward
// and bwd-data have few output tiles and a long reduction, so grid.z slices
// the reduction; each slice writes its fp32 tile into its own slab and
// fc_finalize_kernel adds the slabs in slice order, adds the bias and rounds
// to bf16 once.  A plan without a split stores bf16 from the accumulators.
// bwd-weight has N K / 4096 tiles and reduces over the batch only: one
// launch, fp32 stores, and the workgroups of column tile 0 sum gb from the
// gy tiles they stage anyway.  No atomics anywhere: the same bits every run.
//
// Operand movement: a tile is 64 rows of 64 reduction elements in LDS, row
// stride 144 bytes.  144 = 36 banks, and 36 r mod 64 for r = 0..15 are 16
// distinct multiples of 4, so the ds_read_b128 fragment reads of 16
// consecutive rows cover the 64 banks once.  A thread fetches 2 x 16 bytes
// per operand and tile from global memory into registers while the MFMAs of
// the current tile run, and writes them to the other LDS buffer afterwards;
// two buffers need one barrier per tile.
//   reduction-contiguous: 16-byte stores, row = tid / 8, chunk = tid % 8.
//   reduction-major: a thread loads the same 8 columns of reduction rows 2p
//     and 2p + 1, and stores 8 dwords {row 2p, row 2p + 1} at LDS row =
//     column, so the fragment reads are the same ds_read_b128 as above.
//     Per wave the stores hit 4 column chunks x 16 row pairs: two lanes per
//     bank, against 64 bytes contiguous per global row.
// Tails: a 16-byte chunk is either inside its operand or not loaded and
// zero in LDS (K and N are multiples of 8, so no chunk straddles an end; a
// reduction-major row past the batch is dropped as a row); stores test
// i < I and j < J.
//
// Compiler's kernel-resource-usage figures for gfx950 (256 threads;
// ScratchSize 0 in every variant; the GEMM variants hold 36864 bytes of LDS,
// which alone would allow 4 workgroups per CU):
//   kernel                                 VGPRs  AGPRs  waves/SIMD
//   fc_gemm_kernel<0,0,bf16>  fwd            72     24       4
//   fc_gemm_kernel<0,0,slab>  fwd            72     24       4
//   fc_gemm_kernel<0,1,bf16>  bwd-data       74     24       4
//   fc_gemm_kernel<0,1,slab>  bwd-data       74     24       4
//   fc_gemm_kernel<1,1,grad>  bwd-weight     71     24       4
//   fc_finalize_kernel                       19      0       8
// Timings against the library GEMMs: profiles/linear_mfma.md.

#include "fedkit_common.h"
#include "linear_plan.h"
#include "multi_tensor.h"

namespace {

using fedkit_plan::kLinTile;
using fedkit_plan::LinearPlan;

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __hip_bfloat16 bf16;

constexpr int kT = kLinTile;         // tile edge, reduction tile depth
constexpr int kRowB = kT * 2 + 16;   // LDS row stride in bytes (bank note)
constexpr int kTileB = kT * kRowB;   // one operand tile
static_assert(kT == 64, "thread-to-chunk maps below are written for 64");

constexpr int kOutBf16 = 0;   // bf16(acc + bias)
constexpr int kOutSlab = 1;   // fp32 partial tile of reduction slice z
constexpr int kOutGrad = 2;   // fp32, and gb from the A tiles

// results are compared bit for bit: no packed fp32 ALU forms
#define FC_KERNEL \
  __global__ void __attribute__((target("no-packed-fp32-ops")))

// This thread's 2 x 16 bytes of the tile (rows row0.., reduction r0..) of an
// operand with `rows` rows and reduction length R; zeros outside.
//   !TR: src[rows][R]; chunk tid % 8 of tile rows tid / 8 and tid / 8 + 32.
//   TR:  src[R][rows]; 8 columns of reduction rows 2p, 2p + 1.
template <bool TR>
__device__ __forceinline__ void load_tile(const bf16* __restrict__ src,
                                          int rows, int R, int row0, int r0,
                                          int tid, uint4 (&v)[2]) {
  if (!TR) {
    const int r = r0 + (tid & 7) * 8;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int row = row0 + (tid >> 3) + 32 * h;
      v[h] = make_uint4(0, 0, 0, 0);
      if (row < rows && r < R)
        v[h] = *reinterpret_cast<const uint4*>(src + (long long)row * R + r);
    }
  } else {
    const int wave = tid >> 6, lane = tid & 63;
    const int col = row0 + ((wave & 1) * 4 + (lane & 3)) * 8;
    const int p = (wave >> 1) * 16 + (lane >> 2);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int r = r0 + 2 * p + h;
      v[h] = make_uint4(0, 0, 0, 0);
      if (col < rows && r < R)
        v[h] = *reinterpret_cast<const uint4*>(src + (long long)r * rows + col);
    }
  }
}

// The same 2 x 16 bytes into the LDS tile [64 rows][64 reduction] at `tile`.
template <bool TR>
__device__ __forceinline__ void store_tile(char* tile, int tid,
                                           const uint4 (&v)[2]) {
  if (!TR) {
#pragma unroll
    for (int h = 0; h < 2; ++h)
      *reinterpret_cast<uint4*>(tile + ((tid >> 3) + 32 * h) * kRowB +
                                (tid & 7) * 16) = v[h];
  } else {
    const int wave = tid >> 6, lane = tid & 63;
    const int c0 = ((wave & 1) * 4 + (lane & 3)) * 8;
    const int p = (wave >> 1) * 16 + (lane >> 2);
    const unsigned a[4] = {v[0].x, v[0].y, v[0].z, v[0].w};   // row 2p
    const unsigned b[4] = {v[1].x, v[1].y, v[1].z, v[1].w};   // row 2p + 1
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const unsigned lo = a[j >> 1], hi = b[j >> 1];
      const unsigned pair = (j & 1) ? (lo >> 16) | (hi & 0xffff0000u)
                                    : (lo & 0xffffu) | (hi << 16);
      *reinterpret_cast<unsigned*>(tile + (c0 + j) * kRowB + 4 * p) = pair;
    }
  }
}

__device__ __forceinline__ float bf16_lo(unsigned u) {
  return __uint_as_float(u << 16);
}
__device__ __forceinline__ float bf16_hi(unsigned u) {
  return __uint_as_float(u & 0xffff0000u);
}

// grid (ceil(I / 64), ceil(J / 64), splits); slice z reduces tiles
// [z kt_per_split, (z + 1) kt_per_split) of ceil(R / 64).
//   kOutBf16: out bf16 [I][J], bias fp32 [J] or null (splits == 1)
//   kOutSlab: out fp32 [splits][I][J]
//   kOutGrad: out fp32 [I][J]; gb fp32 [I] or null = sum_r A(i, r)
template <bool TA, bool TB, int OUT>
FC_KERNEL __launch_bounds__(256)
fc_gemm_kernel(const bf16* __restrict__ A, const bf16* __restrict__ B,
               void* __restrict__ out, const float* __restrict__ bias,
               float* __restrict__ gb, int I, int J, int R,
               int kt_per_split) {
  __shared__ __attribute__((aligned(16))) char smem[4 * kTileB];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int i0 = blockIdx.x * kT, j0 = blockIdx.y * kT;
  const int nkt = (R + kT - 1) / kT;
  const int kt0 = blockIdx.z * kt_per_split;
  const int kt1 = min(kt0 + kt_per_split, nkt);
  const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
  // fragment of lane l: row l % 16, 8 reduction elements from (l / 16) * 8
  const int frag = (lane & 15) * kRowB + (lane >> 4) * 16;
  const bool want_gb = OUT == kOutGrad && gb != nullptr && blockIdx.y == 0;

  uint4 va[2], vb[2];
  load_tile<TA>(A, I, R, i0, kt0 * kT, tid, va);
  load_tile<TB>(B, J, R, j0, kt0 * kT, tid, vb);
  store_tile<TA>(smem, tid, va);
  store_tile<TB>(smem + kTileB, tid, vb);

  f32x4 acc[2][2] = {};
  float bsum = 0.f;
  for (int kt = kt0; kt < kt1; ++kt) {
    char* cur = smem + ((kt - kt0) & 1) * 2 * kTileB;
    char* nxt = smem + ((kt - kt0 + 1) & 1) * 2 * kTileB;
    // the stores of tile kt have landed; every wave is done reading nxt
    __syncthreads();
    if (kt + 1 < kt1) {
      load_tile<TA>(A, I, R, i0, (kt + 1) * kT, tid, va);
      load_tile<TB>(B, J, R, j0, (kt + 1) * kT, tid, vb);
    }
#pragma unroll
    for (int kk = 0; kk < kT; kk += 32) {
      bf16x8 a[2], b[2];
#pragma unroll
      for (int f = 0; f < 2; ++f) {
        a[f] = *reinterpret_cast<const bf16x8*>(
            cur + (wm + 16 * f) * kRowB + frag + kk * 2);
        b[f] = *reinterpret_cast<const bf16x8*>(
            cur + kTileB + (wn + 16 * f) * kRowB + frag + kk * 2);
      }
#pragma unroll
      for (int fa = 0; fa < 2; ++fa)
#pragma unroll
        for (int fb = 0; fb < 2; ++fb)
          acc[fa][fb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              a[fa], b[fb], acc[fa][fb], 0, 0, 0);
    }
    if (want_gb) {
      // thread: row tid / 4 of the A tile, its quarter tid % 4 of the batch
      const uint4* q = reinterpret_cast<const uint4*>(
          cur + (tid >> 2) * kRowB + (tid & 3) * 32);
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const uint4 u = q[h];
        bsum += bf16_lo(u.x); bsum += bf16_hi(u.x);
        bsum += bf16_lo(u.y); bsum += bf16_hi(u.y);
        bsum += bf16_lo(u.z); bsum += bf16_hi(u.z);
        bsum += bf16_lo(u.w); bsum += bf16_hi(u.w);
      }
    }
    if (kt + 1 < kt1) {
      store_tile<TA>(nxt, tid, va);
      store_tile<TB>(nxt + kTileB, tid, vb);
    }
  }

  // D fragment: lane l holds column l % 16, rows (l / 16) * 4 + v
#pragma unroll
  for (int fa = 0; fa < 2; ++fa)
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int i = i0 + wm + 16 * fa + (lane >> 4) * 4 + v;
      if (i >= I) continue;
#pragma unroll
      for (int fb = 0; fb < 2; ++fb) {
        const int j = j0 + wn + 16 * fb + (lane & 15);
        if (j >= J) continue;
        const float s = acc[fa][fb][v];
        if (OUT == kOutBf16)
          static_cast<bf16*>(out)[(long long)i * J + j] =
              __float2bfloat16(bias ? s + bias[j] : s);
        else if (OUT == kOutSlab)
          static_cast<float*>(out)[((long long)blockIdx.z * I + i) * J + j] =
              s;
        else
          static_cast<float*>(out)[(long long)i * J + j] = s;
      }
    }
  if (want_gb) {
    bsum += __shfl_xor(bsum, 1, 64);
    bsum += __shfl_xor(bsum, 2, 64);
    const int i = i0 + (tid >> 2);
    if ((tid & 3) == 0 && i < I) gb[i] = bsum;
  }
}

struct __attribute__((aligned(8))) bf16x4 {
  bf16 v[4];
};

// out[e] = bf16(slab[0][e] + slab[1][e] + ... + bias[e % J]), 4 elements per
// thread; total = I J and J are multiples of 4.
FC_KERNEL __launch_bounds__(256)
fc_finalize_kernel(const float* __restrict__ slab, int splits, long long total,
                   int J, const float* __restrict__ bias,
                   bf16* __restrict__ out) {
  for (long long e = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
       e < total; e += (long long)gridDim.x * 256 * 4) {
    f32x4 s = *reinterpret_cast<const f32x4*>(slab + e);
    for (int z = 1; z < splits; ++z)
      s += *reinterpret_cast<const f32x4*>(slab + z * total + e);
    if (bias) {
      const float* b = bias + e % J;
      s += f32x4{b[0], b[1], b[2], b[3]};
    }
    bf16x4 h;
#pragma unroll
    for (int c = 0; c < 4; ++c) h.v[c] = __float2bfloat16(s[c]);
    *reinterpret_cast<bf16x4*>(out + e) = h;
  }
}

void check_operand(const char* op, const char* name, const at::Tensor& t,
                   const at::Tensor& like) {
  TORCH_CHECK(t.is_cuda() && t.device() == like.device(), op, ": ", name,
              " must be on the GPU of the first operand");
  TORCH_CHECK(t.dim() == 2 && t.scalar_type() == at::kBFloat16 &&
                  t.is_contiguous(),
              op, ": ", name, " must be a contiguous 2-D bf16 tensor");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0, op, ": ",
              name, " must start 16-byte aligned");
}

// M >= 1 rows, K and N multiples of 8 (every row starts 16-byte aligned)
void check_sizes(const char* op, long long M, long long N, long long K) {
  const long long lim = (1LL << 31) - 2 * kT;
  TORCH_CHECK(M >= 1 && N >= 8 && K >= 8 && N % 8 == 0 && K % 8 == 0, op,
              ": needs M >= 1 and N, K positive multiples of 8, got M = ", M,
              ", N = ", N, ", K = ", K);
  TORCH_CHECK(M < lim && N < lim && K < lim, op, ": size above 2^31");
}

// bf16 out[I][J] = A B^T (+ bias) through the plan: direct, or slab + finalize
template <bool TB>
at::Tensor gemm_bf16(const char* op, const at::Tensor& a, const at::Tensor& b,
                     const float* bias, long long I, long long J,
                     long long R) {
  const LinearPlan p = fedkit_plan::plan_linear(I, J, R, true);
  TORCH_CHECK(p.tiles_j <= 65535, op, ": more than 65535 column tiles");
  auto out = at::empty({I, J}, a.options());
  const dim3 grid((unsigned)p.tiles_i, p.tiles_j, p.splits);
  const auto* ap = static_cast<const bf16*>(a.data_ptr());
  const auto* bp = static_cast<const bf16*>(b.data_ptr());
  auto stream = fedkit_stream();
  if (p.splits == 1) {
    hipLaunchKernelGGL((fc_gemm_kernel<false, TB, kOutBf16>), grid, dim3(256),
                       0, stream, ap, bp, out.data_ptr(), bias, nullptr,
                       (int)I, (int)J, (int)R, p.kt_per_split);
    return out;
  }
  auto slab = at::empty({(long long)p.splits, I, J},
                        a.options().dtype(at::kFloat));
  hipLaunchKernelGGL((fc_gemm_kernel<false, TB, kOutSlab>), grid, dim3(256), 0,
                     stream, ap, bp, slab.data_ptr(), nullptr, nullptr, (int)I,
                     (int)J, (int)R, p.kt_per_split);
  hipLaunchKernelGGL(fc_finalize_kernel, dim3(grid_1d(I * J / 4, 256)),
                     dim3(256), 0, stream, slab.data_ptr<float>(), p.splits,
                     I * J, (int)J, bias,
                     static_cast<bf16*>(out.data_ptr()));
  return out;
}

}  // namespace

at::Tensor fedkit_linear_mfma_fwd(const at::Tensor& x, const at::Tensor& w,
                                  const c10::optional<at::Tensor>& bias) {
  const char* op = "linear_mfma_fwd";
  check_operand(op, "x", x, x);
  check_operand(op, "w", w, x);
  TORCH_CHECK(x.size(1) == w.size(1), op, ": x [M,K] and w [N,K] differ in K");
  const long long M = x.size(0), N = w.size(0), K = w.size(1);
  check_sizes(op, M, N, K);
  const float* bp = nullptr;
  if (bias.has_value()) {
    TORCH_CHECK(bias->is_cuda() && bias->device() == x.device() &&
                    bias->scalar_type() == at::kFloat && bias->dim() == 1 &&
                    bias->size(0) == N && bias->is_contiguous(),
                op, ": bias must be a contiguous fp32 [N] on x's device");
    bp = bias->data_ptr<float>();
  }
  const fedkit_mt::DeviceGuard guard(x.device());
  return gemm_bf16<false>(op, x, w, bp, M, N, K);
}

at::Tensor fedkit_linear_mfma_bwd_data(const at::Tensor& gy,
                                       const at::Tensor& w) {
  const char* op = "linear_mfma_bwd_data";
  check_operand(op, "gy", gy, gy);
  check_operand(op, "w", w, gy);
  TORCH_CHECK(gy.size(1) == w.size(0), op,
              ": gy [M,N] and w [N,K] differ in N");
  const long long M = gy.size(0), N = w.size(0), K = w.size(1);
  check_sizes(op, M, N, K);
  const fedkit_mt::DeviceGuard guard(gy.device());
  return gemm_bf16<true>(op, gy, w, nullptr, M, K, N);
}

std::vector<at::Tensor> fedkit_linear_mfma_bwd_weight(const at::Tensor& gy,
                                                      const at::Tensor& x,
                                                      bool want_bias) {
  const char* op = "linear_mfma_bwd_weight";
  check_operand(op, "gy", gy, gy);
  check_operand(op, "x", x, gy);
  TORCH_CHECK(gy.size(0) == x.size(0), op,
              ": gy [M,N] and x [M,K] differ in M");
  const long long M = gy.size(0), N = gy.size(1), K = x.size(1);
  check_sizes(op, M, N, K);
  const LinearPlan p = fedkit_plan::plan_linear(N, K, M, false);
  TORCH_CHECK(p.tiles_j <= 65535, op, ": more than 65535 column tiles");
  const fedkit_mt::DeviceGuard guard(gy.device());
  auto opts = gy.options().dtype(at::kFloat);
  auto gw = at::empty({N, K}, opts);
  at::Tensor gb;
  if (want_bias) gb = at::empty({N}, opts);
  hipLaunchKernelGGL((fc_gemm_kernel<true, true, kOutGrad>),
                     dim3((unsigned)p.tiles_i, p.tiles_j, 1), dim3(256), 0,
                     fedkit_stream(), static_cast<const bf16*>(gy.data_ptr()),
                     static_cast<const bf16*>(x.data_ptr()), gw.data_ptr(),
                     nullptr, want_bias ? gb.data_ptr<float>() : nullptr,
                     (int)N, (int)K, (int)M, p.kt_per_split);
  if (want_bias) return {gw, gb};
  return {gw};
}
