// Tiled InfoNCE for patch grids 64 < P <= 1024 (fedkit.ops.losses.info_nce,
// federated_cpc.py:149-180): forward and backward as fp32 MFMA GEMMs.  The
// one-workgroup kernel of losses_extra.hip keeps P <= 64.
//
//   raw[i][j] = sum_d Z[d][i] Zhat[d][j]          Z, Zhat: [D, P], P contiguous
//   zz        = raw / (nz[i] nzh[j])              nz, nzh: column 2-norms
//   soft      = row softmax(zz),   loss = -sum_i log(soft[i][i] + 1e-6)
//
// Forward, three launches, no float atomics, every sum in a fixed order:
//
// 1. nce_sim_kernel: grid (tiles_p, tiles_p, splits), 256 threads, one 64 x 64
//    tile of raw over one slice of D (infonce_plan.h).  D is walked in chunks
//    of 32 rows.  Both operands are reduction-major, so a chunk is staged as it
//    lies in memory: 32 rows of 64 columns, a thread loads 16 bytes (8 for
//    bf16, widened here) of two rows of each operand; rows past the slice and
//    columns past P are staged as zeros and never read.  Two buffers, one
//    barrier per chunk; the next chunk's global loads are issued right after
//    the barrier and are in flight during the MFMAs.
//    MFMA: wave w owns the 32 x 32 block (w / 2, w % 2) of the tile.  For
//    v_mfma_f32_32x32x2_f32 lane l supplies A[l % 32][l / 32] and
//    B[l / 32][l % 32], which here are lds[k][i0 + l % 32] of the two staged
//    tiles: no transpose.  The k rows of one MFMA are (k, k + 8): which rows
//    share an instruction does not matter for a sum.
//    LDS banks: the row stride is 68 floats, so rows k and k + 8 start
//    8 * 68 = 544 = 32 (mod 64) banks apart: lanes 0..31 read 32 consecutive
//    banks, lanes 32..63 the other 32.  The staging stores are 16 bytes per
//    lane, 16 lanes to a row of 256 contiguous bytes.
//    Column sums of squares come from the same registers: every staged value
//    of a wave's 32 columns passes through exactly one lane as an MFMA
//    operand, so a lane adds a * a as it goes, lanes l and l + 32 are added at
//    the end, and the tiles of the first tile row / column write them.
//    Output: part[split][P][P] and ssq[split][2][P].
// 2. nce_row_kernel: one workgroup per row i.  Partials and sums of squares
//    added in split order, zz, row max, sum of exponentials, soft, and the
//    row's loss term (accurate expf / logf).
// 3. nce_loss_kernel: one workgroup adds the P row terms.
//
// Backward, two launches:
//
// 4. nce_prep_kernel: one workgroup per 32 rows of the P x P matrices, wave w
//    takes rows 8 w .. 8 w + 7.  With w_i = g s_ii / (s_ii + 1e-6) and
//    dzz = w_i (soft - I) it writes
//      M[i][j]  = dzz[i][j] / (nz[i] nzh[j]), i != j, and its transpose MT,
//      md[i]    = dzz[i][i] / (nz[i] nzh[i]),
//      ct[i]    = (sum_j dzz zz) / nz[i]^2,
//      up[b][j] = (sum over the block's rows of dzz zz) / nzh[j]^2,
//    so that  gZ = Zhat MT + Zhat md - Z ct  and
//    gZhat = Z M + Z md - Zhat (sum_b up[b]).  The diagonal stays out of the
//    products: dzz[i][i] = -w_i (1 - s_ii) is P times an off-diagonal entry,
//    and inside one long accumulation chain every later add would round at
//    its magnitude (seen at P = 1024, D = 8: 4 x the error of a blocked sum).
//    M and MT are [ld][ld], ld = P rounded up to 64, zero past P: the GEMM
//    stages them with aligned 16-byte loads and no tail.  g is read from its
//    device pointer.
// 5. nce_grad_kernel: grid (ceil(D / 64), tiles_p, 2), blockIdx.z selects gZ
//    or gZhat; out[D][P] = A[D][P] B[P][P], a 64 x 64 tile per workgroup, the
//    reduction over P in chunks of 32, double buffered as in 1.  A is stored
//    [row][k], stride 36 floats: lane l reads 16 bytes of row l % 32 at
//    k = 8 s + 4 (l / 32) and feeds four MFMAs; 36 = 4 (mod 64) spreads 16
//    consecutive lanes over all 64 banks.  B is stored [k][column], stride 72
//    floats: the two k rows of one MFMA are 4 apart, 4 * 72 = 32 (mod 64).
//    The epilogue adds the md term, subtracts the ct / up term, and stores in
//    the input dtype.

#include "fedkit_common.h"
#include "infonce_plan.h"
#include "multi_tensor.h"

namespace {

using namespace fedkit_plan;

constexpr int kBlock = 256;
constexpr int kSimRow = kNceTile + 4;     // 68: rows k, k + 8 half a bank ring apart
constexpr int kSimBuf = kNceChunk * kSimRow;
constexpr int kGradRowA = kNceChunk + 4;  // 36
constexpr int kGradRowB = kNceTile + 8;   // 72
constexpr int kGradBufA = kNceTile * kGradRowA;
constexpr int kGradBufB = kNceChunk * kGradRowB;
constexpr int kPrepRows = 32;

typedef float f4 __attribute__((ext_vector_type(4)));
typedef float acc_t __attribute__((ext_vector_type(16)));
// loads of 4 elements at element alignment: P is odd more often than not
typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));
typedef unsigned short us4u __attribute__((ext_vector_type(4), aligned(2)));

// accumulator register v of lane l is C[acc_row(v, l)][l % 32]
__device__ __forceinline__ int acc_row(int v, int l) {
  return 8 * (v >> 2) + 4 * (l >> 5) + (v & 3);
}

// Elements c .. c + 3 of row `row` of a [rows, ld] matrix as fp32.  Elements
// at or past `limit`, and all four when !row_ok, are zeros and are not read.
template <typename T>
__device__ __forceinline__ f4 load_row4(const T* __restrict__ base,
                                        long long row, int ld, int c, int limit,
                                        bool row_ok) {
  f4 v = {};
  if (!row_ok) return v;
  const T* p = base + row * ld + c;
  if (c + 4 <= limit) {
    if constexpr (is_bf16<T>::value) {
      const us4u r = *reinterpret_cast<const us4u*>(p);
#pragma unroll
      for (int e = 0; e < 4; ++e)
        v[e] = __uint_as_float((unsigned)r[e] << 16);
    } else {
      v = *reinterpret_cast<const f4u*>(p);
    }
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (c + e < limit) v[e] = to_f32(p[e]);
  }
  return v;
}

// Sum (or max) over the 256 threads, in every thread: wave butterfly, then
// the four waves in index order.
template <bool MAX>
__device__ __forceinline__ float block_all(float v, float* red /* [4] */) {
#pragma unroll
  for (int off = 32; off; off >>= 1) {
    const float o = __shfl_xor(v, off, kWave);
    v = MAX ? fmaxf(v, o) : v + o;
  }
  __syncthreads();   // red may still be read from a previous call
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return MAX ? fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]))
             : (red[0] + red[1]) + (red[2] + red[3]);
}

// ------------------------------------------------------------ 1. similarity

template <typename T>
__global__ void __launch_bounds__(kBlock)
nce_sim_kernel(const T* __restrict__ Z, const T* __restrict__ Zh, long long D,
               int P, int chunks_per_split,
               float* __restrict__ part,   // [splits, P, P]
               float* __restrict__ ssq) {  // [splits, 2, P]
  __shared__ __attribute__((aligned(16))) float lds[2][2][kSimBuf];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wi = wave >> 1, wj = wave & 1, h = lane >> 5, l32 = lane & 31;
  const int tj = blockIdx.x, ti = blockIdx.y, sp = blockIdx.z;
  const long long kbeg = (long long)sp * chunks_per_split * kNceChunk;
  const long long kend =
      min(D, kbeg + (long long)chunks_per_split * kNceChunk);
  // staging: rows srow and srow + 16 of the chunk, columns scol .. scol + 3
  const int srow = tid >> 4, scol = 4 * (tid & 15);
  f4 za[2], zb[2];
  auto load_chunk = [&](long long k0) {
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const long long d = k0 + srow + 16 * r;
      za[r] = load_row4(Z, d, P, ti * kNceTile + scol, P, d < kend);
      zb[r] = load_row4(Zh, d, P, tj * kNceTile + scol, P, d < kend);
    }
  };
  acc_t acc = {};
  float sa = 0.f, sb = 0.f;
  load_chunk(kbeg);
  for (long long k0 = kbeg, b = 0; k0 < kend; k0 += kNceChunk, b ^= 1) {
    float* la = lds[b][0];
    float* lb = lds[b][1];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      *reinterpret_cast<f4*>(la + (srow + 16 * r) * kSimRow + scol) = za[r];
      *reinterpret_cast<f4*>(lb + (srow + 16 * r) * kSimRow + scol) = zb[r];
    }
    __syncthreads();
    if (k0 + kNceChunk < kend) load_chunk(k0 + kNceChunk);
    const float* ra = la + 8 * h * kSimRow + 32 * wi + l32;
    const float* rb = lb + 8 * h * kSimRow + 32 * wj + l32;
#pragma unroll
    for (int s = 0; s < kNceChunk / 2; ++s) {
      const int k = (s & 7) + 16 * (s >> 3);      // this lane's row: k + 8 h
      const float a = ra[k * kSimRow], bb = rb[k * kSimRow];
      sa += a * a;
      sb += bb * bb;
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bb, acc, 0, 0, 0);
    }
  }
  const int row0 = ti * kNceTile + 32 * wi, col = tj * kNceTile + 32 * wj + l32;
  if (col < P) {
    float* out = part + (long long)sp * P * P;
#pragma unroll
    for (int v = 0; v < 16; ++v) {
      const int row = row0 + acc_row(v, lane);
      if (row < P) out[(long long)row * P + col] = acc[v];
    }
  }
  // sums of squares: lanes l and l + 32 hold the two halves of a column
  const float sa2 = sa + __shfl_xor(sa, 32, kWave);
  const float sb2 = sb + __shfl_xor(sb, 32, kWave);
  float* sq = ssq + (long long)sp * 2 * P;
  if (tj == 0 && wj == 0 && h == 0 && row0 + l32 < P) sq[row0 + l32] = sa2;
  if (ti == 0 && wi == 0 && h == 0 && col < P) sq[P + col] = sb2;
}

// ------------------------------------------------------------- 2. row pass

__global__ void __launch_bounds__(kBlock)
nce_row_kernel(const float* __restrict__ part, const float* __restrict__ ssq,
               int splits, int P, float* __restrict__ zz,
               float* __restrict__ soft, float* __restrict__ norms,
               float* __restrict__ row_loss) {
  __shared__ float red[4];
  constexpr int kPer = kNceMaxP / kBlock;
  const int i = blockIdx.x, tid = threadIdx.x;
  float s = 0.f;
  for (int p = 0; p < splits; ++p) s += ssq[(long long)p * 2 * P + i];
  const float nz = sqrtf(s);
  if (tid == 0) norms[i] = nz;
  float val[kPer];
  float m = -INFINITY;
#pragma unroll
  for (int q = 0; q < kPer; ++q) {
    const int j = tid + kBlock * q;
    val[q] = -INFINITY;
    if (j < P) {
      float raw = 0.f, sh = 0.f;
      for (int p = 0; p < splits; ++p) {
        raw += part[((long long)p * P + i) * P + j];
        sh += ssq[(long long)p * 2 * P + P + j];
      }
      const float nzh = sqrtf(sh);
      if (i == 0) norms[P + j] = nzh;
      val[q] = raw / (nz * nzh);
      zz[(long long)i * P + j] = val[q];
      m = fmaxf(m, val[q]);
    }
  }
  m = block_all<true>(m, red);
  float e = 0.f;
#pragma unroll
  for (int q = 0; q < kPer; ++q) {
    // -inf past P: expf gives 0
    val[q] = expf(val[q] - m);
    e += val[q];
  }
  e = block_all<false>(e, red);
#pragma unroll
  for (int q = 0; q < kPer; ++q) {
    const int j = tid + kBlock * q;
    if (j < P) {
      const float p = val[q] / e;
      soft[(long long)i * P + j] = p;
      if (j == i) row_loss[i] = -logf(p + 1e-6f);
    }
  }
}

// ----------------------------------------------------------------- 3. loss

__global__ void __launch_bounds__(kBlock)
nce_loss_kernel(const float* __restrict__ row_loss, int P,
                float* __restrict__ loss) {
  __shared__ float red[4];
  float s = 0.f;
  for (int i = threadIdx.x; i < P; i += kBlock) s += row_loss[i];
  s = block_all<false>(s, red);
  if (threadIdx.x == 0) loss[0] = s;
}

// ----------------------------------------------------------------- 4. prep

__global__ void __launch_bounds__(kBlock)
nce_prep_kernel(const float* __restrict__ zz, const float* __restrict__ soft,
                const float* __restrict__ norms,
                const float* __restrict__ gloss, int P, int ld,
                float* __restrict__ Mm,    // [ld, ld]
                float* __restrict__ Mt,    // [ld, ld]
                float* __restrict__ md,    // [ld], written below P
                float* __restrict__ ct,    // [ld]
                float* __restrict__ up) {  // [ld / 32, ld]
  __shared__ float us[4][kNceMaxP];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int i0 = blockIdx.x * kPrepRows + 8 * wave;
  const float g = gloss[0];
  float wr[8], inz[8], t[8];
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const int i = i0 + r;
    wr[r] = inz[r] = t[r] = 0.f;
    if (i < P) {
      const float s = soft[(long long)i * P + i];
      wr[r] = g * s / (s + 1e-6f);
      inz[r] = 1.f / norms[i];
    }
  }
  for (int j = lane; j < ld; j += kWave) {
    const float inzh = j < P ? 1.f / norms[P + j] : 0.f;
    float ucol = 0.f, mt[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const int i = i0 + r;
      float m = 0.f;
      if (i < P && j < P) {
        const float dz = wr[r] * soft[(long long)i * P + j] -
                         (i == j ? wr[r] : 0.f);
        const float pz = dz * zz[(long long)i * P + j];
        t[r] += pz;
        ucol += pz;
        m = dz * inz[r] * inzh;
        if (i == j) {
          md[i] = m;
          m = 0.f;
        }
      }
      Mm[(long long)i * ld + j] = m;
      mt[r] = m;
    }
    f4* mtp = reinterpret_cast<f4*>(Mt + (long long)j * ld + i0);
    mtp[0] = f4{mt[0], mt[1], mt[2], mt[3]};
    mtp[1] = f4{mt[4], mt[5], mt[6], mt[7]};
    us[wave][j] = ucol * inzh * inzh;
  }
#pragma unroll
  for (int r = 0; r < 8; ++r) {
#pragma unroll
    for (int off = 32; off; off >>= 1) t[r] += __shfl_xor(t[r], off, kWave);
    if (lane == 0) ct[i0 + r] = t[r] * inz[r] * inz[r];
  }
  __syncthreads();
  for (int j = tid; j < ld; j += kBlock)
    up[(long long)blockIdx.x * ld + j] =
        ((us[0][j] + us[1][j]) + us[2][j]) + us[3][j];
}

// ------------------------------------------------------- 5. gradient GEMMs

template <typename T>
__global__ void __launch_bounds__(kBlock)
nce_grad_kernel(const T* __restrict__ Z, const T* __restrict__ Zh,
                const float* __restrict__ Mm, const float* __restrict__ Mt,
                const float* __restrict__ md, const float* __restrict__ ct,
                const float* __restrict__ up, int up_blocks, T* __restrict__ gZ, T* __restrict__ gZh,
                long long D, int P, int ld) {
  __shared__ __attribute__((aligned(16))) float lds_a[2][kGradBufA];
  __shared__ __attribute__((aligned(16))) float lds_b[2][kGradBufB];
  const bool hat = blockIdx.z == 1;
  const T* __restrict__ A = hat ? Z : Zh;     // the product's left operand
  const T* __restrict__ X = hat ? Zh : Z;     // the epilogue's own input
  const float* __restrict__ B = hat ? Mm : Mt;
  const float* __restrict__ coef = hat ? up : ct;
  const int ncoef = hat ? up_blocks : 1;
  T* __restrict__ out = hat ? gZh : gZ;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1, h = lane >> 5, l32 = lane & 31;
  const long long d0 = (long long)blockIdx.x * kNceTile;
  const int n0 = blockIdx.y * kNceTile;
  // staging: A rows arow, arow + 32 at k acol ..; B rows brow, brow + 16
  const int arow = tid >> 3, acol = 4 * (tid & 7);
  const int brow = tid >> 4, bcol = 4 * (tid & 15);
  f4 ar[2], br[2];
  auto load_chunk = [&](int k0) {
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const long long d = d0 + arow + 32 * r;
      ar[r] = load_row4(A, d, P, k0 + acol, P, d < D);
      // k0 + brow + 16 r < 32 ceil(P / 32) <= ld and n0 + bcol + 3 < ld
      br[r] = *reinterpret_cast<const f4*>(
          B + (long long)(k0 + brow + 16 * r) * ld + n0 + bcol);
    }
  };
  acc_t acc = {};
  load_chunk(0);
  for (int k0 = 0, b = 0; k0 < P; k0 += kNceChunk, b ^= 1) {
    float* la = lds_a[b];
    float* lb = lds_b[b];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      *reinterpret_cast<f4*>(la + (arow + 32 * r) * kGradRowA + acol) = ar[r];
      *reinterpret_cast<f4*>(lb + (brow + 16 * r) * kGradRowB + bcol) = br[r];
    }
    __syncthreads();
    if (k0 + kNceChunk < P) load_chunk(k0 + kNceChunk);
    const float* ra = la + (32 * wm + l32) * kGradRowA + 4 * h;
    const float* rb = lb + 4 * h * kGradRowB + 32 * wn + l32;
#pragma unroll
    for (int s = 0; s < kNceChunk / 8; ++s) {
      const f4 a = *reinterpret_cast<const f4*>(ra + 8 * s);
#pragma unroll
      for (int e = 0; e < 4; ++e)
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(
            a[e], rb[(8 * s + e) * kGradRowB], acc, 0, 0, 0);
    }
  }
  const int col = n0 + 32 * wn + l32;
  if (col >= P) return;
  float c = 0.f;
  for (int p = 0; p < ncoef; ++p) c += coef[(long long)p * ld + col];
  const float dg = md[col];
#pragma unroll
  for (int v = 0; v < 16; ++v) {
    const long long d = d0 + 32 * wm + acc_row(v, lane);
    if (d < D)
      from_f32((acc[v] + to_f32(A[d * P + col]) * dg) -
                   to_f32(X[d * P + col]) * c,
               out[d * P + col]);
  }
}

void check_inputs(const char* op, const at::Tensor& Z, const at::Tensor& Zhat) {
  TORCH_CHECK(Z.is_cuda() && Zhat.is_cuda(), op, ": Z and Zhat must be on a GPU");
  TORCH_CHECK(Z.dim() == 2 && Zhat.dim() == 2, op,
              ": Z and Zhat must be two-dimensional [D, P]");
  TORCH_CHECK(Z.sizes() == Zhat.sizes(), op, ": Z and Zhat differ in shape");
  TORCH_CHECK(Z.scalar_type() == Zhat.scalar_type() &&
              Z.device() == Zhat.device(), op,
              ": Z and Zhat differ in dtype or device");
  TORCH_CHECK(Z.is_contiguous() && Zhat.is_contiguous(), op,
              ": Z and Zhat must be contiguous");
  TORCH_CHECK(Z.size(0) >= 1, op, ": D must be at least 1");
  TORCH_CHECK(Z.size(1) > kNceMinP && Z.size(1) <= kNceMaxP, op, ": serves ",
              kNceMinP, " < P <= ", kNceMaxP, ", got P = ", Z.size(1));
}

void check_saved(const char* op, const char* name, const at::Tensor& t,
                 const at::Tensor& Z, long long rows, long long cols) {
  TORCH_CHECK(t.device() == Z.device() && t.scalar_type() == at::kFloat &&
              t.is_contiguous() && t.dim() == 2 && t.size(0) == rows &&
              t.size(1) == cols, op, ": ", name, " must be a contiguous fp32 [",
              rows, ", ", cols, "] on Z's device");
}

}  // namespace

std::vector<at::Tensor> fedkit_info_nce_tiled_fwd(const at::Tensor& Z,
                                                  const at::Tensor& Zhat) {
  check_inputs("info_nce_tiled_fwd", Z, Zhat);
  const fedkit_mt::DeviceGuard guard(Z.device());
  const long long D = Z.size(0);
  const int P = (int)Z.size(1);
  const InfoNcePlan pl = plan_info_nce(D, P);
  auto opts = Z.options().dtype(at::kFloat);
  auto loss = at::empty({}, opts);
  auto zz = at::empty({P, P}, opts);
  auto soft = at::empty({P, P}, opts);
  auto norms = at::empty({2, P}, opts);
  auto part = at::empty({pl.splits, P, P}, opts);
  auto ssq = at::empty({pl.splits, 2, P}, opts);
  auto row_loss = at::empty({P}, opts);
  auto stream = fedkit_stream();
  DISPATCH_F32_BF16(Z, "info_nce_tiled_fwd", {
    hipLaunchKernelGGL((nce_sim_kernel<scalar_t>),
                       dim3(pl.tiles_p, pl.tiles_p, pl.splits), dim3(kBlock),
                       0, stream, (const scalar_t*)Z.data_ptr(),
                       (const scalar_t*)Zhat.data_ptr(), D, P,
                       pl.chunks_per_split, part.data_ptr<float>(),
                       ssq.data_ptr<float>());
  });
  hipLaunchKernelGGL(nce_row_kernel, dim3(P), dim3(kBlock), 0, stream,
                     part.data_ptr<float>(), ssq.data_ptr<float>(), pl.splits,
                     P, zz.data_ptr<float>(), soft.data_ptr<float>(),
                     norms.data_ptr<float>(), row_loss.data_ptr<float>());
  hipLaunchKernelGGL(nce_loss_kernel, dim3(1), dim3(kBlock), 0, stream,
                     row_loss.data_ptr<float>(), P, loss.data_ptr<float>());
  return {loss, zz, soft, norms};
}

std::vector<at::Tensor> fedkit_info_nce_tiled_bwd(
    const at::Tensor& Z, const at::Tensor& Zhat, const at::Tensor& zz,
    const at::Tensor& soft, const at::Tensor& norms, const at::Tensor& gloss) {
  const char* op = "info_nce_tiled_bwd";
  check_inputs(op, Z, Zhat);
  const long long D = Z.size(0);
  const int P = (int)Z.size(1);
  check_saved(op, "zz", zz, Z, P, P);
  check_saved(op, "soft", soft, Z, P, P);
  check_saved(op, "norms", norms, Z, 2, P);
  TORCH_CHECK(gloss.device() == Z.device() && gloss.numel() == 1, op,
              ": gloss must be one element on Z's device");
  const fedkit_mt::DeviceGuard guard(Z.device());
  auto g = gloss.to(at::kFloat).contiguous();
  const int ld = (P + kNceTile - 1) / kNceTile * kNceTile;
  const int blocks = ld / kPrepRows;
  auto opts = Z.options().dtype(at::kFloat);
  auto Mm = at::empty({ld, ld}, opts);
  auto Mt = at::empty({ld, ld}, opts);
  auto md = at::empty({ld}, opts);
  auto ct = at::empty({ld}, opts);
  auto up = at::empty({blocks, ld}, opts);
  auto gZ = at::empty_like(Z);
  auto gZh = at::empty_like(Zhat);
  auto stream = fedkit_stream();
  hipLaunchKernelGGL(nce_prep_kernel, dim3(blocks), dim3(kBlock), 0, stream,
                     zz.data_ptr<float>(), soft.data_ptr<float>(),
                     norms.data_ptr<float>(), g.data_ptr<float>(), P, ld,
                     Mm.data_ptr<float>(), Mt.data_ptr<float>(),
                     md.data_ptr<float>(), ct.data_ptr<float>(),
                     up.data_ptr<float>());
  const long long dtiles = (D + kNceTile - 1) / kNceTile;
  TORCH_CHECK(dtiles <= 0x7fffffffLL, op, ": D too large");
  DISPATCH_F32_BF16(Z, "info_nce_tiled_bwd", {
    hipLaunchKernelGGL((nce_grad_kernel<scalar_t>),
                       dim3((unsigned)dtiles, ld / kNceTile, 2), dim3(kBlock),
                       0, stream, (const scalar_t*)Z.data_ptr(),
                       (const scalar_t*)Zhat.data_ptr(), Mm.data_ptr<float>(),
                       Mt.data_ptr<float>(), md.data_ptr<float>(),
                       ct.data_ptr<float>(), up.data_ptr<float>(), blocks, (scalar_t*)gZ.data_ptr(),
                       (scalar_t*)gZh.data_ptr(), D, P, ld);
  });
  return {gZ, gZh};
}
