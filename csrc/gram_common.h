// The MFMA Gram pass shared by krum.hip, geomed.hip and cclip.hip: G = A A^T
// of the K x N matrix of centred client vectors a_k = x_k - c, K <= 32, as
// per workgroup partials, and their sum in double.  The design notes (staging,
// double buffering, MFMA operand layout, LDS banks) are at the head of
// krum.hip.
#pragma once

#include "agg_common.h"
#include "multi_tensor.h"

namespace fedkit_agg {

constexpr int kTile = 256;           // elements per tile: 16 bytes per lane
constexpr int kRow = kTile + 4;      // LDS row stride in floats (bank note)

template <int KT>
struct Mfma;

template <>
struct Mfma<32> {
  typedef float acc_t __attribute__((ext_vector_type(16)));
  static constexpr int kAcc = 16;
  static __device__ __forceinline__ acc_t mma(float a, acc_t c) {
    return __builtin_amdgcn_mfma_f32_32x32x2f32(a, a, c, 0, 0, 0);
  }
  // accumulator register v of lane l is C[row][l % 32]
  static __device__ __forceinline__ int row(int v, int l) {
    return 8 * (v >> 2) + 4 * (l >> 5) + (v & 3);
  }
};

template <>
struct Mfma<16> {
  typedef float acc_t __attribute__((ext_vector_type(4)));
  static constexpr int kAcc = 4;
  static __device__ __forceinline__ acc_t mma(float a, acc_t c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, a, c, 0, 0, 0);
  }
  // accumulator register v of lane l is C[row][l % 16]
  static __device__ __forceinline__ int row(int v, int l) {
    return 4 * (l >> 4) + v;
  }
};

// This lane's 16 bytes of the wave's client rows and of the centre at
// element e0; elements >= n come back as zeros in both, so a = 0 there.
template <int KT>
__device__ __forceinline__ void load_tile(const ClientTable& t,
                                          const float* __restrict__ c, int K,
                                          long long n, long long e0, int wave,
                                          f4 (&xr)[KT / 4], f4& cv) {
  if (e0 + 4 <= n) {
    cv = load4(c + e0);
#pragma unroll
    for (int j = 0; j < KT / 4; ++j)
      if (wave + 4 * j < K) xr[j] = load4(t.x[wave + 4 * j] + e0);
  } else {
    cv = f4{};
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (e0 + e < n) cv[e] = c[e0 + e];
#pragma unroll
    for (int j = 0; j < KT / 4; ++j)
      if (wave + 4 * j < K) {
        xr[j] = f4{};
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (e0 + e < n) xr[j][e] = t.x[wave + 4 * j][e0 + e];
      }
  }
}

// part[blockIdx.x][i * KT + j] = partial sum_e a_i[e] a_j[e], a = x - c,
// over this workgroup's tiles.  gridDim.x <= number of tiles.
template <int KT>
FEDKIT_AGG_KERNEL __launch_bounds__(kBlock)
gram_kernel(ClientTable t, const float* __restrict__ c, int K, long long n,
            float* __restrict__ part) {
  using M = Mfma<KT>;
  constexpr int kSlots = kWave / KT;       // k-slots of one MFMA: 2 or 4
  constexpr int kSteps = 64 / (4 * kSlots);  // 16-byte reads per wave share
  constexpr int kBuf = KT * kRow;
  static_assert(2 * kBuf >= 4 * KT * KT, "the wave tiles reuse the staging");
  __shared__ __attribute__((aligned(16))) float lds[2 * kBuf];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const long long tiles = (n + kTile - 1) / kTile;
  // rows K..KT-1 of both buffers stay zero for the whole walk
  for (int i = K * kRow + tid; i < kBuf; i += kBlock) {
    lds[i] = 0.f;
    lds[kBuf + i] = 0.f;
  }
  typename M::acc_t acc = {};
  f4 xr[KT / 4], cv;
  long long tile = blockIdx.x;
  load_tile<KT>(t, c, K, n, tile * kTile + 4 * lane, wave, xr, cv);
  const int rd = (lane % KT) * kRow + 64 * wave + 4 * (lane / KT);
  for (int b = 0; tile < tiles; tile += gridDim.x, b ^= 1) {
    float* buf = lds + b * kBuf;
#pragma unroll
    for (int j = 0; j < KT / 4; ++j)
      if (wave + 4 * j < K)
        *reinterpret_cast<f4*>(buf + (wave + 4 * j) * kRow + 4 * lane) =
            xr[j] - cv;
    __syncthreads();
    const long long next = tile + gridDim.x;
    if (next < tiles)
      load_tile<KT>(t, c, K, n, next * kTile + 4 * lane, wave, xr, cv);
#pragma unroll
    for (int s = 0; s < kSteps; ++s) {
      const f4 a = *reinterpret_cast<const f4*>(buf + rd + s * 4 * kSlots);
      acc = M::mma(a[0], acc);
      acc = M::mma(a[1], acc);
      acc = M::mma(a[2], acc);
      acc = M::mma(a[3], acc);
    }
  }
  // the four waves' tiles through LDS, added in wave order
  __syncthreads();
#pragma unroll
  for (int v = 0; v < M::kAcc; ++v)
    lds[wave * KT * KT + M::row(v, lane) * KT + lane % KT] = acc[v];
  __syncthreads();
  float* out = part + (long long)blockIdx.x * (KT * KT);
  for (int e = tid; e < KT * KT; e += kBlock)
    out[e] = ((lds[e] + lds[KT * KT + e]) + lds[2 * KT * KT + e]) +
             lds[3 * KT * KT + e];
}

// Entry e of the Gram matrix: the nb partials summed in workgroup order, in
// double.
__device__ __forceinline__ double gram_entry(const float* __restrict__ part,
                                             int nb, int KT, int e) {
  double s = 0.0;
  for (int b = 0; b < nb; ++b) s += (double)part[(long long)b * KT * KT + e];
  return s;
}

// The passes that follow the Gram pass (select_mean_kernel of krum.hip,
// weighted_delta_kernel of weighted_delta.h) hold up to bucket_of(rows) client
// rows per thread.  Unit width of a bucket (tables at fedkit_krum_round and
// fedkit_geomed_round): 16-byte loads except where fedprox holds more than
// 16 clients' values.
constexpr int unit_width(int net, bool prox) {
  return prox && net > 16 ? 2 : 4;
}

constexpr int bucket_of(int K) { return K <= 8 ? 8 : K <= 16 ? 16 : 32; }

// Validates xs against z (and the centre), fills the client table.
inline ClientTable check_clients(const char* op,
                                 const std::vector<at::Tensor>& xs,
                                 const at::Tensor& z,
                                 const at::Tensor& center) {
  TORCH_CHECK(xs.size() >= 1 && xs.size() <= (size_t)kMaxClients, op, ": 1..",
              kMaxClients, " clients, got ", xs.size());
  const long long n = z.numel();
  fedkit_mt::check_flat(op, "z", z, z, n);
  fedkit_mt::check_flat(op, "center", center, z, n);
  ClientTable t = {};
  for (size_t k = 0; k < xs.size(); ++k) {
    fedkit_mt::check_flat(op, "every x_k", xs[k], z, n);
    t.x[k] = xs[k].data_ptr<float>();
  }
  return t;
}

struct GramPartials {
  at::Tensor part;   // fp32 [nb, KT * KT]
  int nb, KT;        // KT = 16 or 32 rows, K of them in use
};

// Launches the Gram pass of the K client rows of t around `center`.
// n = center.numel() > 0; the caller holds the device guard.
inline GramPartials launch_gram(const ClientTable& t, const at::Tensor& center,
                                int K, hipStream_t stream) {
  const long long n = center.numel();
  const int KT = K <= 16 ? 16 : 32;
  const int nb = (int)std::min<long long>((n + kTile - 1) / kTile, kRedGrid);
  auto part = at::empty({nb, KT * KT}, center.options());
  if (KT == 16)
    hipLaunchKernelGGL(gram_kernel<16>, dim3(nb), dim3(kBlock), 0, stream, t,
                       center.data_ptr<float>(), K, n, part.data_ptr<float>());
  else
    hipLaunchKernelGGL(gram_kernel<32>, dim3(nb), dim3(kBlock), 0, stream, t,
                       center.data_ptr<float>(), K, n, part.data_ptr<float>());
  return {part, nb, KT};
}

}  // namespace fedkit_agg
