// Krum / Multi-Krum aggregation round (Blanchard et al., 2017) over K <= 32
// client vectors: distance-based selection, then the mean of the selected
// clients with the round's residuals.
//
//   D_ij    = sum (x_i - x_j)^2                     non-finite counts as +inf
//   score_i = sum of the K - f - 2 smallest D_ij, j != i, in ascending order
//   sel     = the m clients of lowest score, ties to the lower index
//   znew    = (0 + x_k ... for selected k ascending) * inv      inv = 1/m
//   r_z     = sum (z - znew)^2;   fedprox: r_k = sum (rho (x_k - znew))^2
//
// Three kernels, no host read between them:
//
// 1. gram_kernel<KT>, KT = 16 or 32 rows (in gram_common.h, shared with
//    geomed.hip).  With a_k = x_k - c (c the centre, the old consensus) the
//    distances are D_ij = G_ii + G_jj - 2 G_ij of the Gram matrix G = A A^T
//    of the K x N matrix A.  Centring is what makes that form usable: its
//    error scales with |a_i|^2 + |a_j|^2, not with |x|^2.  At a block's
//    round 0 the consensus is 0 and the conditioning is that of the raw
//    vectors; nothing works around that.
//
//    A 256-thread workgroup walks tiles of T = 256 elements, grid-stride.
//    Staging: the four waves share the client rows (wave w takes rows w,
//    w + 4, ...); a lane loads 16 bytes of a row, so one instruction reads
//    1 KB of one client, coalesced, subtracts the centre's 16 bytes (loaded
//    once per tile) and writes a to an LDS tile [KT][T + 4].  Rows >= K are
//    zeroed once, elements >= n are written as zeros.  The tile is double
//    buffered: the next tile's global loads are issued right after the
//    barrier and are in flight during the MFMAs; two buffers need one
//    barrier per tile (a wave that writes buffer b again has passed the
//    barrier that follows every wave's last read of b).
//    MFMA: wave w owns elements [64 w, 64 w + 64) of the tile and all KT
//    rows.  Lane l reads 16 bytes of row l % KT at column group l / KT and
//    issues four v_mfma_f32_32x32x2_f32 (KT = 32) or v_mfma_f32_16x16x4_f32
//    (KT = 16) with the same VGPR as A and B: for these shapes the A layout
//    (row = lane % KT, k = lane / KT) is the B layout transposed, so one
//    register yields A A^T, and which elements share a k-slot does not
//    matter for a sum.  G_ij and G_ji are the same products added in the
//    same order, bit for bit.  A NaN or Inf client reaches only its own row
//    and column: C[i][j] holds products of rows i and j alone.
//    LDS banks: the row stride is T + 4 = 260 floats, 260 = 4 (mod 64), so
//    lane l's 16 bytes start at bank 4 (l % KT) + const (mod 64): 16
//    consecutive lanes cover all 64 banks once (8 lanes cover 32 once), and
//    the 16-byte reads are conflict-free under either grouping.  The
//    staging writes of a wave are 1 KB consecutive.
//    At the end the four waves' accumulators are added through LDS in wave
//    order and the workgroup writes one partial Gram, part[nb][KT * KT].
//    No float atomics.
//
// 2. krum_select_kernel, one workgroup: the partials summed in workgroup
//    order in double, D from the upper triangle (exactly symmetric), ranks
//    by counting with index tie-break, scores, selection.
//
// 3. select_mean_kernel<NET, V, PROX>: robust_kernel's thread work (a unit
//    of V elements, all loads first) with the sort replaced by the
//    selection, read from device memory with plain loads as the ascending
//    list of selected clients.  fedavg loads the listed rows only; fedprox
//    loads all K for the residuals.  znew is bitwise the torch sequence
//    `zeros; += xs[k] for selected k ascending; /= m`.

#include "gram_common.h"

#include <cmath>

namespace {

using namespace fedkit_agg;

enum { kFedAvg = 0, kFedProx = 1, kAdmm = 2 };   // aggregate_round's modes

// One workgroup.  D (fp32 [K, K]) from the nb partial Gram matrices; with
// q = K - f - 2 >= 1 also scores (fp32 [K]) and sel (int32 [2][K]: sel[0][k]
// is 1 for the m clients of lowest score, sel[1][0..m-1] lists them in
// ascending order, the rest is -1).  q = 0: D only.
FEDKIT_AGG_KERNEL __launch_bounds__(kBlock)
krum_select_kernel(const float* __restrict__ part, int nb, int KT, int K,
                   int q, int m, float* __restrict__ D,
                   float* __restrict__ scores, int* __restrict__ sel) {
#pragma clang fp contract(off)
  __shared__ double G[kMaxClients * kMaxClients];
  __shared__ float Dl[kMaxClients][kMaxClients + 1];
  __shared__ float asc[kMaxClients][kMaxClients + 1];
  __shared__ float sc[kMaxClients];
  __shared__ int chosen[kMaxClients];
  const int tid = threadIdx.x;
  for (int e = tid; e < KT * KT; e += kBlock)
    G[e] = gram_entry(part, nb, KT, e);
  __syncthreads();
  for (int e = tid; e < K * K; e += kBlock) {
    const int i = e / K, j = e % K;
    const int lo = min(i, j), hi = max(i, j);   // one triangle: D_ij == D_ji
    float d = (float)(G[lo * KT + lo] + G[hi * KT + hi] - 2.0 * G[lo * KT + hi]);
    if (!(fabsf(d) < INFINITY)) d = INFINITY;   // NaN and +-Inf
    else if (d < 0.f) d = 0.f;
    if (i == j) d = 0.f;
    Dl[i][j] = d;
    D[e] = d;
  }
  if (q < 1) return;
  __syncthreads();
  // rank of D_ij among client i's K - 1 distances, ties to the lower index:
  // a permutation of 0..K-2, so every slot of asc[i] is written once
  for (int e = tid; e < K * K; e += kBlock) {
    const int i = e / K, j = e % K;
    if (i == j) continue;
    const float d = Dl[i][j];
    int r = 0;
    for (int o = 0; o < K; ++o) {
      const float w = Dl[i][o];
      r += (o != i) && (w < d || (w == d && o < j));
    }
    asc[i][r] = d;
  }
  __syncthreads();
  if (tid < K) {
    double s = 0.0;
    for (int r = 0; r < q; ++r) s += (double)asc[tid][r];
    sc[tid] = (float)s;
    scores[tid] = (float)s;
  }
  __syncthreads();
  if (tid < K) {
    const float v = sc[tid];   // never NaN: a sum of values in [0, +inf]
    int r = 0;
    for (int o = 0; o < K; ++o) r += sc[o] < v || (sc[o] == v && o < tid);
    sel[tid] = chosen[tid] = r < m;   // the ranks are a permutation: m ones
    if (tid >= m) sel[K + tid] = -1;
  }
  __syncthreads();
  if (tid < K && chosen[tid]) {
    int pos = 0;
    for (int o = 0; o < tid; ++o) pos += chosen[o];
    sel[K + pos] = tid;
  }
}

// One unit of V elements at i0: znew, and this thread's residual sums.
// list[0..m-1] are the selected clients in ascending order.  Without PROX
// only their rows are loaded, slot j holding client list[j].  With PROX all
// K rows are loaded for the residuals and an unselected client adds +0.0f
// in its turn, which leaves every bit of the sum as it is: the sum starts
// from +0.0f and an fp32 sum is -0.0f only if both terms are, so it never
// is.  The value is selected, not multiplied: a NaN row stays out.
template <int NET, int V, bool PROX>
__device__ __forceinline__ void mean_unit(
    const ClientTable& t, const float* __restrict__ z,
    const int* __restrict__ list, float* __restrict__ znew, float rho,
    float inv, int K, int m, unsigned mask, long long i0, float& accz,
    float (&acck)[PROX ? NET : 1]) {
#pragma clang fp contract(off)
  // all loads of the unit are issued before the first use
  const int rows = PROX ? K : m;
  fv<V> raw[NET];
#pragma unroll
  for (int k = 0; k < NET; ++k)
    if (k < rows) {
      const int c = PROX ? k : __builtin_amdgcn_readfirstlane(list[k]);
      raw[k] = loadv<V>(t.x[c] + i0);
    }
  const fv<V> zv = loadv<V>(z + i0);
  fv<V> zn;
#pragma unroll
  for (int e = 0; e < V; ++e) {
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < NET; ++k)
      if (k < rows)
        s = s + ((!PROX || ((mask >> k) & 1u)) ? raw[k][e] : 0.f);
    zn[e] = s * inv;
  }
  storev<V>(znew + i0, zn);
  const fv<V> d = zv - zn;
#pragma unroll
  for (int e = 0; e < V; ++e) accz += d[e] * d[e];
  if constexpr (PROX) {
#pragma unroll
    for (int k = 0; k < NET; ++k)
      if (k < K) {
        const fv<V> yd = rho * (raw[k] - zn);
#pragma unroll
        for (int e = 0; e < V; ++e) acck[k] += yd[e] * yd[e];
      }
  }
}

// part[blockIdx.x][0] = partial sum (z - znew)^2 and, with PROX,
// part[blockIdx.x][1 + k] = partial sum (rho (x_k - znew))^2.  NET bounds
// the rows a thread holds: K with PROX, m without.
template <int NET, int V, bool PROX>
FEDKIT_AGG_KERNEL __launch_bounds__(kBlock)
select_mean_kernel(ClientTable t, const float* __restrict__ z,
                   const int* __restrict__ list, float* __restrict__ znew,
                   float rho, float inv, int K, int m, long long n,
                   float* __restrict__ part) {
  __shared__ float red[4];
  unsigned bits = 0;
  if constexpr (PROX)
    for (int j = 0; j < m; ++j) bits |= 1u << (list[j] & 31);
  const unsigned mask = __builtin_amdgcn_readfirstlane(bits);  // wave-uniform
  float accz = 0.f, acck[PROX ? NET : 1] = {};
  const int tid = threadIdx.x;
  const long long units = n / V;   // whole units; the tail follows the loop
#pragma nounroll
  for (long long u = blockIdx.x * (long long)kBlock + tid; u < units;
       u += (long long)gridDim.x * kBlock)
    mean_unit<NET, V, PROX>(t, z, list, znew, rho, inv, K, m, mask, u * V,
                            accz, acck);
  if constexpr (V > 1) {
    const long long it = units * V + tid;
    if (blockIdx.x == 0 && it < n)
      mean_unit<NET, 1, PROX>(t, z, list, znew, rho, inv, K, m, mask, it,
                              accz, acck);
  }
  float* row = part + (long long)blockIdx.x * (PROX ? 1 + K : 1);
  float r = block_sum(accz, red);
  if (tid == 0) row[0] = r;
  if constexpr (PROX) {
#pragma unroll
    for (int k = 0; k < NET; ++k)
      if (k < K) {
        r = block_sum(acck[k], red);
        if (tid == 0) row[1 + k] = r;
      }
  }
}

struct MeanArgs {
  ClientTable t;
  const float* z;
  const int* list;
  float* znew;
  float rho, inv;
  int K, m;
  long long n;
  int nb;
  float* part;
  hipStream_t stream;
};

template <int NET, bool PROX>
void launch_mean(const MeanArgs& a) {
  hipLaunchKernelGGL((select_mean_kernel<NET, unit_width(NET, PROX), PROX>),
                     dim3(a.nb), dim3(kBlock), 0, a.stream, a.t, a.z, a.list,
                     a.znew, a.rho, a.inv, a.K, a.m, a.n, a.part);
}

template <bool PROX>
void launch_bucket(const MeanArgs& a) {
  switch (bucket_of(PROX ? a.K : a.m)) {
    case 8: return launch_mean<8, PROX>(a);
    case 16: return launch_mean<16, PROX>(a);
    default: return launch_mean<32, PROX>(a);
  }
}

// Gram pass, then the select kernel: D fresh fp32 [K, K]; scores and sel are
// written when q >= 1.  n > 0; the caller holds the device guard.
at::Tensor launch_distances(const ClientTable& t, const at::Tensor& center,
                            int K, int q, int m, float* scores, int* sel) {
  auto D = at::empty({K, K}, center.options());
  hipStream_t stream = fedkit_stream();
  const GramPartials g = launch_gram(t, center, K, stream);
  hipLaunchKernelGGL(krum_select_kernel, dim3(1), dim3(kBlock), 0, stream,
                     g.part.data_ptr<float>(), g.nb, g.KT, K, q, m,
                     D.data_ptr<float>(), scores, sel);
  return D;
}

}  // namespace

// fp32 [K, K] of squared distances sum (xs[i] - xs[j])^2 from the centred
// Gram matrix (see the head of this file); exactly symmetric, zero diagonal,
// non-finite entries +inf.
at::Tensor fedkit_pairwise_sqdist(std::vector<at::Tensor> xs,
                                  const at::Tensor& center) {
  const char* op = "pairwise_sqdist";
  const ClientTable t = check_clients(op, xs, center, center);
  const int K = (int)xs.size();
  const fedkit_mt::DeviceGuard guard(center.device());
  if (center.numel() == 0) return at::zeros({K, K}, center.options());
  return launch_distances(t, center, K, 0, 0, nullptr, nullptr);
}

// One Krum / Multi-Krum round (see the head of this file).  Returns
// {znew, res, sel, D, scores}: znew a fresh fp32 [N]; res as robust_round's;
// sel int32 [K]; D fp32 [K, K]; scores fp32 [K].  mode: 0 fedavg, 1 fedprox.
// Every output is new, so none can alias an operand.
//
// Compiler's kernel-resource-usage figures for gfx950 (256 threads,
// ScratchSize 0 in every variant; 512 VGPRs per SIMD lane):
//   kernel               VGPRs  AGPRs  LDS bytes  waves/SIMD
//   gram_kernel<16>        52      4     33280        4   (LDS bound)
//   gram_kernel<32>        86     16     66560        2   (LDS bound)
//   krum_select_kernel     20      0     16896        8
// select_mean_kernel (16 B LDS); the bucket bounds the rows a thread holds,
// the m selected clients in fedavg mode and all K in fedprox mode:
//             fedavg                      fedprox
//   bucket    unit  VGPRs  waves/SIMD     unit  VGPRs  waves/SIMD
//   <=  8       4     47       8            4     60       7
//   <= 16       4     79       6            4    102       4
//   <= 32       4    143       3            2    118       4
// The sum is written per element: as one conditional vector sum the
// compiler kept the held rows in a single 32-register tuple and copied it
// at every client (176..256 VGPRs, a private segment at 32 rows).
std::vector<at::Tensor> fedkit_krum_round(std::vector<at::Tensor> xs,
                                          const at::Tensor& z,
                                          const at::Tensor& center, double rho,
                                          int64_t mode, int64_t f, int64_t m) {
  const char* op = "krum_round";
  TORCH_CHECK(mode != kAdmm, op, ": there is no robust ADMM round (the duals "
              "have no established robust update); use fedavg or fedprox");
  TORCH_CHECK(mode == kFedAvg || mode == kFedProx, op, ": unknown mode ",
              mode);
  const ClientTable t = check_clients(op, xs, z, center);
  const int K = (int)xs.size();
  TORCH_CHECK(f >= 0 && K - f - 2 >= 1, op, ": f = ", f,
              " must satisfy f >= 0 and K - f - 2 >= 1 for K = ", K);
  TORCH_CHECK(m >= 1 && m <= K, op, ": m = ", m, " must be in 1..K = ", K);
  TORCH_CHECK(mode == kFedAvg || (rho > 0.0 && std::isfinite(rho)), op,
              ": fedprox needs a finite rho > 0, got ", rho);
  const long long n = z.numel();
  const fedkit_mt::DeviceGuard guard(z.device());
  const int cols = mode == kFedAvg ? 1 : 1 + K;
  const auto ints = z.options().dtype(at::kInt);
  auto znew = at::empty({n}, z.options());
  if (n == 0)   // every distance and score is 0: the first m clients
    return {znew, at::zeros({cols}, z.options()),
            at::arange(K, ints).lt(m).to(at::kInt),
            at::zeros({K, K}, z.options()), at::zeros({K}, z.options())};
  auto res = at::empty({cols}, z.options());
  auto scores = at::empty({K}, z.options());
  auto sel = at::empty({2, K}, ints);   // flags, then the ascending list
  auto D = launch_distances(t, center, K, (int)(K - f - 2), (int)m,
                            scores.data_ptr<float>(), sel.data_ptr<int>());
  const bool prox = mode == kFedProx;
  const int V = unit_width(bucket_of(prox ? K : (int)m), prox);
  const int nb = grid_1d((n + V - 1) / V, kBlock, kRedGrid);
  auto part = at::empty({nb, cols}, z.options());
  // the reciprocal torch forms for `znew /= m`: in double, then rounded
  const float inv = (float)(1.0 / (double)m);
  const MeanArgs a = {t, z.data_ptr<float>(), sel.data_ptr<int>() + K,
                      znew.data_ptr<float>(), (float)rho, inv, K, (int)m, n, nb,
                      part.data_ptr<float>(), fedkit_stream()};
  if (mode == kFedAvg) launch_bucket<false>(a);
  else launch_bucket<true>(a);
  fedkit_colsum_finalize(a.part, nb, cols, res.data_ptr<float>(), a.stream);
  return {znew, res, sel[0], D, scores};
}
