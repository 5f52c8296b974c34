// Geometric-median aggregation round (RFA: Pillutla, Kakade and Harchaoui,
// 2022) over K <= 32 client vectors: smoothed Weiszfeld re-weighting of the
// clients, run entirely in Gram space, then the weighted update with the
// round's residuals.
//
//   keep_k  = sum (x_k - z)^2 is finite          K' = number kept
//   r_k     = median distance of kept client k to the other kept clients
//   s       = median of the kept |x_k - z|;  floor = nu s
//   c       = 1 / max(floor, r_k), normalised; then `iters` times
//             d_k = max(floor, |x_k - v|), v = z + sum_j c_j (x_j - z),
//             c_k = (1 / d_k) / sum_j (1 / d_j)
//             (uniform 1 / K' when floor == 0 or K' <= 2; 0 if not kept)
//   znew    = z; += c_k * (x_k - z) for kept k ascending
//   r_z     = sum (z - znew)^2;   fedprox: r_k = sum (rho (x_k - znew))^2
//   (both medians: index (K' - 1) / 2 of the ascending values)
//
// Weiszfeld's iterate stays in the affine span of the clients, so with
// a_k = x_k - z and v = z + sum_j c_j a_j every distance of the iteration is
//   |x_k - v|^2 = G_kk - 2 (G c)_k + c^T G c          G = A A^T
// and the K x N block is read twice in all, whatever `iters` is.  Three
// kernels, no host read between them:
//
// 1. gram_kernel<KT> of gram_common.h around the centre z (design notes at
//    the head of krum.hip).
//
// 2. geomed_solve_kernel, one 256-thread workgroup, all arithmetic in
//    double, no contraction.  G is summed from the partials in workgroup
//    order into LDS as double[32][33]; rows and columns of clients that are
//    not kept (and of rows >= K) are then zeroed, so no later loop meets a
//    NaN.  keep is the finiteness of that double sum of fp32 partials, not
//    of one fp32 sum: a client whose squared norm overflows fp32 only in the
//    full sum (about 1e38..1e40) is kept here and dropped by the torch
//    sequence.  D comes from one triangle of G (exactly symmetric), clamped
//    at 0.
//    The medians are found by rank counting with index tie-break, one
//    (i, j) pair per thread and trip; there is no sort.  One iteration:
//      matvec   8 lanes per row take 4 columns each of (G c)_k and combine
//               them with a 3-step xor shuffle (the adds commute, so the 8
//               lanes hold the same bits); barrier
//      form     thread k < 32 sums c^T G c = sum_j c_j (G c)_j in client
//               order from LDS, forms d_k and 1 / d_k; barrier
//      weights  thread k sums 1 / d in client order and writes c_k; barrier
//    Every sum has a fixed order: the result is the same from run to run.
//    Outputs with ordinary vector stores: c fp32 [K]; kept int32 [2 K + 1]
//    (flags, the ascending list of kept clients padded with -1, their
//    count); d fp32 [K], the floored distances the final c was formed from
//    (|x_k - z| in the uniform case, +inf for a client that is not kept).
//
// 3. weighted_delta_kernel<NET, V, PROX> of weighted_delta.h (design notes
//    at its head), over this round's own c and keep.

#include "weighted_delta.h"

#include <cmath>

namespace {

using namespace fedkit_agg;

enum { kFedAvg = 0, kFedProx = 1, kAdmm = 2 };   // aggregate_round's modes

constexpr int kG = kMaxClients + 1;   // LDS row stride of G and D in doubles

// c, kept and d as described at the head of this file.  part holds nb
// partial Gram matrices of KT x KT; iters >= 1, nu > 0.
FEDKIT_AGG_KERNEL __launch_bounds__(kBlock)
geomed_solve_kernel(const float* __restrict__ part, int nb, int KT, int K,
                    int iters, double nu, float* __restrict__ c_out,
                    int* __restrict__ kept, float* __restrict__ d_out) {
#pragma clang fp contract(off)
  __shared__ double G[kMaxClients][kG];
  __shared__ double D[kMaxClients][kG];
  __shared__ double cw[kMaxClients], Gc[kMaxClients], w[kMaxClients];
  __shared__ double r[kMaxClients];
  __shared__ double s_med;
  __shared__ int keep[kMaxClients];
  const int tid = threadIdx.x;
  // every thread sums KT * KT / 256 entries (1 or 4), as krum_select_kernel
  for (int e = tid; e < kMaxClients * kMaxClients; e += kBlock)
    G[e / kMaxClients][e % kMaxClients] = 0.0;
  __syncthreads();
  for (int e = tid; e < KT * KT; e += kBlock)
    G[e / KT][e % KT] = gram_entry(part, nb, KT, e);
  __syncthreads();
  if (tid < kMaxClients)
    keep[tid] = tid < K && fabs(G[tid][tid]) < (double)INFINITY;
  __syncthreads();
  int Kp = 0, before = 0;
  for (int o = 0; o < kMaxClients; ++o) {
    Kp += keep[o];
    before += o < tid && keep[o];
  }
  const bool mine = tid < kMaxClients && keep[tid];
  if (tid < K) {
    kept[tid] = mine;
    if (mine) kept[K + before] = tid;
    if (tid >= Kp) kept[K + tid] = -1;
  }
  if (tid == 0) kept[2 * K] = Kp;
  // D between kept clients; the rest of G and D is zeroed (those entries are
  // read by no kept pair, so the two do not race)
  for (int e = tid; e < kMaxClients * kMaxClients; e += kBlock) {
    const int i = e / kMaxClients, j = e % kMaxClients;
    double d = 0.0;
    if (keep[i] && keep[j]) {
      const int lo = min(i, j), hi = max(i, j);   // one triangle: D_ij == D_ji
      d = G[lo][lo] + G[hi][hi] - 2.0 * G[lo][hi];
      if (d < 0.0 || i == j) d = 0.0;
    } else {
      G[i][j] = 0.0;
    }
    D[i][j] = d;
  }
  __syncthreads();
  // the medians: the value whose rank (ties to the lower index) is mid
  const int mid = (Kp - 1) / 2;
  for (int e = tid; e < kMaxClients * kMaxClients; e += kBlock) {
    const int i = e / kMaxClients, j = e % kMaxClients;
    if (i == j || !keep[i] || !keep[j]) continue;
    const double d = D[i][j];
    int rank = 0;
    for (int o = 0; o < kMaxClients; ++o) {
      const double v = D[i][o];
      rank += o != i && keep[o] && (v < d || (v == d && o < j));
    }
    if (rank == mid) r[i] = sqrt(d);
  }
  if (mine) {
    const double g = G[tid][tid];
    int rank = 0;
    for (int o = 0; o < kMaxClients; ++o) {
      const double v = G[o][o];
      rank += o != tid && keep[o] && (v < g || (v == g && o < tid));
    }
    if (rank == mid) s_med = sqrt(g);
  }
  __syncthreads();
  const double floor_d = Kp > 0 ? nu * s_med : 0.0;
  if (floor_d == 0.0 || Kp <= 2) {   // workgroup-uniform
    if (tid < K) {
      c_out[tid] = mine ? (float)(1.0 / (double)Kp) : 0.f;
      d_out[tid] = mine ? (float)sqrt(G[tid][tid]) : INFINITY;
    }
    return;
  }
  // the start: c ~ 1 / max(floor, r)
  if (tid < kMaxClients) w[tid] = mine ? 1.0 / fmax(floor_d, r[tid]) : 0.0;
  __syncthreads();
  if (tid < kMaxClients) {
    double sum = 0.0;
    for (int j = 0; j < kMaxClients; ++j) sum = sum + w[j];
    cw[tid] = w[tid] / sum;
  }
  __syncthreads();
  const int row = tid >> 3, col0 = 4 * (tid & 7);
  double dist = 0.0;
  for (int it = 0; it < iters; ++it) {
    double p = 0.0;
#pragma unroll
    for (int q = 0; q < 4; ++q) p = p + G[row][col0 + q] * cw[col0 + q];
    p = p + __shfl_xor(p, 1, kWave);
    p = p + __shfl_xor(p, 2, kWave);
    p = p + __shfl_xor(p, 4, kWave);
    if ((tid & 7) == 0) Gc[row] = p;
    __syncthreads();
    if (tid < kMaxClients) {
      double quad = 0.0;
      for (int j = 0; j < kMaxClients; ++j) quad = quad + cw[j] * Gc[j];
      double sq = (G[tid][tid] - 2.0 * Gc[tid]) + quad;
      if (sq < 0.0) sq = 0.0;
      dist = fmax(floor_d, sqrt(sq));
      w[tid] = mine ? 1.0 / dist : 0.0;
    }
    __syncthreads();
    if (tid < kMaxClients) {
      double sum = 0.0;
      for (int j = 0; j < kMaxClients; ++j) sum = sum + w[j];
      cw[tid] = w[tid] / sum;
    }
    __syncthreads();
  }
  if (tid < K) {
    c_out[tid] = (float)cw[tid];
    d_out[tid] = mine ? (float)dist : INFINITY;
  }
}

}  // namespace

// One geometric-median round (see the head of this file).  Returns
// {znew, res, c, keep, d}: znew a fresh fp32 [N]; res as robust_round's;
// c fp32 [K] the clients' weights; keep int32 [K]; d fp32 [K].  mode: 0
// fedavg, 1 fedprox.  Every output is new, so none can alias an operand.
//
// Compiler's kernel-resource-usage figures for gfx950 (256 threads,
// ScratchSize 0 in every variant; 512 VGPRs per SIMD lane):
//   kernel                 VGPRs  AGPRs  LDS bytes  waves/SIMD
//   gram_kernel<16>          52      4     33280        4   (LDS bound)
//   gram_kernel<32>          86     16     66560        2   (LDS bound)
//   geomed_solve_kernel      50      0     18056        7
// weighted_delta_kernel (16 B LDS); the bucket bounds K in both modes:
//             fedavg                      fedprox
//   bucket    unit  VGPRs  waves/SIMD     unit  VGPRs  waves/SIMD
//   <=  8       4     56       8            4     72       7
//   <= 16       4     96       5            4    122       4
//   <= 32       4    176       2            2    151       3
// The wave-uniform coefficients live in SGPRs next to the row pointers; the
// fedprox variants (all K pointers and coefficients live at once) and the
// solver keep the overflow in VGPR lanes, not in memory.
std::vector<at::Tensor> fedkit_geomed_round(std::vector<at::Tensor> xs,
                                            const at::Tensor& z, double rho,
                                            int64_t mode, int64_t iters,
                                            double nu) {
  const char* op = "geomed_round";
  TORCH_CHECK(mode != kAdmm, op, ": there is no robust ADMM round (the duals "
              "have no established robust update); use fedavg or fedprox");
  TORCH_CHECK(mode == kFedAvg || mode == kFedProx, op, ": unknown mode ",
              mode);
  const ClientTable t = check_clients(op, xs, z, z);
  const int K = (int)xs.size();
  TORCH_CHECK(iters >= 1 && iters <= 1024, op, ": iters = ", iters,
              " must be in 1..1024");
  TORCH_CHECK(nu > 0.0 && std::isfinite(nu), op,
              ": nu must be finite and > 0, got ", nu);
  TORCH_CHECK(mode == kFedAvg || (rho > 0.0 && std::isfinite(rho)), op,
              ": fedprox needs a finite rho > 0, got ", rho);
  const long long n = z.numel();
  const fedkit_mt::DeviceGuard guard(z.device());
  const int cols = mode == kFedAvg ? 1 : 1 + K;
  const auto ints = z.options().dtype(at::kInt);
  auto znew = at::empty({n}, z.options());
  if (n == 0)   // every client is at z: uniform weights
    return {znew, at::zeros({cols}, z.options()),
            at::full({K}, 1.0 / K, z.options()), at::ones({K}, ints),
            at::zeros({K}, z.options())};
  auto res = at::empty({cols}, z.options());
  auto c = at::empty({K}, z.options());
  auto d = at::empty({K}, z.options());
  auto kept = at::empty({2 * K + 1}, ints);   // flags, list, count
  hipStream_t stream = fedkit_stream();
  const GramPartials g = launch_gram(t, z, K, stream);
  hipLaunchKernelGGL(geomed_solve_kernel, dim3(1), dim3(kBlock), 0, stream,
                     g.part.data_ptr<float>(), g.nb, g.KT, K, (int)iters, nu,
                     c.data_ptr<float>(), kept.data_ptr<int>(),
                     d.data_ptr<float>());
  const bool prox = mode == kFedProx;
  const int V = unit_width(bucket_of(K), prox);
  const int nb = grid_1d((n + V - 1) / V, kBlock, kRedGrid);
  auto part = at::empty({nb, cols}, z.options());
  const DeltaArgs a = {t, z.data_ptr<float>(), c.data_ptr<float>(),
                       kept.data_ptr<int>(), znew.data_ptr<float>(),
                       (float)rho, K, n, nb, part.data_ptr<float>(), stream};
  if (prox) launch_bucket<true>(a);
  else launch_bucket<false>(a);
  fedkit_colsum_finalize(a.part, nb, cols, res.data_ptr<float>(), stream);
  return {znew, res, c, kept.slice(0, 0, K), d};
}
