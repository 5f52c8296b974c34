// Centred-clipping aggregation round (Karimireddy, He and Jaggi, 2021) with
// bucketing (the same authors, 2022) over K <= 32 client vectors: the clients
// are averaged in groups of s, the group means are clipped towards the old
// consensus z for `iters` rounds, run entirely in Gram space, then the
// weighted update with the round's residuals.
//
//   keep_k  = sum (x_k - z)^2 is finite          K' = number kept
//   buckets   perm[0..K-1] without the clients that are not kept, cut into
//             consecutive groups of s (the last may be smaller);
//             B = ceil(K' / s);  u_b = mean of a_k = x_k - z over bucket b
//   tau     = the argument if > 0, else the median of the |u_b| (index
//             (B - 1) / 2 of the ascending values)
//   c       = 0 in R^B; then `iters` times
//             dist_b = |u_b - sum_j c_j u_j|
//             s_b    = tau / dist_b if dist_b > tau else 1
//             c_b    = c_b (1 - S / B) + s_b / B,  S = sum_b s_b
//             (v <- v + (1 / B) sum_b s_b (u_b - v) in coefficients)
//   w_k     = c_b(k) / |bucket b(k)| for kept k, 0 otherwise
//   znew    = z; += w_k * (x_k - z) for kept k ascending
//   r_z     = sum (z - znew)^2;   fedprox: r_k = sum (rho (x_k - znew))^2
//
// The clip iterate stays in the affine span of the clients and bucketing is a
// linear map on them (u = Bm a, Bm the B x K matrix of the bucket means), so
// with G = A A^T and Gb = Bm G Bm^T every distance of the iteration is
//   |u_b - v|^2 = Gb_bb - 2 (Gb c)_b + c^T Gb c
// and the K x N block is read twice in all, whatever `iters` and s are.  The
// difference of nearly equal terms loses accuracy only where a bucket is
// close to the iterate, and there s_b is exactly 1: no floor is needed.
// Three kernels, no host read between them:
//
// 1. gram_kernel<KT> of gram_common.h around the centre z (design notes at
//    the head of krum.hip).
//
// 2. cclip_solve_kernel, one 256-thread workgroup, all arithmetic in double,
//    no contraction.  G is summed from the partials in workgroup order into
//    LDS as double[32][33] and keep is derived from its diagonal, both as in
//    geomed_solve_kernel; rows and columns of clients that are not kept are
//    zeroed, so no later loop meets a NaN.
//    The bucket map is built on the device: thread t < K holds perm[t] and,
//    if that client is kept, counts the kept entries of perm before t (a
//    prefix count over LDS, no sort); its bucket is that rank / s.
//    Gb comes from two staged products in the matvec's thread layout (8
//    lanes per row, 4 columns per lane): first H = G Bm^T, row i of which is
//    the sums of G_i. over each bucket's members in client order, divided by
//    the bucket's size; then Gb = Bm H, row a of which is the sum of the
//    rows of H over bucket a's members, divided likewise.  That is
//    2 * 32 * 32 * 32 multiply-free adds, not the K^4 of the definition.
//    Rows and columns >= B of Gb are zero.
//    The median of sqrt(Gb_bb) is found by rank counting with index
//    tie-break.  One iteration:
//      matvec   8 lanes per row take 4 columns each of (Gb c)_b and combine
//               them with a 3-step xor shuffle (the adds commute, so the 8
//               lanes hold the same bits); barrier
//      form     thread b < 32 sums c^T Gb c = sum_j c_j (Gb c)_j in bucket
//               order from LDS, forms dist_b (the square clamped at 0) and
//               s_b; barrier
//      update   thread b sums S in bucket order and updates c_b; barrier
//    Every sum has a fixed order: the result is the same from run to run.
//    Outputs with ordinary vector stores: w fp32 [K]; kept int32 [2 K + 1]
//    (flags, the ascending list of kept clients padded with -1, their
//    count); d fp32 [K], the last dist of the client's bucket (+inf for a
//    client that is not kept); tau_used fp32 [1].
//
// 3. weighted_delta_kernel<NET, V, PROX> of weighted_delta.h, over this
//    round's own w and keep.  The weights need not sum to 1.

#include "weighted_delta.h"

#include <cmath>

namespace {

using namespace fedkit_agg;

enum { kFedAvg = 0, kFedProx = 1, kAdmm = 2 };   // aggregate_round's modes

constexpr int kG = kMaxClients + 1;   // LDS row stride of G, H, Gb in doubles

// w, kept, d and tau_used as described at the head of this file.  part holds
// nb partial Gram matrices of KT x KT (nb = 0: every client is at z);
// iters >= 1, tau >= 0 (0: the median radius), 1 <= s <= K, perm int32 [K].
FEDKIT_AGG_KERNEL __launch_bounds__(kBlock)
cclip_solve_kernel(const float* __restrict__ part, int nb, int KT, int K,
                   int iters, double tau_arg, int s,
                   const int* __restrict__ perm, float* __restrict__ w_out,
                   int* __restrict__ kept, float* __restrict__ d_out,
                   float* __restrict__ tau_out) {
#pragma clang fp contract(off)
  __shared__ double G[kMaxClients][kG];    // G, after the contraction Gb
  __shared__ double H[kMaxClients][kG];    // G Bm^T
  __shared__ double cw[kMaxClients], Gc[kMaxClients], sv[kMaxClients];
  __shared__ double distb[kMaxClients];
  __shared__ double tau_s;
  __shared__ int keep[kMaxClients], pk[kMaxClients];
  __shared__ int bof[kMaxClients], bsize[kMaxClients];
  const int tid = threadIdx.x;
  // every thread sums KT * KT / 256 entries (1 or 4), as krum_select_kernel
  for (int e = tid; e < kMaxClients * kMaxClients; e += kBlock)
    G[e / kMaxClients][e % kMaxClients] = 0.0;
  __syncthreads();
  for (int e = tid; e < KT * KT; e += kBlock)
    G[e / KT][e % KT] = gram_entry(part, nb, KT, e);
  __syncthreads();
  if (tid < kMaxClients) {
    keep[tid] = tid < K && fabs(G[tid][tid]) < (double)INFINITY;
    // a client index out of range counts as one that is not kept
    const int p = tid < K ? perm[tid] : -1;
    pk[tid] = p >= 0 && p < K ? p : -1;
    bof[tid] = -1;
    cw[tid] = 0.0;
    distb[tid] = 0.0;
  }
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
  const int B = (Kp + s - 1) / s;   // workgroup-uniform
  if (B == 0) {
    if (tid < K) {
      w_out[tid] = 0.f;
      d_out[tid] = INFINITY;
    }
    if (tid == 0) tau_out[0] = 0.f;
    return;
  }
  // the bucket map: the rank of this thread's entry among the kept entries
  // of perm, and the sizes (only the last bucket can be short)
  if (tid < kMaxClients) {
    const int cl = pk[tid];
    if (cl >= 0 && keep[cl]) {
      int rank = 0;
      for (int o = 0; o < tid; ++o) rank += pk[o] >= 0 && keep[pk[o]];
      bof[cl] = rank / s;
    }
    bsize[tid] = tid < B ? min(s, Kp - tid * s) : 0;
  }
  for (int e = tid; e < kMaxClients * kMaxClients; e += kBlock) {
    const int i = e / kMaxClients, j = e % kMaxClients;
    if (!(keep[i] && keep[j])) G[i][j] = 0.0;
  }
  __syncthreads();
  // Gb = Bm (G Bm^T): two staged products, 8 lanes per row and 4 bucket
  // columns per lane.  H[i][b] = mean over the clients j of bucket b,
  // ascending, of G[i][j] ...
  const int row = tid >> 3, col0 = 4 * (tid & 7);
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  for (int j = 0; j < kMaxClients; ++j) {
    const double g = G[row][j];
    const int b = bof[j];
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (b == col0 + q) acc[q] = acc[q] + g;
  }
#pragma unroll
  for (int q = 0; q < 4; ++q)
    H[row][col0 + q] = acc[q] / (double)max(bsize[col0 + q], 1);
  __syncthreads();
  // ... and Gb[a][b] = mean over the clients i of bucket a of H[i][b], which
  // replaces G (rows and columns >= B come out 0)
#pragma unroll
  for (int q = 0; q < 4; ++q) acc[q] = 0.0;
  for (int i = 0; i < kMaxClients; ++i)
    if (bof[i] == row) {
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[q] = acc[q] + H[i][col0 + q];
    }
#pragma unroll
  for (int q = 0; q < 4; ++q)
    G[row][col0 + q] = acc[q] / (double)max(bsize[row], 1);
  __syncthreads();
  // the radius: the value whose rank (ties to the lower index) is mid
  const bool bucket = tid < B;
  if (tau_arg > 0.0) {
    if (tid == 0) tau_s = tau_arg;
  } else if (bucket) {
    const int mid = (B - 1) / 2;
    const double g = G[tid][tid];
    int rank = 0;
    for (int o = 0; o < B; ++o) {
      const double v = G[o][o];
      rank += o != tid && (v < g || (v == g && o < tid));
    }
    if (rank == mid) tau_s = sqrt(g < 0.0 ? 0.0 : g);
  }
  __syncthreads();
  const double tau = tau_s;
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
      const double dist = sqrt(sq);
      distb[tid] = dist;
      sv[tid] = !bucket ? 0.0 : dist > tau ? tau / dist : 1.0;
    }
    __syncthreads();
    if (tid < kMaxClients) {
      double S = 0.0;
      for (int j = 0; j < kMaxClients; ++j) S = S + sv[j];
      if (bucket)
        cw[tid] = cw[tid] * (1.0 - S / (double)B) + sv[tid] / (double)B;
    }
    __syncthreads();
  }
  if (tid < K) {
    // a kept client is outside 0..B-1 only if perm is no permutation
    const int b = mine && bof[tid] < B ? bof[tid] : -1;
    w_out[tid] = b >= 0 ? (float)(cw[b] / (double)bsize[b]) : 0.f;
    d_out[tid] = b >= 0 ? (float)distb[b] : INFINITY;
  }
  if (tid == 0) tau_out[0] = (float)tau;
}

}  // namespace

// One centred-clipping round (see the head of this file).  Returns
// {znew, res, w, keep, d, tau_used}: znew a fresh fp32 [N]; res as
// robust_round's; w fp32 [K] the clients' weights; keep int32 [K]; d fp32
// [K]; tau_used fp32 [1].  mode: 0 fedavg, 1 fedprox.  perm is int32 [K] on
// z's device and holds a permutation of 0..K-1 (the caller's to check: the
// round reads nothing back).  Every output is new, so none can alias an
// operand.
//
// Compiler's kernel-resource-usage figures for gfx950 (256 threads,
// ScratchSize 0; 512 VGPRs per SIMD lane):
//   kernel                 VGPRs  AGPRs  LDS bytes  waves/SIMD
//   cclip_solve_kernel       44      0     18440        8
// gram_kernel and weighted_delta_kernel: the tables at fedkit_geomed_round.
std::vector<at::Tensor> fedkit_cclip_round(std::vector<at::Tensor> xs,
                                           const at::Tensor& z, double rho,
                                           int64_t mode, int64_t iters,
                                           double tau, int64_t bucket,
                                           const at::Tensor& perm) {
  const char* op = "cclip_round";
  TORCH_CHECK(mode != kAdmm, op, ": there is no robust ADMM round (the duals "
              "have no established robust update); use fedavg or fedprox");
  TORCH_CHECK(mode == kFedAvg || mode == kFedProx, op, ": unknown mode ",
              mode);
  const ClientTable t = check_clients(op, xs, z, z);
  const int K = (int)xs.size();
  TORCH_CHECK(iters >= 1 && iters <= 1024, op, ": iters = ", iters,
              " must be in 1..1024");
  TORCH_CHECK(tau >= 0.0 && std::isfinite(tau), op,
              ": tau must be finite and >= 0 (0: the median radius), got ",
              tau);
  TORCH_CHECK(bucket >= 1 && bucket <= K, op, ": bucket = ", bucket,
              " must be in 1..K = ", K);
  TORCH_CHECK(perm.device() == z.device() && perm.scalar_type() == at::kInt &&
              perm.dim() == 1 && perm.numel() == K && perm.is_contiguous(),
              op, ": perm must be a contiguous int32 [", K,
              "] tensor on z's device");
  TORCH_CHECK(mode == kFedAvg || (rho > 0.0 && std::isfinite(rho)), op,
              ": fedprox needs a finite rho > 0, got ", rho);
  const long long n = z.numel();
  const fedkit_mt::DeviceGuard guard(z.device());
  const int cols = mode == kFedAvg ? 1 : 1 + K;
  const auto ints = z.options().dtype(at::kInt);
  auto znew = at::empty({n}, z.options());
  auto res = at::empty({cols}, z.options());
  auto w = at::empty({K}, z.options());
  auto d = at::empty({K}, z.options());
  auto tau_used = at::empty({1}, z.options());
  auto kept = at::empty({2 * K + 1}, ints);   // flags, list, count
  hipStream_t stream = fedkit_stream();
  // n == 0: every client is at z; the solver runs on G = 0 (no partials)
  GramPartials g = {at::Tensor(), 0, K <= 16 ? 16 : 32};
  if (n > 0) g = launch_gram(t, z, K, stream);
  hipLaunchKernelGGL(cclip_solve_kernel, dim3(1), dim3(kBlock), 0, stream,
                     n > 0 ? g.part.data_ptr<float>() : nullptr, g.nb, g.KT,
                     K, (int)iters, tau, (int)bucket, perm.data_ptr<int>(),
                     w.data_ptr<float>(), kept.data_ptr<int>(),
                     d.data_ptr<float>(), tau_used.data_ptr<float>());
  if (n == 0)
    return {znew, at::zeros({cols}, z.options()), w, kept.slice(0, 0, K), d,
            tau_used};
  const bool prox = mode == kFedProx;
  const int V = unit_width(bucket_of(K), prox);
  const int nb = grid_1d((n + V - 1) / V, kBlock, kRedGrid);
  auto part = at::empty({nb, cols}, z.options());
  const DeltaArgs a = {t, z.data_ptr<float>(), w.data_ptr<float>(),
                       kept.data_ptr<int>(), znew.data_ptr<float>(),
                       (float)rho, K, n, nb, part.data_ptr<float>(), stream};
  if (prox) launch_bucket<true>(a);
  else launch_bucket<false>(a);
  fedkit_colsum_finalize(a.part, nb, cols, res.data_ptr<float>(), stream);
  return {znew, res, w, kept.slice(0, 0, K), d, tau_used};
}
