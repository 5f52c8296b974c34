// Byzantine-robust aggregation round: coordinate-wise trimmed mean / median
// of K client vectors (Yin et al., 2018) with the round's residuals, in one
// pass over the operands.
//
//   m = K - 2 trim;  per element sort the K client values ascending, drop the
//   trim smallest and the trim largest, and
//     znew = (0 + v_(trim) + ... + v_(K-trim-1)) * inv        inv = 1/m
//     r_z  = sum (z - znew)^2;   fedprox: r_k = sum (rho (x_k - znew))^2
// The median is trim = (K-1)/2: the middle value times 1.0f for odd K, the
// mean of the two middle values for even K.  No second code path.
//
// It is bitwise the torch sequence `sort(stack(xs), 0)`, m in-place adds in
// rank order into a zero vector, `/= m`: contraction is off, the sum starts
// from +0.0f, every add is rounded, and the division is a multiply by the
// reciprocal formed on the host in double (see aggregate_kernel).
//
// Order.  torch.sort's order is total: -inf < finite < +inf < NaN, every NaN
// last whatever its sign bit.  fminf / fmaxf cannot build that: with a NaN
// operand both return the other value, the NaN vanishes, its partner is
// duplicated, and the network stops being a permutation without any error.
// Each float is mapped to a uint32 key instead (all bits flipped if the sign
// is set, else the sign bit flipped; any NaN to 0xFFFFFFFF), compare-exchange
// is integer min / max, and the kept ranks are mapped back.  0xFFFFFFFF maps
// back to a NaN by the same rule, so no rank needs a special case.  -0.0
// ranks below +0.0 here and either way in torch; the sum from +0.0f is the
// same.
//
// Thread work.  A thread owns a unit of V consecutive elements: it issues the
// loads of all K clients (16 bytes at V = 4) and then, one element after the
// other, turns the K values into NET keys, sorts them with a fully unrolled
// Batcher odd-even merge network (constant indices: the keys never leave
// VGPRs), and adds the ranks trim <= r < K - trim, a wave-uniform predicate.
// A lane so holds V x NET loaded values but only NET keys, and the elements'
// networks are independent work for the scheduler.  NET is a template bucket
// chosen on the host from K; K and trim are run-time arguments.  A network
// for NET inputs is the next power of two's without the exchanges that touch
// an index >= NET: those slots would hold the largest key and never move.
// Slots K..NET-1 carry 0xFFFFFFFF.  In fedprox mode the thread keeps the
// loaded values next to the keys for the per-client residual; the unit width
// per bucket is chosen so that this fits (table at fedkit_robust_round).
// The n % V tail elements are done after the unit loop, one thread each, by
// the same code at V = 1.

#include "multi_tensor.h"
#include "sort_network.h"

#include <cmath>

namespace {

using namespace fedkit_agg;

enum { kFedAvg = 0, kFedProx = 1, kAdmm = 2 };   // aggregate_round's modes

// One unit of V elements at i0: znew, and this thread's residual sums.
template <int NET, int V, bool PROX>
__device__ __forceinline__ void robust_unit(
    const ClientTable& t, const float* __restrict__ z,
    float* __restrict__ znew, float rho, float inv, int K, int trim,
    long long i0, float& accz, float (&acck)[PROX ? NET : 1]) {
#pragma clang fp contract(off)
  // all loads of the unit are issued before the first use
  fv<V> raw[NET];
#pragma unroll
  for (int k = 0; k < NET; ++k)
    if (k < K) raw[k] = loadv<V>(t.x[k] + i0);
  const fv<V> zv = loadv<V>(z + i0);
  fv<V> zn;
#pragma unroll
  for (int e = 0; e < V; ++e) {
    unsigned key[NET];
#pragma unroll
    for (int k = 0; k < NET; ++k)
      key[k] = k < K ? key_of(raw[k][e]) : 0xFFFFFFFFu;
    Sorter<NET>::sort(key);
    float s = 0.f;
#pragma unroll
    for (int r = 0; r < NET; ++r)
      if (r >= trim && r < K - trim) s = s + value_of(key[r]);
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
// part[blockIdx.x][1 + k] = partial sum (rho (x_k - znew))^2
template <int NET, int V, bool PROX>
FEDKIT_AGG_KERNEL __launch_bounds__(kBlock)
robust_kernel(ClientTable t, const float* __restrict__ z,
              float* __restrict__ znew, float rho, float inv, int K, int trim,
              long long n, float* __restrict__ part) {
  __shared__ float red[4];
  float accz = 0.f, acck[PROX ? NET : 1] = {};
  const int tid = threadIdx.x;
  const long long units = n / V;   // whole units; the tail follows the loop
  for (long long u = blockIdx.x * (long long)kBlock + tid; u < units;
       u += (long long)gridDim.x * kBlock)
    robust_unit<NET, V, PROX>(t, z, znew, rho, inv, K, trim, u * V, accz,
                              acck);
  if constexpr (V > 1) {
    const long long it = units * V + tid;
    if (blockIdx.x == 0 && it < n)
      robust_unit<NET, 1, PROX>(t, z, znew, rho, inv, K, trim, it, accz,
                                acck);
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

struct RobustArgs {
  ClientTable t;
  const float* z;
  float* znew;
  float rho, inv;
  int K, trim;
  long long n;
  int nb;
  float* part;
  hipStream_t stream;
};

// Unit width of a bucket: 4 floats (16-byte loads) wherever that leaves three
// waves per SIMD; fedprox above 16 clients also holds the loaded values and
// would run one wave, so it takes 2 (table at fedkit_robust_round).
constexpr int unit_width(int net, bool prox) {
  return prox && net > 16 ? 2 : 4;
}

constexpr int bucket_of(int K) {
  return K <= 4 ? 4 : K <= 8 ? 8 : K <= 12 ? 12 : K <= 16 ? 16
         : K <= 24 ? 24 : 32;
}

template <int NET, bool PROX>
void launch_robust(const RobustArgs& a) {
  hipLaunchKernelGGL((robust_kernel<NET, unit_width(NET, PROX), PROX>),
                     dim3(a.nb), dim3(kBlock), 0, a.stream, a.t, a.z, a.znew,
                     a.rho, a.inv, a.K, a.trim, a.n, a.part);
}

template <bool PROX>
void launch_bucket(const RobustArgs& a) {
  switch (bucket_of(a.K)) {
    case 4: return launch_robust<4, PROX>(a);
    case 8: return launch_robust<8, PROX>(a);
    case 12: return launch_robust<12, PROX>(a);
    case 16: return launch_robust<16, PROX>(a);
    case 24: return launch_robust<24, PROX>(a);
    default: return launch_robust<32, PROX>(a);
  }
}

}  // namespace

// One robust aggregation round (see the head of this file).  Returns
// {znew, res}: znew a fresh fp32 [N]; res device fp32, res[0] =
// sum (z - znew)^2 and, in fedprox mode, res[1 + k] =
// sum (rho (xs[k] - znew))^2.  mode: 0 fedavg, 1 fedprox.  Nothing is
// written but znew and res, which are new, so no output can alias an operand.
//
// Compiler's kernel-resource-usage figures for gfx950 (256 threads, 16 B
// LDS, ScratchSize 0 in every variant; 512 VGPRs per SIMD lane).  A thread
// sorts its unit's elements one after the other, so it holds V x NET loaded
// values and NET keys, not V x NET keys:
//             fedavg                      fedprox
//   bucket    unit  VGPRs  waves/SIMD     unit  VGPRs  waves/SIMD
//   K <=  4     4     32       8            4     42       8
//   K <=  8     4     49       7            4     66       7
//   K <= 12     4     66       7            4     92       5
//   K <= 16     4     83       5            4    116       4
//   K <= 24     4    121       4            2    121       4
//   K <= 32     4    150       3            2    160       3
// Not chosen: fedprox at unit 4 is 174 VGPRs / 2 waves (K <= 24) and 256 / 1
// (K <= 32); fedavg K <= 32 at unit 2 is 94 VGPRs / 5 waves.
std::vector<at::Tensor> fedkit_robust_round(std::vector<at::Tensor> xs,
                                            const at::Tensor& z, double rho,
                                            int64_t mode, int64_t trim) {
  const char* op = "robust_round";
  TORCH_CHECK(mode != kAdmm, op, ": there is no robust ADMM round (the duals "
              "have no established robust update); use fedavg or fedprox");
  TORCH_CHECK(mode == kFedAvg || mode == kFedProx, op, ": unknown mode ",
              mode);
  const int K = (int)xs.size();
  TORCH_CHECK(xs.size() >= 1 && xs.size() <= (size_t)kMaxClients, op,
              ": 1..", kMaxClients, " clients, got ", xs.size());
  TORCH_CHECK(trim >= 0 && 2 * trim < K, op, ": trim ", trim,
              " must satisfy 0 <= 2 trim < K = ", K);
  TORCH_CHECK(mode == kFedAvg || (rho > 0.0 && std::isfinite(rho)), op,
              ": fedprox needs a finite rho > 0, got ", rho);
  const long long n = z.numel();
  fedkit_mt::check_flat(op, "z", z, z, n);
  ClientTable t = {};
  for (int k = 0; k < K; ++k) {
    fedkit_mt::check_flat(op, "every x_k", xs[k], z, n);
    t.x[k] = xs[k].data_ptr<float>();
  }
  const fedkit_mt::DeviceGuard guard(z.device());
  const int cols = mode == kFedAvg ? 1 : 1 + K;
  auto znew = at::empty({n}, z.options());
  if (n == 0) return {znew, at::zeros({cols}, z.options())};
  auto res = at::empty({cols}, z.options());
  const int V = unit_width(bucket_of(K), mode == kFedProx);
  const int nb = grid_1d((n + V - 1) / V, kBlock, kRedGrid);
  auto part = at::empty({nb, cols}, z.options());
  // the reciprocal torch forms for `znew /= m`: in double, then rounded
  const float inv = (float)(1.0 / (double)(K - 2 * trim));
  const RobustArgs a = {t, z.data_ptr<float>(), znew.data_ptr<float>(),
                        (float)rho, inv, K, (int)trim, n, nb,
                        part.data_ptr<float>(), fedkit_stream()};
  if (mode == kFedAvg) launch_bucket<false>(a);
  else launch_bucket<true>(a);
  fedkit_colsum_finalize(a.part, nb, cols, res.data_ptr<float>(), a.stream);
  return {znew, res};
}
