// Bulyan aggregation round (El Mhamdi, Guerraoui and Rouault, 2018) over
// K <= 32 client vectors, of which up to f may be Byzantine, K >= 4 f + 3:
// theta = K - 2 f clients are selected by iterated Krum, and per coordinate
// the beta = theta - 2 f selected values closest to their median are averaged.
//
//   D_ij    = sum (x_i - x_j)^2                     non-finite counts as +inf
//   R = all clients; theta times: q = max(1, |R| - f - 2),
//     score_i = sum of the q smallest D_ij, j in R \ {i}, in ascending order,
//     the client of lowest score (ties to the lower index) leaves R for S
//   per coordinate: s = the theta values of S ascending, med = s[mid],
//     mid = (theta - 1) / 2; lo = max(0, mid - beta + 1), go = true;
//     for c = lo .. min(mid, theta - beta) - 1:
//       go &= (s[c + beta] - med) < (med - s[c]);  lo += go
//   znew    = (0 + s[lo] + ... + s[lo + beta - 1]) * inv      inv = 1/beta
//   r_z     = sum (z - znew)^2;   fedprox: r_k = sum (rho (x_k - znew))^2
//
// Three kernels, no host read between them:
//
// 1. gram_kernel<KT> (gram_common.h; notes at the head of krum.hip): the MFMA
//    Gram pass over x_k - c as per-workgroup partials.
//
// 2. bulyan_select_kernel, one workgroup.  The partials are summed in
//    workgroup order in double and D is formed from one triangle, exactly
//    symmetric, as krum_select_kernel does.  Each client's row is then sorted
//    ONCE, by rank counting with the index tie-break, and what is kept is the
//    order of the neighbours j (a byte each), not only the values.  The theta
//    iterations run in LDS over a removed-mask: the thread of a remaining
//    client walks its sorted neighbour list, skips the removed ones and adds
//    the first q distances in double (Krum's score arithmetic), O(K) per row
//    and iteration; the arg-min is a rank count against the other remaining
//    scores with the index tie-break, so exactly one thread removes itself.
//    Three barriers per iteration, at most 96 in all.  With q = 1 two mutually
//    nearest clients share one D entry and tie exactly; D's symmetry makes
//    that tie the same on every path, and the index decides it.
//    It writes D, the picking order, sel and the ascending list of S in the
//    int32 [2][K] shape of krum_select_kernel.
//
// 3. bulyan_window_kernel<NET, V, PROX>: robust_kernel's thread work.  A
//    thread owns a unit of V elements, issues all loads first and then, one
//    element after the other, forms NET uint32 keys (sort_network.h) and
//    sorts them with Batcher's network over constant indices; the keys never
//    leave VGPRs.  fedavg loads the theta listed rows only (the list through
//    scalar loads, as mean_unit does), NET bucketed by theta.  fedprox loads
//    all K rows for the residuals, NET bucketed by K, and an unselected
//    client's key is 0xFFFFFFFF: it sorts past rank theta - 1, where the
//    window never reaches.
//    Median and slide.  mid, beta and theta are kernel arguments, so every
//    bound below is wave-uniform and every register index a constant:
//      med      a chain of uniform selects over the slots;
//      s[c+beta] the key array shifted down by beta with a barrel shifter,
//               one uniform branch per bit of beta around constant-index
//               moves; only slots c < (NET - 1) / 2 of the result are read
//               (c < mid), the moves that feed no such slot are dead code;
//      slide    an unrolled loop over c with the uniform predicate
//               lo0 <= c < min(mid, theta - beta), a per-lane go and lo;
//      sum      a predicated sum over the slots, lo <= r < lo + beta per
//               lane; a slot outside adds +0.0f, which leaves every bit of
//               a sum that started from +0.0f (see mean_unit in krum.hip).
//    A NaN compares false and never enters by sliding.  There are at most
//    2 f slide steps.  The n % V tail is the same code at V = 1.
//
// znew is bitwise the torch sequence `sort(stack(selected), 0)`, the slide as
// vectorised steps, beta in-place adds of gathered ranks into a zero vector,
// `/= beta`: contraction is off, every add is rounded, the division is a
// multiply by the reciprocal formed on the host in double.

#include "gram_common.h"
#include "sort_network.h"

#include <cmath>

namespace {

using namespace fedkit_agg;

enum { kFedAvg = 0, kFedProx = 1, kAdmm = 2 };   // aggregate_round's modes

// One workgroup.  D (fp32 [K, K]) from the nb partial Gram matrices; order
// (int32 [K]): order[t] is the client picked at iteration t < theta, the rest
// -1; sel (int32 [2][K]): sel[0][k] is 1 for the theta picked clients,
// sel[1][0..theta-1] lists them in ascending order, the rest is -1.
FEDKIT_AGG_KERNEL __launch_bounds__(kBlock)
bulyan_select_kernel(const float* __restrict__ part, int nb, int KT, int K,
                     int f, int theta, float* __restrict__ D,
                     int* __restrict__ order, int* __restrict__ sel) {
#pragma clang fp contract(off)
  __shared__ double G[kMaxClients * kMaxClients];
  __shared__ float Dl[kMaxClients][kMaxClients + 1];
  __shared__ unsigned char nbr[kMaxClients][kMaxClients];
  __shared__ float sc[kMaxClients];
  __shared__ int removed[kMaxClients];
  const int tid = threadIdx.x;
  for (int e = tid; e < KT * KT; e += kBlock)
    G[e] = gram_entry(part, nb, KT, e);
  if (tid < kMaxClients) removed[tid] = 0;
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
  __syncthreads();
  // rank of D_ij among client i's K - 1 distances, ties to the lower index:
  // a permutation of 0..K-2, so every slot of nbr[i] is written once
  for (int e = tid; e < K * K; e += kBlock) {
    const int i = e / K, j = e % K;
    if (i == j) continue;
    const float d = Dl[i][j];
    int r = 0;
    for (int o = 0; o < K; ++o) {
      const float w = Dl[i][o];
      r += (o != i) && (w < d || (w == d && o < j));
    }
    nbr[i][r] = (unsigned char)j;
  }
  __syncthreads();
  for (int t = 0; t < theta; ++t) {
    const int q = max(1, K - t - f - 2);   // |R| = K - t
    const bool alive = tid < K && !removed[tid];
    if (alive) {
      double s = 0.0;
      int taken = 0;
      for (int r = 0; r < K - 1 && taken < q; ++r) {
        const int j = nbr[tid][r];
        if (removed[j]) continue;
        s += (double)Dl[tid][j];
        ++taken;
      }
      sc[tid] = (float)s;   // a lone remaining client: 0
    }
    __syncthreads();
    bool won = false;
    if (alive) {
      const float v = sc[tid];   // never NaN: a sum of values in [0, +inf]
      int before = 0;
      for (int o = 0; o < K; ++o)
        before += !removed[o] && (sc[o] < v || (sc[o] == v && o < tid));
      won = before == 0;         // the ranks are a permutation: one thread
    }
    __syncthreads();             // every read of removed[] is done
    if (won) {
      removed[tid] = 1;
      order[t] = tid;
    }
    __syncthreads();
  }
  if (tid >= theta && tid < K) order[tid] = -1;
  if (tid < K) {
    sel[tid] = removed[tid];
    if (tid >= theta) sel[K + tid] = -1;
  }
  if (tid < K && removed[tid]) {
    int pos = 0;
    for (int o = 0; o < tid; ++o) pos += removed[o];
    sel[K + pos] = tid;
  }
}

// What the window needs of the rule, all wave-uniform.
struct Window {
  int theta, beta, mid, lo0, hi0;   // slide steps c = lo0 .. hi0 - 1
};

// One element: the NET keys sorted, the median window found, its mean.
template <int NET>
__device__ __forceinline__ float window_mean(unsigned (&key)[NET],
                                             const Window& w, float inv) {
#pragma clang fp contract(off)
  Sorter<NET>::sort(key);
  float med = 0.f;
#pragma unroll
  for (int r = 0; r < (NET + 1) / 2; ++r)   // mid <= (theta - 1) / 2
    if (r == w.mid) med = value_of(key[r]);
  // up[c] = key[c + beta]: a barrel shifter over the bits of beta
  unsigned up[NET];
#pragma unroll
  for (int c = 0; c < NET; ++c) up[c] = key[c];
#pragma unroll
  for (int b = 1; b < NET; b *= 2)
    if (w.beta & b) {
#pragma unroll
      for (int c = 0; c + b < NET; ++c) up[c] = up[c + b];
    }
  int lo = w.lo0;
  bool go = true;
#pragma unroll
  for (int c = 0; c < (NET - 1) / 2; ++c)   // c < mid
    if (c >= w.lo0 && c < w.hi0) {
      go = go && (value_of(up[c]) - med) < (med - value_of(key[c]));
      lo += go ? 1 : 0;
    }
  float s = 0.f;
#pragma unroll
  for (int r = 0; r < NET; ++r)
    if (r >= w.lo0 && r < w.hi0 + w.beta)
      s = s + ((unsigned)(r - lo) < (unsigned)w.beta ? value_of(key[r]) : 0.f);
  return s * inv;
}

// One unit of V elements at i0: znew, and this thread's residual sums.
// list[0..theta-1] are the selected clients in ascending order.  Without PROX
// only their rows are loaded, slot j holding client list[j]; with PROX all K
// rows, and bit k of mask says whether client k is selected.
template <int NET, int V, bool PROX>
__device__ __forceinline__ void window_unit(
    const ClientTable& t, const float* __restrict__ z,
    const int* __restrict__ list, float* __restrict__ znew, float rho,
    float inv, int K, const Window& w, unsigned mask, long long i0,
    float& accz, float (&acck)[PROX ? NET : 1]) {
#pragma clang fp contract(off)
  // all loads of the unit are issued before the first use
  const int rows = PROX ? K : w.theta;
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
    unsigned key[NET];
#pragma unroll
    for (int k = 0; k < NET; ++k)
      key[k] = k < rows && (!PROX || ((mask >> k) & 1u)) ? key_of(raw[k][e])
                                                          : 0xFFFFFFFFu;
    zn[e] = window_mean<NET>(key, w, inv);
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
// the rows a thread holds: K with PROX, theta without.
template <int NET, int V, bool PROX>
FEDKIT_AGG_KERNEL __launch_bounds__(kBlock)
bulyan_window_kernel(ClientTable t, const float* __restrict__ z,
                     const int* __restrict__ list, float* __restrict__ znew,
                     float rho, float inv, int K, int theta, int beta,
                     long long n, float* __restrict__ part) {
  __shared__ float red[4];
  unsigned bits = 0;
  if constexpr (PROX)
    for (int j = 0; j < theta; ++j) bits |= 1u << (list[j] & 31);
  const unsigned mask = __builtin_amdgcn_readfirstlane(bits);  // wave-uniform
  const int mid = (theta - 1) / 2;
  const Window w = {theta, beta, mid, max(0, mid - beta + 1),
                    min(mid, theta - beta)};
  float accz = 0.f, acck[PROX ? NET : 1] = {};
  const int tid = threadIdx.x;
  const long long units = n / V;   // whole units; the tail follows the loop
#pragma nounroll
  for (long long u = blockIdx.x * (long long)kBlock + tid; u < units;
       u += (long long)gridDim.x * kBlock)
    window_unit<NET, V, PROX>(t, z, list, znew, rho, inv, K, w, mask, u * V,
                              accz, acck);
  if constexpr (V > 1) {
    const long long it = units * V + tid;
    if (blockIdx.x == 0 && it < n)
      window_unit<NET, 1, PROX>(t, z, list, znew, rho, inv, K, w, mask, it,
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

struct WindowArgs {
  ClientTable t;
  const float* z;
  const int* list;
  float* znew;
  float rho, inv;
  int K, theta, beta;
  long long n;
  int nb;
  float* part;
  hipStream_t stream;
};

// The sort buckets of robust.hip without the smallest: theta >= 3.
constexpr int sort_bucket(int rows) {
  return rows <= 8 ? 8 : rows <= 12 ? 12 : rows <= 16 ? 16
         : rows <= 24 ? 24 : 32;
}

// Unit width of a bucket: 16-byte loads wherever that leaves three waves per
// SIMD, else 8-byte loads (table at fedkit_bulyan_round).
constexpr int window_width(int net, bool prox) {
  return prox ? (net > 16 ? 2 : 4) : (net > 24 ? 2 : 4);
}

template <int NET, bool PROX>
void launch_window(const WindowArgs& a) {
  hipLaunchKernelGGL((bulyan_window_kernel<NET, window_width(NET, PROX), PROX>),
                     dim3(a.nb), dim3(kBlock), 0, a.stream, a.t, a.z, a.list,
                     a.znew, a.rho, a.inv, a.K, a.theta, a.beta, a.n, a.part);
}

template <bool PROX>
void launch_bucket(const WindowArgs& a) {
  switch (sort_bucket(PROX ? a.K : a.theta)) {
    case 8: return launch_window<8, PROX>(a);
    case 12: return launch_window<12, PROX>(a);
    case 16: return launch_window<16, PROX>(a);
    case 24: return launch_window<24, PROX>(a);
    default: return launch_window<32, PROX>(a);
  }
}

}  // namespace

// One Bulyan round (see the head of this file).  Returns {znew, res, sel, D,
// order}: znew a fresh fp32 [N]; res as robust_round's; sel int32 [K]; D fp32
// [K, K]; order int32 [K], the picks in picking order, then -1.  mode: 0
// fedavg, 1 fedprox.  Every output is new, so none can alias an operand.
//
// Compiler's kernel-resource-usage figures for gfx950 (256 threads,
// ScratchSize 0 in every variant; 512 VGPRs per SIMD lane):
//   kernel                 VGPRs  LDS bytes  waves/SIMD
//   bulyan_select_kernel     18     13696        8
// (gram_kernel: the table at fedkit_krum_round.)  bulyan_window_kernel (16 B
// LDS); the bucket bounds the rows a thread holds, the theta selected clients
// in fedavg mode and all K in fedprox mode.  A thread holds V x NET loaded
// values, NET keys and the shifted keys the slide reads:
//             fedavg                      fedprox
//   bucket    unit  VGPRs  waves/SIMD     unit  VGPRs  waves/SIMD
//   <=  8       4     55       7            4     75       6
//   <= 12       4     71       7            4    105       4
//   <= 16       4     92       5            4    135       3
//   <= 24       4    132       3            2    143       3
//   <= 32       2    112       4            2    187       2
// Not chosen: unit 4 is 180 VGPRs / 2 waves (fedavg <= 32), 195 / 2 and
// 255 / 2 (fedprox <= 24, <= 32); fedprox <= 32 at unit 1 is 153 / 3 with
// 4-byte loads; fedprox <= 16 at unit 2 is 99 / 4.
std::vector<at::Tensor> fedkit_bulyan_round(std::vector<at::Tensor> xs,
                                            const at::Tensor& z,
                                            const at::Tensor& center,
                                            double rho, int64_t mode,
                                            int64_t f) {
  const char* op = "bulyan_round";
  TORCH_CHECK(mode != kAdmm, op, ": there is no robust ADMM round (the duals "
              "have no established robust update); use fedavg or fedprox");
  TORCH_CHECK(mode == kFedAvg || mode == kFedProx, op, ": unknown mode ",
              mode);
  const ClientTable t = check_clients(op, xs, z, center);
  const int K = (int)xs.size();
  TORCH_CHECK(f >= 0 && K >= 4 * f + 3, op, ": f = ", f,
              " must satisfy f >= 0 and K >= 4 f + 3 for K = ", K);
  TORCH_CHECK(mode == kFedAvg || (rho > 0.0 && std::isfinite(rho)), op,
              ": fedprox needs a finite rho > 0, got ", rho);
  const int theta = K - 2 * (int)f, beta = K - 4 * (int)f;
  const long long n = z.numel();
  const fedkit_mt::DeviceGuard guard(z.device());
  const int cols = mode == kFedAvg ? 1 : 1 + K;
  const auto ints = z.options().dtype(at::kInt);
  auto znew = at::empty({n}, z.options());
  if (n == 0) {   // every distance and score is 0: clients 0..theta-1 in turn
    auto first = at::arange(K, ints);
    return {znew, at::zeros({cols}, z.options()), first.lt(theta).to(at::kInt),
            at::zeros({K, K}, z.options()),
            at::where(first.lt(theta), first, at::full({K}, -1, ints))};
  }
  auto res = at::empty({cols}, z.options());
  auto D = at::empty({K, K}, z.options());
  auto order = at::empty({K}, ints);
  auto sel = at::empty({2, K}, ints);   // flags, then the ascending list
  hipStream_t stream = fedkit_stream();
  const GramPartials g = launch_gram(t, center, K, stream);
  hipLaunchKernelGGL(bulyan_select_kernel, dim3(1), dim3(kBlock), 0, stream,
                     g.part.data_ptr<float>(), g.nb, g.KT, K, (int)f, theta,
                     D.data_ptr<float>(), order.data_ptr<int>(),
                     sel.data_ptr<int>());
  const bool prox = mode == kFedProx;
  const int V = window_width(sort_bucket(prox ? K : theta), prox);
  const int nb = grid_1d((n + V - 1) / V, kBlock, kRedGrid);
  auto part = at::empty({nb, cols}, z.options());
  // the reciprocal torch forms for `znew /= beta`: in double, then rounded
  const float inv = (float)(1.0 / (double)beta);
  const WindowArgs a = {t, z.data_ptr<float>(), sel.data_ptr<int>() + K,
                        znew.data_ptr<float>(), (float)rho, inv, K, theta,
                        beta, n, nb, part.data_ptr<float>(), stream};
  if (prox) launch_bucket<true>(a);
  else launch_bucket<false>(a);
  fedkit_colsum_finalize(a.part, nb, cols, res.data_ptr<float>(), stream);
  return {znew, res, sel[0], D, order};
}
