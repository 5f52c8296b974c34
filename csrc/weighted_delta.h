// The weighted pass shared by geomed.hip and cclip.hip: znew = z + sum over
// the kept clients of c_k (x_k - z), with the round's residuals, from a
// solver's coefficients c and its kept record (flags [K], ascending list
// [K] padded with -1, count).
//
// weighted_delta_kernel<NET, V, PROX>: select_mean_kernel's thread shape (a
// unit of V elements, every load issued before the first use).  The kept
// count is known on the device only, so the bucket NET bounds K in both
// modes; fedavg loads the listed rows only, fedprox all K for the residuals.
// Coefficients, list and mask are read once per wave and held wave-uniform.
// A client that is not kept is skipped by a select of the whole step: the
// sum starts from z, and adding +0.0f to a z element of -0.0f would flip its
// sign bit.  znew is bitwise the torch sequence
// `znew = z.clone(); znew += c[k] * (xs[k] - z)` for kept k ascending.
#pragma once

#include "gram_common.h"

namespace fedkit_agg {

// One unit of V elements at i0: znew, and this thread's residual sums.
// Without PROX slot k holds client list[k] and coefficient ck[k], k < rows =
// the kept count.  With PROX slot k is client k, rows = K, and bit k of mask
// says whether the client is kept; one that is not leaves s as it is.
template <int NET, int V, bool PROX>
__device__ __forceinline__ void delta_unit(
    const ClientTable& t, const float* __restrict__ z,
    const int* __restrict__ list, float* __restrict__ znew, float rho,
    const float (&ck)[NET], int rows, unsigned mask, long long i0,
    float& accz, float (&acck)[PROX ? NET : 1]) {
#pragma clang fp contract(off)
  // all loads of the unit are issued before the first use
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
    float s = zv[e];
#pragma unroll
    for (int k = 0; k < NET; ++k)
      if (k < rows) {
        const float step = s + ck[k] * (raw[k][e] - zv[e]);
        s = (!PROX || ((mask >> k) & 1u)) ? step : s;
      }
    zn[e] = s;
  }
  storev<V>(znew + i0, zn);
  const fv<V> d = zv - zn;
#pragma unroll
  for (int e = 0; e < V; ++e) accz += d[e] * d[e];
  if constexpr (PROX) {
#pragma unroll
    for (int k = 0; k < NET; ++k)
      if (k < rows) {
        const fv<V> yd = rho * (raw[k] - zn);
#pragma unroll
        for (int e = 0; e < V; ++e) acck[k] += yd[e] * yd[e];
      }
  }
}

// znew of the round from the solver's c and kept (flags [K], list [K],
// count).  part[blockIdx.x][0] = partial sum (z - znew)^2 and, with PROX,
// part[blockIdx.x][1 + k] = partial sum (rho (x_k - znew))^2.  K <= NET.
template <int NET, int V, bool PROX>
FEDKIT_AGG_KERNEL __launch_bounds__(kBlock)
weighted_delta_kernel(ClientTable t, const float* __restrict__ z,
                      const float* __restrict__ c,
                      const int* __restrict__ kept, float* __restrict__ znew,
                      float rho, int K, long long n,
                      float* __restrict__ part) {
  __shared__ float red[4];
  const int* list = kept + K;
  const int count = min(__builtin_amdgcn_readfirstlane(kept[2 * K]), K);
  const int rows = PROX ? K : count;
  // once per wave: the coefficients of the held slots and the kept mask
  float ck[NET];
  unsigned bits = 0;
#pragma unroll
  for (int k = 0; k < NET; ++k) {
    ck[k] = 0.f;
    if (k < rows) {
      const int src = PROX ? k : (list[k] & (kMaxClients - 1));
      ck[k] = __int_as_float(
          __builtin_amdgcn_readfirstlane(__float_as_int(c[src])));
      if (PROX && kept[k]) bits |= 1u << k;
    }
  }
  const unsigned mask = __builtin_amdgcn_readfirstlane(bits);
  float accz = 0.f, acck[PROX ? NET : 1] = {};
  const int tid = threadIdx.x;
  const long long units = n / V;   // whole units; the tail follows the loop
#pragma nounroll
  for (long long u = blockIdx.x * (long long)kBlock + tid; u < units;
       u += (long long)gridDim.x * kBlock)
    delta_unit<NET, V, PROX>(t, z, list, znew, rho, ck, rows, mask, u * V,
                             accz, acck);
  if constexpr (V > 1) {
    const long long it = units * V + tid;
    if (blockIdx.x == 0 && it < n)
      delta_unit<NET, 1, PROX>(t, z, list, znew, rho, ck, rows, mask, it,
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

struct DeltaArgs {
  ClientTable t;
  const float* z;
  const float* c;
  const int* kept;
  float* znew;
  float rho;
  int K;
  long long n;
  int nb;
  float* part;
  hipStream_t stream;
};

template <int NET, bool PROX>
void launch_delta(const DeltaArgs& a) {
  hipLaunchKernelGGL((weighted_delta_kernel<NET, unit_width(NET, PROX), PROX>),
                     dim3(a.nb), dim3(kBlock), 0, a.stream, a.t, a.z, a.c,
                     a.kept, a.znew, a.rho, a.K, a.n, a.part);
}

template <bool PROX>
void launch_bucket(const DeltaArgs& a) {
  switch (bucket_of(a.K)) {
    case 8: return launch_delta<8, PROX>(a);
    case 16: return launch_delta<16, PROX>(a);
    default: return launch_delta<32, PROX>(a);
  }
}

}  // namespace fedkit_agg
