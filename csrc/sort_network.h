// The register sorting network of the coordinate-wise kernels (robust.hip,
// bulyan.hip): floats as uint32 keys in torch.sort's total order, and
// Batcher's odd-even merge sort over constant indices.  The notes on the
// order and on the network are at the head of robust.hip.
#pragma once

#include "agg_common.h"

#include <utility>

namespace fedkit_agg {

__device__ __forceinline__ unsigned key_of(float v) {
  const unsigned b = __float_as_uint(v);
  if ((b & 0x7FFFFFFFu) > 0x7F800000u) return 0xFFFFFFFFu;
  return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}

__device__ __forceinline__ float value_of(unsigned k) {
  return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xFFFFFFFFu));
}

// Batcher's odd-even merge sort for NET inputs as a list of exchanges
// (lo < hi), built at compile time: 5 / 19 / 42 / 63 / 132 / 191 exchanges
// for 4 / 8 / 12 / 16 / 24 / 32 inputs.
struct Network {
  int n;
  unsigned char lo[192], hi[192];
};

template <int NET>
constexpr Network make_network() {
  Network w = {};
  int P = 1;
  while (P < NET) P *= 2;
  for (int p = 1; p < P; p *= 2)
    for (int k = p; k >= 1; k /= 2)
      for (int j = k % p; j + k < P; j += 2 * k)
        for (int i = 0; i < k && i + j + k < P; ++i)
          if ((i + j) / (2 * p) == (i + j + k) / (2 * p) && i + j + k < NET) {
            w.lo[w.n] = (unsigned char)(i + j);
            w.hi[w.n] = (unsigned char)(i + j + k);
            ++w.n;
          }
  return w;
}

template <int NET>
struct Sorter {
  static constexpr Network net = make_network<NET>();

  template <size_t... I>
  static __device__ __forceinline__ void run(unsigned (&key)[NET],
                                             std::index_sequence<I...>) {
    ((void)exchange<net.lo[I], net.hi[I]>(key), ...);
  }
  template <int LO, int HI>
  static __device__ __forceinline__ int exchange(unsigned (&key)[NET]) {
    const unsigned a = key[LO], b = key[HI];
    key[LO] = min(a, b);
    key[HI] = max(a, b);
    return 0;
  }
  static __device__ __forceinline__ void sort(unsigned (&key)[NET]) {
    run(key, std::make_index_sequence<net.n>());
  }
};

}  // namespace fedkit_agg
