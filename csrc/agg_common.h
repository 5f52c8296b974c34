// Shared by the aggregation kernels (consensus.hip, robust.hip, krum.hip,
// geomed.hip, cclip.hip, bulyan.hip): the client table, the aligned 16-byte and unit-wide
// accessors, the workgroup sum and the attribute of kernels whose results
// are compared bit for bit.
#pragma once

#include "fedkit_common.h"

namespace fedkit_agg {

constexpr int kBlock = 256;
constexpr int kRedGrid = 512;   // workgroup cap of the reduction kernels
constexpr int kMaxClients = 32;

typedef __attribute__((ext_vector_type(4))) float f4;

struct ClientTable {              // by value in the kernarg segment, 512 B
  const float* x[kMaxClients];
  float* y[kMaxClients];
};

// kernels whose results are compared bit for bit: no packed fp32 ALU forms
#define FEDKIT_AGG_KERNEL \
  __global__ void __attribute__((target("no-packed-fp32-ops")))

__device__ __forceinline__ bool aligned16(const void* p) {
  return (reinterpret_cast<uintptr_t>(p) & 15) == 0;
}

__device__ __forceinline__ f4 load4(const float* p) {
  if (aligned16(p)) return *reinterpret_cast<const f4*>(p);
  f4 v;
  v[0] = p[0]; v[1] = p[1]; v[2] = p[2]; v[3] = p[3];
  return v;
}

__device__ __forceinline__ void store4(float* p, f4 v) {
  if (aligned16(p)) {
    *reinterpret_cast<f4*>(p) = v;
  } else {
    p[0] = v[0]; p[1] = v[1]; p[2] = v[2]; p[3] = v[3];
  }
}

template <int V>
using fv = float __attribute__((ext_vector_type(V)));

// V consecutive floats at p; one load where p is aligned to the unit
template <int V>
__device__ __forceinline__ fv<V> loadv(const float* p) {
  if ((reinterpret_cast<uintptr_t>(p) & (4 * V - 1)) == 0)
    return *reinterpret_cast<const fv<V>*>(p);
  fv<V> v;
#pragma unroll
  for (int e = 0; e < V; ++e) v[e] = p[e];
  return v;
}

template <int V>
__device__ __forceinline__ void storev(float* p, fv<V> v) {
  if ((reinterpret_cast<uintptr_t>(p) & (4 * V - 1)) == 0) {
    *reinterpret_cast<fv<V>*>(p) = v;
    return;
  }
#pragma unroll
  for (int e = 0; e < V; ++e) p[e] = v[e];
}

// Sum of v over the 256-thread workgroup (NW = 4 waves; 128 threads with
// NW = 2), valid in thread 0.  Wave64 shuffle tree, then the wave sums in
// index order: a fixed order.
template <int NW = 4>
__device__ __forceinline__ float block_sum(float v, float* red /* [4] */) {
  static_assert(NW == 4 || NW == 2, "256- or 128-thread workgroups");
#pragma unroll
  for (int off = 32; off; off >>= 1) v += __shfl_down(v, off, kWave);
  __syncthreads();   // red may still be read from a previous call
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  if constexpr (NW == 2) return red[0] + red[1];
  else return (red[0] + red[1]) + (red[2] + red[3]);
}

}  // namespace fedkit_agg
