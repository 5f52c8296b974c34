// Multi-tensor segment tables: the one copy of the mechanism behind
// pack/unpack/axpy, the batched casts (flat_ops.hip), the fused Adam step
// (adam.hip) and the consensus penalty (consensus.hip).
//
// A list of tensors is treated as one flat index space in list order, each
// tensor walked in PHYSICAL (storage) order.  The list is cut into tables
// of at most kMaxTensors tensors; a table travels to the kernel by value
// (kernarg) and holds NP parallel pointer arrays plus prefix offsets into
// the table's slice of the flat space.  The device side maps a flat index
// to (tensor, offset in tensor) with one binary search.
//
// Rule: build_chunks() performs every check over the WHOLE list before it
// returns, so a caller cannot launch on a half-validated list; callers with
// a flat vector run check_flat() on it before their first launch as well.
#pragma once

#include "fedkit_common.h"

#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>

#include <array>
#include <vector>

namespace fedkit_mt {

// launches and allocations go to the operands' device, not the current one
using DeviceGuard = c10::hip::OptionalHIPGuardMasqueradingAsCUDA;

constexpr int kMaxTensors = 48;

// NP parallel pointer arrays: 1 pack/unpack/axpy and penalty, 2 casts
// (src, dst), 4 Adam (param, grad, exp_avg, exp_avg_sq).  NP = 4 is 1.9 KB,
// inside the 4 KB kernarg budget.
template <int NP>
struct SegTable {
  void* ptr[NP][kMaxTensors];
  long long offset[kMaxTensors + 1];  // prefix offsets into the table's slice
  int n;

  template <typename T>
  __host__ __device__ __forceinline__ T* at(int a, int t) const {
    return static_cast<T*>(ptr[a][t]);
  }
};

// Tensor holding flat index i: the last t with offset[t] <= i (zero-length
// tensors are stepped over).  Offsets are sorted; <= 48 entries -> a short,
// mostly wave-uniform loop.
template <int NP>
__device__ __forceinline__ int find_segment(const SegTable<NP>& d,
                                            long long i) {
  int lo = 0, hi = d.n - 1;
  while (lo < hi) {
    int mid = (lo + hi + 1) >> 1;
    if (i >= d.offset[mid]) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// Grid-stride walk over units of V consecutive flat elements, ONE search
// per unit.  A unit inside one tensor calls fast(t, j, i0) once (j = offset
// in tensor t, i0 = flat index of the unit's first element; V elements are
// valid at both).  A unit that straddles a tensor boundary or the tail calls
// slow(t, j, i) per element (<= n + 1 such units per table).
template <int V, int NP, typename Fast, typename Slow>
__device__ __forceinline__ void for_each_unit(const SegTable<NP>& d,
                                              long long total, Fast&& fast,
                                              Slow&& slow) {
  static_assert(V > 0 && (V & (V - 1)) == 0, "V must be a power of two");
  constexpr int kShift = __builtin_ctz(V);
  const long long units = (total + V - 1) >> kShift;
  // HIP workgroups are uniform; the builtin keeps the size in a scalar
  // register, where blockDim.x inside an inlined helper costs two VGPRs
  const long long block = __builtin_amdgcn_workgroup_size_x();
  for (long long u = blockIdx.x * block + threadIdx.x; u < units;
       u += gridDim.x * block) {
    long long i0 = u << kShift;
    int t = find_segment(d, i0);
    if (i0 + V <= d.offset[t + 1]) {
      fast(t, i0 - d.offset[t], i0);
    } else {
      for (long long i = i0; i < i0 + V && i < total; ++i) {
        int tt = find_segment(d, i);
        slow(tt, i - d.offset[tt], i);
      }
    }
  }
}

// One table per <= kMaxTensors tensors; `base` is the chunk's offset into
// the flat index space and `total` its element count (> 0).
template <int NP>
struct Chunk {
  SegTable<NP> d;
  long long base, total;
};

template <int NP>
struct Chunks {
  std::vector<Chunk<NP>> chunks;  // empty-total chunks are dropped
  long long total = 0;
};

// Validates NP parallel tensor lists and cuts them into chunks.  Checked,
// over the whole list, before anything is returned: non-empty lists of equal
// length; every tensor on the GPU and on the first tensor's device; list a
// has dtype dtypes[a]; every tensor non-overlapping and dense; parallel
// tensors agree in numel and in the strides of every dim larger than 1
// (size-1 dims do not move the storage walk, and autograd's layout contract
// leaves them free), so walking the storages linearly pairs the same
// logical elements.
template <int NP>
Chunks<NP> build_chunks(
    const char* op,
    const std::array<const std::vector<at::Tensor>*, NP>& lists,
    const std::array<at::ScalarType, NP>& dtypes) {
  const size_t count = lists[0]->size();
  TORCH_CHECK(count > 0, op, ": empty tensor list");
  for (int a = 1; a < NP; ++a)
    TORCH_CHECK(lists[a]->size() == count, op,
                ": parallel lists differ in length");
  const at::Tensor& first = (*lists[0])[0];
  for (size_t i = 0; i < count; ++i) {
    const at::Tensor& lead = (*lists[0])[i];
    for (int a = 0; a < NP; ++a) {
      const at::Tensor& t = (*lists[a])[i];
      TORCH_CHECK(t.is_cuda() && t.device() == first.device(), op,
                  ": tensor ", i, " of list ", a,
                  " is not on the first tensor's GPU");
      TORCH_CHECK(t.scalar_type() == dtypes[a], op, ": tensor ", i,
                  " of list ", a, " is ", t.scalar_type(), ", expected ",
                  dtypes[a]);
      TORCH_CHECK(t.is_non_overlapping_and_dense(), op, ": tensor ", i,
                  " of list ", a, " is not dense");
      if (a == 0) continue;
      TORCH_CHECK(t.numel() == lead.numel(), op, ": tensor ", i, " of list ",
                  a, " has ", t.numel(), " elements, list 0 has ",
                  lead.numel());
      bool same = t.dim() == lead.dim();
      for (int64_t k = 0; same && k < t.dim(); ++k)
        same = t.size(k) == lead.size(k) &&
               (t.size(k) <= 1 || t.stride(k) == lead.stride(k));
      TORCH_CHECK(same, op, ": tensor ", i, " of list ", a,
                  " differs from list 0 in shape or physical layout");
    }
  }
  Chunks<NP> out;
  size_t idx = 0;
  while (idx < count) {
    Chunk<NP> c;
    c.d.n = 0;
    c.base = out.total;
    while (idx < count && c.d.n < kMaxTensors) {
      c.d.offset[c.d.n] = out.total - c.base;
      for (int a = 0; a < NP; ++a)
        c.d.ptr[a][c.d.n] = (*lists[a])[idx].data_ptr();
      out.total += (*lists[0])[idx].numel();
      ++c.d.n;
      ++idx;
    }
    c.d.offset[c.d.n] = out.total - c.base;
    c.total = out.total - c.base;
    if (c.total > 0) out.chunks.push_back(c);
  }
  return out;
}

// A flat vector paired with a validated list: contiguous, of the given
// dtype, on the list's device, exactly `total` elements.
inline void check_flat(const char* op, const char* name, const at::Tensor& v,
                       const at::Tensor& like, long long total,
                       at::ScalarType dtype = at::kFloat) {
  TORCH_CHECK(v.is_cuda() && v.device() == like.device() &&
              v.scalar_type() == dtype && v.is_contiguous() &&
              v.numel() == total,
              op, ": ", name, " must be a contiguous ", dtype, " vector of ",
              total, " elements on the tensors' device (got ", v.numel(),
              " x ", v.scalar_type(), " on ", v.device(), ")");
}

}  // namespace fedkit_mt
