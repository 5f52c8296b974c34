// Multi-tensor flat pack/unpack/axpy — the federation/optimizer data plane.
// The reference does these as Python loops of per-tensor copies
// (simple_utils.py:47-77, lbfgsnew.py:81-121); here ONE kernel covers up to
// 48 tensors per launch via a descriptor table passed by kernel argument
// (fits the 4 KB kernarg budget), grid-stride over the total element count.
// fp32 only (parameters, gradients and federation vectors are fp32 master).

#include "multi_tensor.h"

namespace {

using fedkit_mt::DeviceGuard;
using fedkit_mt::find_segment;
using fedkit_mt::for_each_unit;
using fedkit_mt::SegTable;

// flat[off_t + j] = tensor_t[j]
__global__ void pack_kernel(SegTable<1> d, float* __restrict__ flat,
                            long long total) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
       i < total; i += (long long)gridDim.x * blockDim.x) {
    int t = find_segment(d, i);
    flat[i] = d.at<const float>(0, t)[i - d.offset[t]];
  }
}

// tensor_t[j] = flat[off_t + j]
__global__ void unpack_kernel(SegTable<1> d, const float* __restrict__ flat,
                              long long total) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
       i < total; i += (long long)gridDim.x * blockDim.x) {
    int t = find_segment(d, i);
    d.at<float>(0, t)[i - d.offset[t]] = flat[i];
  }
}

// tensor_t[j] += alpha * flat[off_t + j]   (LBFGS _add_grad / axpy)
__global__ void axpy_kernel(SegTable<1> d, const float* __restrict__ flat,
                            float alpha, long long total) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
       i < total; i += (long long)gridDim.x * blockDim.x) {
    int t = find_segment(d, i);
    d.at<float>(0, t)[i - d.offset[t]] += alpha * flat[i];
  }
}

enum class Op { Pack, Unpack, Axpy };

void run_flat_op(const char* name, const std::vector<at::Tensor>& tensors,
                 const at::Tensor& flat, Op op, float alpha) {
  auto cs = fedkit_mt::build_chunks<1>(name, {&tensors}, {at::kFloat});
  fedkit_mt::check_flat(name, "flat", flat, tensors[0], cs.total);
  const DeviceGuard guard(tensors[0].device());
  auto stream = fedkit_stream();
  for (const auto& c : cs.chunks) {
    float* f = flat.data_ptr<float>() + c.base;
    int grid = grid_1d(c.total, 256);
    switch (op) {
      case Op::Pack:
        hipLaunchKernelGGL(pack_kernel, dim3(grid), dim3(256), 0, stream,
                           c.d, f, c.total);
        break;
      case Op::Unpack:
        hipLaunchKernelGGL(unpack_kernel, dim3(grid), dim3(256), 0, stream,
                           c.d, (const float*)f, c.total);
        break;
      case Op::Axpy:
        hipLaunchKernelGGL(axpy_kernel, dim3(grid), dim3(256), 0, stream,
                           c.d, (const float*)f, alpha, c.total);
        break;
    }
  }
}

}  // namespace

void fedkit_pack_params(std::vector<at::Tensor> tensors, at::Tensor flat) {
  run_flat_op("pack_params", tensors, flat, Op::Pack, 0.f);
}

void fedkit_unpack_params(at::Tensor flat, std::vector<at::Tensor> tensors) {
  run_flat_op("unpack_params", tensors, flat, Op::Unpack, 0.f);
}

void fedkit_add_flat_params(std::vector<at::Tensor> tensors, at::Tensor flat,
                            double alpha) {
  run_flat_op("add_flat_params", tensors, flat, Op::Axpy, (float)alpha);
}

// ------------------------------------------------- L-BFGS fused multi-ops
// The two-loop recursion's 3n+1 separate torch dots each cost a launch AND
// a device->host sync (lbfgsnew.py:588-659 equivalent).  fedkit instead
// keeps the small Gram matrices (S^T Y, Y^T Y) on the host and refreshes
// them with ONE fused pass per history update: multi_dot computes x . v_i
// for up to 24 history vectors in a single read of x (partials slab +
// wave-per-column finalize, same shape as the BN stage 2), and lincomb
// materializes d = c_g * g + sum c_i v_i in one pass.  One sync per
// step() iteration instead of ~21.

namespace {

constexpr int kMaxVecs = 24;

struct VecPack {
  const float* p[kMaxVecs];
  int n;
};

struct CoefPack {
  const float* p[kMaxVecs];
  float c[kMaxVecs];
  int n;
};

// partials[b][v] = block b's partial dot of x . p[v]
__global__ void multi_dot_kernel(VecPack vp, const float* __restrict__ x,
                                 long long total,
                                 float* __restrict__ part /* [nb][nvec] */) {
  __shared__ float red[256];
  float acc[kMaxVecs] = {};
  long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
       i < total; i += stride) {
    float xv = x[i];
    for (int v = 0; v < vp.n; ++v) acc[v] += xv * vp.p[v][i];
  }
  for (int v = 0; v < vp.n; ++v) {
    __syncthreads();
    red[threadIdx.x] = acc[v];
    __syncthreads();
    for (int off = 128; off; off >>= 1) {
      if (threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
      __syncthreads();
    }
    if (threadIdx.x == 0) part[(long long)blockIdx.x * vp.n + v] = red[0];
  }
}

// out[c] = sum_r part[r][c] — one wave per column, rows in a fixed order
// (deterministic: no atomics).  The one finalize of every partials slab:
// multi_dot here, the penalty / ADMM / BB reductions in consensus.hip.
__global__ void colsum_finalize_kernel(const float* __restrict__ part,
                                       int rows, int cols,
                                       float* __restrict__ out) {
  int c = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  int lane = threadIdx.x & 63;
  if (c >= cols) return;
  float s = 0.f;
  for (int r = lane; r < rows; r += 64) s += part[(long long)r * cols + c];
#pragma unroll
  for (int off = 32; off; off >>= 1) s += __shfl_down(s, off, kWave);
  if (lane == 0) out[c] = s;
}

// out[i] = cg * g[i] + sum_v c[v] * p[v][i]
__global__ void lincomb_kernel(CoefPack cp, const float* __restrict__ g,
                               float cg, float* __restrict__ out,
                               long long total) {
  long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
       i < total; i += stride) {
    float s = cg * g[i];
    for (int v = 0; v < cp.n; ++v) s += cp.c[v] * cp.p[v][i];
    out[i] = s;
  }
}

}  // namespace

void fedkit_colsum_finalize(const float* part, int rows, int cols, float* out,
                            hipStream_t stream) {
  hipLaunchKernelGGL(colsum_finalize_kernel, dim3((cols + 3) / 4), dim3(256),
                     0, stream, part, rows, cols, out);
}

// returns a DEVICE fp32 tensor [len(vecs)] of dots x . vecs[i]; the caller
// syncs once with .cpu() when it needs the scalars
at::Tensor fedkit_multi_dot(std::vector<at::Tensor> vecs,
                            const at::Tensor& x) {
  TORCH_CHECK(!vecs.empty() && (int)vecs.size() <= kMaxVecs,
              "multi_dot supports 1..", kMaxVecs, " vectors");
  TORCH_CHECK(x.scalar_type() == at::kFloat && x.is_contiguous(),
              "multi_dot: x must be contiguous fp32");
  VecPack vp;
  vp.n = (int)vecs.size();
  long long total = x.numel();
  for (int i = 0; i < vp.n; ++i) {
    TORCH_CHECK(vecs[i].scalar_type() == at::kFloat &&
                vecs[i].is_contiguous() && vecs[i].numel() == total,
                "multi_dot: vecs must be contiguous fp32 of x's length");
    vp.p[i] = vecs[i].data_ptr<float>();
  }
  auto stream = fedkit_stream();
  int nb = grid_1d(total, 256, 512);
  auto part = at::empty({nb, vp.n}, x.options());
  auto out = at::empty({vp.n}, x.options());
  hipLaunchKernelGGL(multi_dot_kernel, dim3(nb), dim3(256), 0, stream, vp,
                     x.data_ptr<float>(), total, part.data_ptr<float>());
  fedkit_colsum_finalize(part.data_ptr<float>(), nb, vp.n,
                         out.data_ptr<float>(), stream);
  return out;
}

// out = cg * g + sum coeffs[i] * vecs[i]   (fused direction build)
at::Tensor fedkit_lincomb(const at::Tensor& g, double cg,
                          std::vector<at::Tensor> vecs,
                          std::vector<double> coeffs) {
  TORCH_CHECK(vecs.size() == coeffs.size() && (int)vecs.size() <= kMaxVecs,
              "lincomb: vecs/coeffs mismatch or too many");
  TORCH_CHECK(g.scalar_type() == at::kFloat && g.is_contiguous(),
              "lincomb: g must be contiguous fp32");
  CoefPack cp;
  cp.n = (int)vecs.size();
  long long total = g.numel();
  for (int i = 0; i < cp.n; ++i) {
    TORCH_CHECK(vecs[i].scalar_type() == at::kFloat &&
                vecs[i].is_contiguous() && vecs[i].numel() == total,
                "lincomb: vecs must be contiguous fp32 of g's length");
    cp.p[i] = vecs[i].data_ptr<float>();
    cp.c[i] = (float)coeffs[i];
  }
  auto out = at::empty_like(g);
  hipLaunchKernelGGL(lincomb_kernel, dim3(grid_1d(total, 256)), dim3(256), 0,
                     fedkit_stream(), cp, g.data_ptr<float>(), (float)cg,
                     out.data_ptr<float>(), total);
  return out;
}

// --------------------------------------------------- batched weight casts
// In a full-model training step every FedConv2d pays one fp32->bf16 cast
// kernel forward and one bf16->fp32 grad cast backward (~40 launches,
// ~200 us/step on ResNet18).  One segment-table kernel covers all of them
// per direction (one launch per 48 pairs); both sides are traversed flat,
// and build_chunks() checks that each dst has its src's physical layout.

namespace {

// 8 elements per unit (guide G13: 16-B/lane traffic): vector loads/stores
// on the in-tensor fast path, per-element fallback only for units
// straddling a tensor boundary.  The scalar original measured 68 us for
// the ResNet18 grad-cast sweep — pure search+scalar-store overhead.
template <typename S, typename D>
__global__ void cast_kernel(SegTable<2> d, long long total) {
  for_each_unit<8>(
      d, total,
      [&](int t, long long j, long long) {
        S in[8];
        D out[8];
        __builtin_memcpy(in, d.at<const S>(0, t) + j, sizeof(in));
#pragma unroll
        for (int k = 0; k < 8; ++k) from_f32(to_f32(in[k]), out[k]);
        __builtin_memcpy(d.at<D>(1, t) + j, out, sizeof(out));
      },
      [&](int t, long long j, long long) {
        from_f32(to_f32(d.at<const S>(0, t)[j]), d.at<D>(1, t)[j]);
      });
}

template <typename S, typename D>
void run_cast(const char* name, const std::vector<at::Tensor>& srcs,
              at::ScalarType src_dtype, const std::vector<at::Tensor>& dsts,
              at::ScalarType dst_dtype) {
  auto cs = fedkit_mt::build_chunks<2>(name, {&srcs, &dsts},
                                       {src_dtype, dst_dtype});
  const DeviceGuard guard(srcs[0].device());
  auto stream = fedkit_stream();
  for (const auto& c : cs.chunks)
    hipLaunchKernelGGL((cast_kernel<S, D>), dim3(grid_1d(c.total, 256)),
                       dim3(256), 0, stream, c.d, c.total);
}

}  // namespace

void fedkit_cast_f32_to_bf16(std::vector<at::Tensor> srcs,
                             std::vector<at::Tensor> dsts) {
  run_cast<float, __hip_bfloat16>("cast_f32_to_bf16", srcs, at::kFloat, dsts,
                                  at::kBFloat16);
}

void fedkit_cast_bf16_to_f32(std::vector<at::Tensor> srcs,
                             std::vector<at::Tensor> dsts) {
  run_cast<__hip_bfloat16, float>("cast_bf16_to_f32", srcs, at::kBFloat16,
                                  dsts, at::kFloat);
}

// ------------------------------------------------- fused Welford update
// LBFGS batch mode, new-minibatch statistics (SURVEY §2a "Online grad
// mean/variance (Welford) ... fused into the flat-grad kernel"; reference
// lbfgsnew.py:600-615).  One kernel replaces 2 clones + 2 axpys +
// 1 addcmul + 1 sum (~6 launches + 2 allocations):
//   d_old = g - avg;  avg += d_old/n;  d_new = g - avg;
//   avg_sq += d_new * d_old;  out = sum(avg_sq)
namespace {
__global__ void welford_update_kernel(const float* __restrict__ g,
                                      float* __restrict__ avg,
                                      float* __restrict__ avg_sq,
                                      float inv_n,
                                      float* __restrict__ out,
                                      long long n) {
  float acc = 0.f;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
       i < n; i += (long long)gridDim.x * blockDim.x) {
    float gi = g[i];
    float d_old = gi - avg[i];
    float a_new = avg[i] + d_old * inv_n;
    avg[i] = a_new;
    float sq = avg_sq[i] + (gi - a_new) * d_old;
    avg_sq[i] = sq;
    acc += sq;
  }
  for (int off = 32; off > 0; off >>= 1)
    acc += __shfl_xor(acc, off, 64);
  if ((threadIdx.x & 63) == 0) atomicAdd(out, acc);
}
}  // namespace

at::Tensor fedkit_welford_update(const at::Tensor& g, at::Tensor avg,
                                 at::Tensor avg_sq, double inv_n) {
  TORCH_CHECK(g.scalar_type() == at::kFloat && avg.scalar_type() == at::kFloat
              && avg_sq.scalar_type() == at::kFloat,
              "welford_update is fp32");
  long long n = g.numel();
  auto out = at::zeros({}, g.options());
  hipLaunchKernelGGL(welford_update_kernel, dim3(grid_1d(n, 256)), dim3(256),
                     0, fedkit_stream(), g.contiguous().data_ptr<float>(),
                     avg.data_ptr<float>(), avg_sq.data_ptr<float>(),
                     (float)inv_n, out.data_ptr<float>(), n);
  return out;
}
