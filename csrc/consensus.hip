// Fused consensus penalty and ADMM update kernels (FedProx / consensus ADMM).
//
// The closure-side penalty of the reference (consensus_multi.py:209-218,
// fedprox_multi.py:183-190, plus the L1/L2 regulariser of
// federated_multi.py:183-187) is, per minibatch closure call,
//   y.(x-z) + (rho/2)||x-z||^2 + lambda1 ||x||_1 + lambda2 ||x||^2
// over the trainable block x.  As stock torch ops that is a cat of the
// block, ~10 elementwise/reduction launches forward and the autograd replay
// backward.  Here the forward is ONE streaming reduction that reads the
// parameter tensors in place through by-value segment tables (<= 48
// tensors per launch, csrc/multi_tensor.h) and the
// backward is ONE elementwise pass writing the closed-form gradient
//   go * (y + rho (x-z) + lambda1 sign(x) + 2 lambda2 x)
// in the same physical (storage) element order the packed z / y use.
//
// The aggregation side gets the same treatment: admm_dual_update fuses
// y += rho (x-z) with the primal-residual norm, bb_stats forms the six
// Barzilai-Borwein inner products in one pass over five vectors.
//
// Every reduction is deterministic: fixed grid (a function of the length
// only), per-workgroup partials in a slab, one finalize kernel that sums
// the slab in a fixed order.  No floating-point atomics — the bit-exact
// kill-and-resume and nccl==local tests run through penalty_fwd.
//
// Memory access: 16-byte loads/stores are used per pointer only when that
// pointer is 16-byte aligned (parameter tensors come from separate
// allocations, so their offsets into the flat vectors are arbitrary);
// otherwise that side falls back to four dword accesses.  Units that
// straddle a tensor boundary or the tail take a per-element scalar path.

#include "multi_tensor.h"

namespace {

using fedkit_mt::DeviceGuard;
using fedkit_mt::for_each_unit;
using fedkit_mt::SegTable;

constexpr int kBlock = 256;
constexpr int kRedGrid = 512;   // workgroup cap of the reduction kernels

typedef __attribute__((ext_vector_type(4))) float f4;

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

// Sum of v over the 256-thread workgroup, valid in thread 0.  Wave64
// shuffle tree, then the four wave sums in index order: a fixed order.
__device__ __forceinline__ float block_sum(float v, float* red /* [4] */) {
#pragma unroll
  for (int off = 32; off; off >>= 1) v += __shfl_down(v, off, kWave);
  __syncthreads();   // red may still be read from a previous call
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

template <bool HZ, bool HY>
__device__ __forceinline__ float pen_term(float x, float z, float y,
                                          float hrho, float l1, float l2) {
  float s = l1 * fabsf(x) + l2 * x * x;
  if (HZ) {
    float dlt = x - z;
    s += hrho * dlt * dlt;
    if (HY) s += y * dlt;
  }
  return s;
}

template <bool HZ, bool HY>
__device__ __forceinline__ float pen_grad(float x, float z, float y,
                                          float rho, float l1, float l2x2,
                                          float go) {
  float sgn = (float)(x > 0.f) - (float)(x < 0.f);   // sign(0) = 0
  float g = l1 * sgn + l2x2 * x;
  if (HZ) {
    g += rho * (x - z);
    if (HY) g += y;
  }
  return go * g;
}

// part[blockIdx.x] = this workgroup's share of the penalty over the chunk.
// z / y already point at the chunk's slice of the flat vectors.
template <bool HZ, bool HY>
__global__ void __launch_bounds__(kBlock)
penalty_fwd_kernel(SegTable<1> d, const float* __restrict__ z,
                   const float* __restrict__ y, float hrho, float l1,
                   float l2, long long total, float* __restrict__ part) {
  __shared__ float red[4];
  float acc = 0.f;
  for_each_unit<4>(
      d, total,
      [&](int t, long long j, long long i0) {
        f4 xv = load4(d.at<const float>(0, t) + j);
        f4 zv = {}, yv = {};
        if (HZ) zv = load4(z + i0);
        if (HY) yv = load4(y + i0);
#pragma unroll
        for (int k = 0; k < 4; ++k)
          acc += pen_term<HZ, HY>(xv[k], zv[k], yv[k], hrho, l1, l2);
      },
      [&](int t, long long j, long long i) {
        acc += pen_term<HZ, HY>(d.at<const float>(0, t)[j], HZ ? z[i] : 0.f,
                                HY ? y[i] : 0.f, hrho, l1, l2);
      });
  float s = block_sum(acc, red);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// g[i] = go * dPenalty/dx_i over the chunk; g / z / y point at the chunk's
// slice of the flat vectors, go is a device scalar.
template <bool HZ, bool HY>
__global__ void __launch_bounds__(kBlock)
penalty_bwd_kernel(SegTable<1> d, const float* __restrict__ z,
                   const float* __restrict__ y, float rho, float l1,
                   float l2x2, const float* __restrict__ go_ptr,
                   long long total, float* __restrict__ g) {
  const float go = *go_ptr;
  for_each_unit<4>(
      d, total,
      [&](int t, long long j, long long i0) {
        f4 xv = load4(d.at<const float>(0, t) + j);
        f4 zv = {}, yv = {}, gv;
        if (HZ) zv = load4(z + i0);
        if (HY) yv = load4(y + i0);
#pragma unroll
        for (int k = 0; k < 4; ++k)
          gv[k] = pen_grad<HZ, HY>(xv[k], zv[k], yv[k], rho, l1, l2x2, go);
        store4(g + i0, gv);
      },
      [&](int t, long long j, long long i) {
        g[i] = pen_grad<HZ, HY>(d.at<const float>(0, t)[j], HZ ? z[i] : 0.f,
                                HY ? y[i] : 0.f, rho, l1, l2x2, go);
      });
}

// y += rho (x - z);  part[blockIdx.x] = partial sum of (rho (x - z))^2
__global__ void __launch_bounds__(kBlock)
admm_dual_update_kernel(float* __restrict__ y, const float* __restrict__ x,
                        const float* __restrict__ z, float rho, long long n,
                        float* __restrict__ part) {
  __shared__ float red[4];
  float acc = 0.f;
  const long long units = (n + 3) >> 2;
  for (long long u = blockIdx.x * (long long)kBlock + threadIdx.x; u < units;
       u += (long long)gridDim.x * kBlock) {
    long long i0 = u << 2;
    if (i0 + 4 <= n) {
      f4 xv = load4(x + i0), zv = load4(z + i0), yv = load4(y + i0);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float yd = rho * (xv[k] - zv[k]);
        yv[k] += yd;
        acc += yd * yd;
      }
      store4(y + i0, yv);
    } else {
      for (long long i = i0; i < n; ++i) {
        float yd = rho * (x[i] - z[i]);
        y[i] += yd;
        acc += yd * yd;
      }
    }
  }
  float s = block_sum(acc, red);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

__device__ __forceinline__ void bb_accum(float* acc, float y, float yh,
                                         float x, float z, float x0) {
  float a = y - yh, b = x - z, dx = x - x0;
  acc[0] += a * a;
  acc[1] += a * b;
  acc[2] += b * b;
  acc[3] += a * dx;
  acc[4] += b * dx;
  acc[5] += dx * dx;
}

// part[blockIdx.x][0..5] = partial (a.a, a.b, b.b, a.dx, b.dx, dx.dx)
__global__ void __launch_bounds__(kBlock)
bb_stats_kernel(const float* __restrict__ y, const float* __restrict__ yh,
                const float* __restrict__ x, const float* __restrict__ z,
                const float* __restrict__ x0, long long n,
                float* __restrict__ part) {
  __shared__ float red[4];
  float acc[6] = {};
  const long long units = (n + 3) >> 2;
  for (long long u = blockIdx.x * (long long)kBlock + threadIdx.x; u < units;
       u += (long long)gridDim.x * kBlock) {
    long long i0 = u << 2;
    if (i0 + 4 <= n) {
      f4 yv = load4(y + i0), hv = load4(yh + i0), xv = load4(x + i0),
         zv = load4(z + i0), pv = load4(x0 + i0);
#pragma unroll
      for (int k = 0; k < 4; ++k)
        bb_accum(acc, yv[k], hv[k], xv[k], zv[k], pv[k]);
    } else {
      for (long long i = i0; i < n; ++i)
        bb_accum(acc, y[i], yh[i], x[i], z[i], x0[i]);
    }
  }
#pragma unroll
  for (int c = 0; c < 6; ++c) {
    float s = block_sum(acc[c], red);
    if (threadIdx.x == 0) part[(long long)blockIdx.x * 6 + c] = s;
  }
}

const float* flat_ptr(const c10::optional<at::Tensor>& v, long long n,
                      const at::Tensor& like, const char* name) {
  if (!v.has_value()) return nullptr;
  fedkit_mt::check_flat("consensus penalty", name, *v, like, n);
  return v->data_ptr<float>();
}

void check_vec(const at::Tensor& v, const at::Tensor& like, const char* op) {
  fedkit_mt::check_flat(op, "every operand", v, like, like.numel());
}

}  // namespace

// 0-dim device fp32: [y.(x-z)] + (rho/2)||x-z||^2 + l1 ||x||_1 + l2 ||x||^2
at::Tensor fedkit_penalty_fwd(std::vector<at::Tensor> params,
                              c10::optional<at::Tensor> z,
                              c10::optional<at::Tensor> y, double rho,
                              double lambda1, double lambda2) {
  TORCH_CHECK(z.has_value() || !y.has_value(),
              "consensus penalty: y needs z");
  const auto cs = fedkit_mt::build_chunks<1>("consensus penalty", {&params},
                                             {at::kFloat});
  const auto& chunks = cs.chunks;
  const long long n = cs.total;
  const DeviceGuard guard(params[0].device());
  const float* zp = flat_ptr(z, n, params[0], "z");
  const float* yp = flat_ptr(y, n, params[0], "y");
  auto opts = params[0].options();
  if (chunks.empty()) return at::zeros({}, opts);
  auto out = at::empty({1}, opts);
  auto stream = fedkit_stream();
  auto part = at::empty({(long long)chunks.size() * kRedGrid}, opts);
  float* pp = part.data_ptr<float>();
  const float hrho = 0.5f * (float)rho, l1 = (float)lambda1,
              l2 = (float)lambda2;
  int np = 0;
  for (const auto& c : chunks) {
    int nb = grid_1d((c.total + 3) >> 2, kBlock, kRedGrid);
    if (yp) {
      hipLaunchKernelGGL((penalty_fwd_kernel<true, true>), dim3(nb),
                         dim3(kBlock), 0, stream, c.d, zp + c.base,
                         yp + c.base, hrho, l1, l2, c.total, pp + np);
    } else if (zp) {
      hipLaunchKernelGGL((penalty_fwd_kernel<true, false>), dim3(nb),
                         dim3(kBlock), 0, stream, c.d, zp + c.base,
                         (const float*)nullptr, hrho, l1, l2, c.total,
                         pp + np);
    } else {
      hipLaunchKernelGGL((penalty_fwd_kernel<false, false>), dim3(nb),
                         dim3(kBlock), 0, stream, c.d, (const float*)nullptr,
                         (const float*)nullptr, hrho, l1, l2, c.total,
                         pp + np);
    }
    np += nb;
  }
  fedkit_colsum_finalize(pp, np, 1, out.data_ptr<float>(), stream);
  return out.reshape({});
}

// flat fp32 [N] gradient in physical order, scaled by the device scalar go
at::Tensor fedkit_penalty_bwd(std::vector<at::Tensor> params,
                              c10::optional<at::Tensor> z,
                              c10::optional<at::Tensor> y, double rho,
                              double lambda1, double lambda2,
                              const at::Tensor& grad_out) {
  TORCH_CHECK(z.has_value() || !y.has_value(),
              "consensus penalty: y needs z");
  const auto cs = fedkit_mt::build_chunks<1>("consensus penalty", {&params},
                                             {at::kFloat});
  const auto& chunks = cs.chunks;
  const long long n = cs.total;
  fedkit_mt::check_flat("consensus penalty", "grad_out", grad_out, params[0],
                        1);
  const DeviceGuard guard(params[0].device());
  const float* zp = flat_ptr(z, n, params[0], "z");
  const float* yp = flat_ptr(y, n, params[0], "y");
  auto g = at::empty({n}, params[0].options());
  float* gp = g.data_ptr<float>();
  const float* go = grad_out.data_ptr<float>();
  auto stream = fedkit_stream();
  const float r = (float)rho, l1 = (float)lambda1,
              l2x2 = 2.f * (float)lambda2;
  for (const auto& c : chunks) {
    int nb = grid_1d((c.total + 3) >> 2, kBlock);
    if (yp) {
      hipLaunchKernelGGL((penalty_bwd_kernel<true, true>), dim3(nb),
                         dim3(kBlock), 0, stream, c.d, zp + c.base,
                         yp + c.base, r, l1, l2x2, go, c.total, gp + c.base);
    } else if (zp) {
      hipLaunchKernelGGL((penalty_bwd_kernel<true, false>), dim3(nb),
                         dim3(kBlock), 0, stream, c.d, zp + c.base,
                         (const float*)nullptr, r, l1, l2x2, go, c.total,
                         gp + c.base);
    } else {
      hipLaunchKernelGGL((penalty_bwd_kernel<false, false>), dim3(nb),
                         dim3(kBlock), 0, stream, c.d, (const float*)nullptr,
                         (const float*)nullptr, r, l1, l2x2, go, c.total,
                         gp + c.base);
    }
  }
  return g;
}

// y += rho (x - z) in place; returns the device scalar sum (rho (x-z))^2
at::Tensor fedkit_admm_dual_update(at::Tensor y, const at::Tensor& x,
                                   const at::Tensor& z, double rho) {
  check_vec(y, y, "admm_dual_update");
  check_vec(x, y, "admm_dual_update");
  check_vec(z, y, "admm_dual_update");
  const DeviceGuard guard(y.device());
  long long n = y.numel();
  if (n == 0) return at::zeros({}, y.options());
  auto out = at::empty({1}, y.options());
  auto stream = fedkit_stream();
  int nb = grid_1d((n + 3) >> 2, kBlock, kRedGrid);
  auto part = at::empty({nb}, y.options());
  hipLaunchKernelGGL(admm_dual_update_kernel, dim3(nb), dim3(kBlock), 0,
                     stream, y.data_ptr<float>(), x.data_ptr<float>(),
                     z.data_ptr<float>(), (float)rho, n,
                     part.data_ptr<float>());
  fedkit_colsum_finalize(part.data_ptr<float>(), nb, 1,
                         out.data_ptr<float>(), stream);
  return out.reshape({});
}

// device fp32 [6] = (a.a, a.b, b.b, a.dx, b.dx, dx.dx) with a = y - yhat0,
// b = x - z, dx = x - x0
at::Tensor fedkit_bb_stats(const at::Tensor& y, const at::Tensor& yhat0,
                           const at::Tensor& x, const at::Tensor& z,
                           const at::Tensor& x0) {
  check_vec(y, y, "bb_stats");
  check_vec(yhat0, y, "bb_stats");
  check_vec(x, y, "bb_stats");
  check_vec(z, y, "bb_stats");
  check_vec(x0, y, "bb_stats");
  const DeviceGuard guard(y.device());
  long long n = y.numel();
  if (n == 0) return at::zeros({6}, y.options());
  auto out = at::empty({6}, y.options());
  auto stream = fedkit_stream();
  int nb = grid_1d((n + 3) >> 2, kBlock, kRedGrid);
  auto part = at::empty({nb, 6}, y.options());
  hipLaunchKernelGGL(bb_stats_kernel, dim3(nb), dim3(kBlock), 0, stream,
                     y.data_ptr<float>(), yhat0.data_ptr<float>(),
                     x.data_ptr<float>(), z.data_ptr<float>(),
                     x0.data_ptr<float>(), n, part.data_ptr<float>());
  fedkit_colsum_finalize(part.data_ptr<float>(), nb, 6,
                         out.data_ptr<float>(), stream);
  return out;
}
