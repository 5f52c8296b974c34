// Fused Adam step: ONE kernel updates every parameter tensor of the
// model (segment tables of csrc/multi_tensor.h).  torch's foreach
// Adam spends ~110 us/step on ResNet18 across ~10 multi-tensor sweeps
// (lerp/addcmul/sqrt/div chains re-reading m/v each time); the fused
// form is one pass at the traffic floor:
//   m = b1*m + (1-b1)*g
//   v = b2*v + (1-b2)*g^2
//   p -= lr * (m / bc1) / (sqrt(v / bc2) + eps)
// with bias corrections bc1 = 1-b1^t, bc2 = 1-b2^t computed on host.
// All fp32 (master weights / grads / state), 4 elems per lane.

#include "multi_tensor.h"

namespace {

using fedkit_mt::SegTable;

// pointer arrays of the table: param, grad, exp_avg, exp_avg_sq
enum { kP, kG, kM, kV };

__global__ void adam_step_kernel(SegTable<4> d, long long total, float lr,
                                 float b1, float b2, float eps,
                                 float inv_bc1, float inv_sqrt_bc2,
                                 float weight_decay) {
  // Roundings are spelled out (contraction off, explicit fmaf) so they do
  // not depend on which products the optimizer picks to fuse.  The two paths
  // round v and the denominator differently, as they always have: fused on
  // the vector path, separate multiply and add on the per-element path.
#pragma clang fp contract(off)
  typedef __attribute__((ext_vector_type(4))) float f4;
  fedkit_mt::for_each_unit<4>(
      d, total,
      [&](int t, long long j, long long) {
        f4 pv, gv, mv, vv;
        __builtin_memcpy(&pv, d.at<float>(kP, t) + j, 16);
        __builtin_memcpy(&gv, d.at<const float>(kG, t) + j, 16);
        __builtin_memcpy(&mv, d.at<float>(kM, t) + j, 16);
        __builtin_memcpy(&vv, d.at<float>(kV, t) + j, 16);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          float g = fmaf(weight_decay, pv[k], gv[k]);
          float m = fmaf(b1, mv[k], (1.f - b1) * g);
          float v = fmaf(b2, vv[k], (1.f - b2) * g * g);
          mv[k] = m;
          vv[k] = v;
          pv[k] -= lr * (m * inv_bc1) / fmaf(sqrtf(v), inv_sqrt_bc2, eps);
        }
        __builtin_memcpy(d.at<float>(kP, t) + j, &pv, 16);
        __builtin_memcpy(d.at<float>(kM, t) + j, &mv, 16);
        __builtin_memcpy(d.at<float>(kV, t) + j, &vv, 16);
      },
      [&](int t, long long j, long long) {
        float* pp = d.at<float>(kP, t) + j;
        float* mp = d.at<float>(kM, t) + j;
        float* vp = d.at<float>(kV, t) + j;
        float g = fmaf(weight_decay, *pp, d.at<const float>(kG, t)[j]);
        float m = fmaf(b1, *mp, (1.f - b1) * g);
        float v = b2 * *vp + (1.f - b2) * g * g;
        *mp = m;
        *vp = v;
        *pp -= lr * (m * inv_bc1) / (sqrtf(v) * inv_sqrt_bc2 + eps);
      });
}

}  // namespace

// params/grads/exp_avg/exp_avg_sq: parallel lists of any length; every
// tensor is validated before the first launch, then one launch per 48.
// step is the POST-increment step count (torch Adam semantics:
// state['step'] += 1 before use).
void fedkit_adam_step(std::vector<at::Tensor> params,
                      std::vector<at::Tensor> grads,
                      std::vector<at::Tensor> exp_avg,
                      std::vector<at::Tensor> exp_avg_sq, double lr,
                      double beta1, double beta2, double eps, long step,
                      double weight_decay) {
  auto cs = fedkit_mt::build_chunks<4>(
      "adam_step", {&params, &grads, &exp_avg, &exp_avg_sq},
      {at::kFloat, at::kFloat, at::kFloat, at::kFloat});
  const fedkit_mt::DeviceGuard guard(params[0].device());
  double bc1 = 1.0 - std::pow(beta1, (double)step);
  double bc2 = 1.0 - std::pow(beta2, (double)step);
  auto stream = fedkit_stream();
  for (const auto& c : cs.chunks)
    hipLaunchKernelGGL(adam_step_kernel,
                       dim3(grid_1d((c.total + 3) / 4, 256)), dim3(256), 0,
                       stream, c.d, c.total, (float)lr, (float)beta1,
                       (float)beta2, (float)eps, (float)(1.0 / bc1),
                       (float)(1.0 / std::sqrt(bc2)), (float)weight_decay);
}
