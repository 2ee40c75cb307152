// adamw.hip -- fused AdamW over a flat parameter range.
//
// The reference builds torch.optim.AdamW over two parameter groups (weight decay
// 0.05 / 0, tools/builder.py:41-101); PyTorch then runs it as ~35 multi-tensor
// launches per step over 203 tensors.  FlatDataParallel (data_parallel.py) keeps
// all parameters, gradients and both moments in contiguous fp32 buffers with the
// no-decay range first, so the whole update is two launches of this kernel, each
// a single streaming pass: 16 B read + 12 B written per parameter (0.81 GB per
// step for 29 M parameters, HBM-bound).
// Arithmetic follows torch.optim.AdamW (decoupled decay, bias correction,
// eps added to sqrt(v_hat)):
//   p *= 1 - lr*wd;  m = b1 m + (1-b1) g;  v = b2 v + (1-b2) g^2
//   p -= (lr / (1 - b1^t)) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)
// pdae_adamw_step_gscale reads g * (*gscale) in place of g (the multiply first, as torch.nn.utils.clip_grad_norm_
// scales .grad before the optimiser reads it): the clip coefficient of pdae_grad_norm_clip never leaves the device.
#include "common.h"

namespace pdae {

template <bool SCALED>
__global__ __launch_bounds__(256) void adamw_kernel(long long n4, float4* __restrict__ p,
                                                    const float4* __restrict__ g,
                                                    float4* __restrict__ m, float4* __restrict__ v,
                                                    float lr, float beta1, float beta2, float eps,
                                                    float weight_decay, float bc1, float bc2_sqrt,
                                                    const float* __restrict__ gscale) {
  const long long stride = (long long)gridDim.x * 256;
  const float decay = 1.f - lr * weight_decay;
  const float step = lr / bc1;
  const float gs = SCALED ? *gscale : 1.f;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
    float4 pp = p[i], mm = m[i], vv = v[i];
    float4 gg = g[i];
    if (SCALED) gg.x *= gs, gg.y *= gs, gg.z *= gs, gg.w *= gs;
#define PDAE_ADAMW(c)                                               \
    pp.c *= decay;                                                  \
    mm.c = beta1 * mm.c + (1.f - beta1) * gg.c;                     \
    vv.c = beta2 * vv.c + (1.f - beta2) * gg.c * gg.c;              \
    pp.c -= step * (mm.c / (sqrtf(vv.c) / bc2_sqrt + eps));
    PDAE_ADAMW(x) PDAE_ADAMW(y) PDAE_ADAMW(z) PDAE_ADAMW(w)
#undef PDAE_ADAMW
    p[i] = pp;
    m[i] = mm;
    v[i] = vv;
  }
}

template <bool SCALED>
__global__ void adamw_tail_kernel(int n, float* p, const float* g, float* m, float* v, float lr,
                                  float beta1, float beta2, float eps, float weight_decay, float bc1,
                                  float bc2_sqrt, const float* gscale) {
  const int i = threadIdx.x;
  if (i >= n) return;
  const float gi = SCALED ? g[i] * *gscale : g[i];
  float pp = p[i] * (1.f - lr * weight_decay);
  const float mm = beta1 * m[i] + (1.f - beta1) * gi;
  const float vv = beta2 * v[i] + (1.f - beta2) * gi * gi;
  pp -= (lr / bc1) * (mm / (sqrtf(vv) / bc2_sqrt + eps));
  p[i] = pp, m[i] = mm, v[i] = vv;
}

}  // namespace pdae

using namespace pdae;

template <bool SCALED>
static int adamw_launch(long long n, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float lr,
                        float beta1, float beta2, float eps, float weight_decay, int step, const float* gscale,
                        pdae_stream_t stream) {
  if (n < 0 || step < 1) return bad_arg("adamw_step: n >= 0 and step >= 1 required");
  if (n == 0) return PDAE_OK;
  if (!param || !grad || !exp_avg || !exp_avg_sq || (SCALED && !gscale)) return bad_arg("adamw_step: null pointer");
  if (reinterpret_cast<uintptr_t>(param) % 16 || reinterpret_cast<uintptr_t>(grad) % 16 ||
      reinterpret_cast<uintptr_t>(exp_avg) % 16 || reinterpret_cast<uintptr_t>(exp_avg_sq) % 16)
    return bad_arg("adamw_step: buffers must be 16-byte aligned");
  const float bc1 = 1.f - powf(beta1, (float)step);
  const float bc2_sqrt = sqrtf(1.f - powf(beta2, (float)step));
  hipStream_t s = as_stream(stream);
  const long long n4 = n / 4;
  if (n4 > 0) {
    long long blocks = (n4 + 255) / 256;
    if (blocks > 256 * 16) blocks = 256 * 16;
    hipLaunchKernelGGL(adamw_kernel<SCALED>, dim3((unsigned)blocks), dim3(256), 0, s, n4,
                       reinterpret_cast<float4*>(param), reinterpret_cast<const float4*>(grad),
                       reinterpret_cast<float4*>(exp_avg), reinterpret_cast<float4*>(exp_avg_sq), lr,
                       beta1, beta2, eps, weight_decay, bc1, bc2_sqrt, gscale);
  }
  const int tail = (int)(n - n4 * 4);
  if (tail)
    hipLaunchKernelGGL(adamw_tail_kernel<SCALED>, dim3(1), dim3(64), 0, s, tail, param + n4 * 4, grad + n4 * 4,
                       exp_avg + n4 * 4, exp_avg_sq + n4 * 4, lr, beta1, beta2, eps, weight_decay, bc1,
                       bc2_sqrt, gscale);
  return check_launch("adamw_step");
}

extern "C" int pdae_adamw_step(long long n, float* param, const float* grad, float* exp_avg,
                               float* exp_avg_sq, float lr, float beta1, float beta2, float eps,
                               float weight_decay, int step, pdae_stream_t stream) {
  return adamw_launch<false>(n, param, grad, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, weight_decay, step, nullptr,
                             stream);
}

extern "C" int pdae_adamw_step_gscale(long long n, float* param, const float* grad, float* exp_avg,
                                      float* exp_avg_sq, float lr, float beta1, float beta2, float eps,
                                      float weight_decay, int step, const float* gscale, pdae_stream_t stream) {
  return adamw_launch<true>(n, param, grad, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, weight_decay, step, gscale,
                            stream);
}
