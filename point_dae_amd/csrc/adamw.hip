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

// one element's update on the component c of pp / mm / vv / gg (every kernel below)
#define PDAE_ADAMW(c)                                               \
    pp.c *= decay;                                                  \
    mm.c = beta1 * mm.c + (1.f - beta1) * gg.c;                     \
    vv.c = beta2 * vv.c + (1.f - beta2) * gg.c * gg.c;              \
    pp.c -= step * (mm.c / (sqrtf(vv.c) / bc2_sqrt + eps));

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
    PDAE_ADAMW(x) PDAE_ADAMW(y) PDAE_ADAMW(z) PDAE_ADAMW(w)
    p[i] = pp;
    m[i] = mm;
    v[i] = vv;
  }
}

// The segment table of pdae_adamw_step_segments, passed BY VALUE as a kernel argument (a learning-rate change is a
// new argument, not a device write, so the launch stays capturable).  Segment s covers [off, off + cnt) of the flat
// buffers, cut by the host into a scalar head [off, a), a float4 body [a, e) (a, e multiples of 4) and a scalar tail
// [e, off + cnt); head and tail hold at most 3 elements each.
struct AdamwSegments {
  int n;
  long long off[PDAE_ADAMW_MAX_SEGMENTS], a[PDAE_ADAMW_MAX_SEGMENTS], e[PDAE_ADAMW_MAX_SEGMENTS],
      end[PDAE_ADAMW_MAX_SEGMENTS];
  float lr[PDAE_ADAMW_MAX_SEGMENTS], wd[PDAE_ADAMW_MAX_SEGMENTS];
};

// adamw_kernel over up to 8 segments in one launch: the segments one after the other, each as the same float4
// grid-stride stream (no LDS); the first 8 threads of block 0 per segment update its head and tail elements.
// Elements outside every segment are neither read nor written.
template <bool SCALED>
__global__ __launch_bounds__(256) void adamw_segments_kernel(AdamwSegments t, float* __restrict__ p,
                                                             const float* __restrict__ g, float* __restrict__ m,
                                                             float* __restrict__ v, float beta1, float beta2,
                                                             float eps, float bc1, float bc2_sqrt,
                                                             const float* __restrict__ gscale) {
  const long long stride = (long long)gridDim.x * 256;
  const float gs = SCALED ? *gscale : 1.f;
  for (int s = 0; s < t.n; ++s) {
    const float lr = t.lr[s];
    const float decay = 1.f - lr * t.wd[s];
    const float step = lr / bc1;
    const long long n4 = (t.e[s] - t.a[s]) / 4;
    float4* p4 = reinterpret_cast<float4*>(p + t.a[s]);
    const float4* g4 = reinterpret_cast<const float4*>(g + t.a[s]);
    float4* m4 = reinterpret_cast<float4*>(m + t.a[s]);
    float4* v4 = reinterpret_cast<float4*>(v + t.a[s]);
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
      float4 pp = p4[i], mm = m4[i], vv = v4[i];
      float4 gg = g4[i];
      if (SCALED) gg.x *= gs, gg.y *= gs, gg.z *= gs, gg.w *= gs;
      PDAE_ADAMW(x) PDAE_ADAMW(y) PDAE_ADAMW(z) PDAE_ADAMW(w)
      p4[i] = pp;
      m4[i] = mm;
      v4[i] = vv;
    }
    if (blockIdx.x == 0 && threadIdx.x < 8) {
      const int j = threadIdx.x;                        // 0..3: head element j, 4..7: tail element j - 4
      const long long k = j < 4 ? t.off[s] + j : t.e[s] + (j - 4);
      if (j < 4 ? k < t.a[s] : k < t.end[s]) {
        float4 pp, mm, vv, gg;
        pp.x = p[k], mm.x = m[k], vv.x = v[k], gg.x = g[k];
        if (SCALED) gg.x *= gs;
        PDAE_ADAMW(x)
        p[k] = pp.x, m[k] = mm.x, v[k] = vv.x;
      }
    }
  }
}
#undef PDAE_ADAMW

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

template <bool SCALED>
static int adamw_segments_launch(const AdamwSegments& t, long long widest, float* param, const float* grad,
                                 float* exp_avg, float* exp_avg_sq, float beta1, float beta2, float eps, float bc1,
                                 float bc2_sqrt, const float* gscale, hipStream_t s) {
  long long blocks = (widest + 255) / 256;
  if (blocks < 1) blocks = 1;
  if (blocks > 256 * 16) blocks = 256 * 16;
  hipLaunchKernelGGL(adamw_segments_kernel<SCALED>, dim3((unsigned)blocks), dim3(256), 0, s, t, param, grad, exp_avg,
                     exp_avg_sq, beta1, beta2, eps, bc1, bc2_sqrt, gscale);
  return check_launch("adamw_step_segments");
}

extern "C" int pdae_adamw_step_segments(long long n, int num_segments, const pdae_adamw_segment* segments, float* param,
                                        const float* grad, float* exp_avg, float* exp_avg_sq, float beta1,
                                        float beta2, float eps, int step, const float* gscale,
                                        pdae_stream_t stream) {
  if (n < 0 || step < 1) return bad_arg("adamw_step_segments: n >= 0 and step >= 1 required");
  if (num_segments < 0 || num_segments > PDAE_ADAMW_MAX_SEGMENTS)
    return bad_arg("adamw_step_segments: 0 <= num_segments <= 8 required");
  if (num_segments > 0 && !segments) return bad_arg("adamw_step_segments: null segment table");
  AdamwSegments t;
  t.n = 0;
  long long widest = 0;
  for (int i = 0; i < num_segments; ++i) {
    const pdae_adamw_segment& sg = segments[i];
    if (sg.offset < 0 || sg.count < 0 || sg.offset > n || sg.count > n - sg.offset)
      return bad_arg("adamw_step_segments: a segment leaves [0, n)");
    for (int j = 0; j < i; ++j) {
      const pdae_adamw_segment& o = segments[j];
      if (sg.count > 0 && o.count > 0 && sg.offset < o.offset + o.count && o.offset < sg.offset + sg.count)
        return bad_arg("adamw_step_segments: segments overlap");
    }
    if (sg.count == 0) continue;
    const long long end = sg.offset + sg.count;
    long long a = (sg.offset + 3) / 4 * 4;
    if (a > end) a = end;
    long long e = end / 4 * 4;
    if (e < a) e = a;
    const int k = t.n++;
    t.off[k] = sg.offset, t.a[k] = a, t.e[k] = e, t.end[k] = end;
    t.lr[k] = sg.lr, t.wd[k] = sg.weight_decay;
    if ((e - a) / 4 > widest) widest = (e - a) / 4;
  }
  if (t.n == 0) return PDAE_OK;
  if (!param || !grad || !exp_avg || !exp_avg_sq) return bad_arg("adamw_step_segments: null pointer");
  if (reinterpret_cast<uintptr_t>(param) % 16 || reinterpret_cast<uintptr_t>(grad) % 16 ||
      reinterpret_cast<uintptr_t>(exp_avg) % 16 || reinterpret_cast<uintptr_t>(exp_avg_sq) % 16)
    return bad_arg("adamw_step_segments: buffers must be 16-byte aligned");
  const float bc1 = 1.f - powf(beta1, (float)step);
  const float bc2_sqrt = sqrtf(1.f - powf(beta2, (float)step));
  hipStream_t s = as_stream(stream);
  if (gscale)
    return adamw_segments_launch<true>(t, widest, param, grad, exp_avg, exp_avg_sq, beta1, beta2, eps, bc1, bc2_sqrt,
                                       gscale, s);
  return adamw_segments_launch<false>(t, widest, param, grad, exp_avg, exp_avg_sq, beta1, beta2, eps, bc1, bc2_sqrt,
                                      nullptr, s);
}
