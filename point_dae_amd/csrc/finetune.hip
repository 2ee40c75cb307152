// finetune.hip -- the glue of the classification fine-tuning step (models/Point_MAE.py:578-706 PointTransformer,
// tools/runner_finetune.py:81-270) around the patch embedder and the Transformer blocks the pretraining step already has.
//   pdae_prepend_token / _grad    per cloud [token | G rows] (the cls token and cls_pos, :690-694); backward strips row 0
//                                 and sums it over the clouds in cloud order
//   pdae_cls_max_concat / _grad   [x[:, 0] | max_{t >= 1} x[:, t]] (:698), arg = the first maximal t
//   pdae_bn_relu_dropout / _grad  Linear -> BatchNorm1d -> ReLU -> Dropout(p) of cls_head_finetune (:616-626) after its
//                                 Linear: batch statistics, running estimates, the affine, ReLU and the dropout mask in
//                                 ONE launch (a thread owns a column and walks the B rows), backward likewise
//                                 _eval_grad: the backward on the running estimates (a frozen BatchNorm, training 0 / 2)
//   pdae_bn_lrelu_dropout / _grad the same for DGCNN's head (models/PointCAE_DGCNN.py:572-663): BatchNorm1d ->
//                                 LeakyReLU(slope) -> Dropout(p); at slope 0 it gives bn_relu_dropout's bits.  Both
//                                 entries launch bn_act_dropout_kernel / _grad_kernel, templated on the activation
//   pdae_softmax_xent / _grad     nn.CrossEntropyLoss() (mean) + the argmax hit count (get_loss_acc, :634-638)
//   pdae_softmax_xent_smooth / _grad  DGCNN's smoothloss (get_loss_acc, :592-600): cross-entropy against the target
//                                 t = onehot (1 - eps) + (1 - onehot) eps / (K - 1), + the same hit count.  Both entries
//                                 launch softmax_xent_kernel / _grad_kernel, templated on the target
//   pdae_grad_norm_clip           torch.nn.utils.clip_grad_norm_ (runner_finetune.py:201-202) on the flat gradient
//                                 buffer: per-block fp64 partials, then one block adds them in block order; the
//                                 clip coefficient stays on the device (AdamW reads it: pdae_adamw_step_gscale)
// Every reduction runs in a fixed order (no float atomics): results do not depend on scheduling.
#include <string>

#include "common.h"

namespace pdae {

// out (B, 1 + G, C): row 0 of cloud b = token, rows 1.. = x (B, G, C); one float4 per thread
__global__ __launch_bounds__(256) void prepend_token_kernel(long long n4, int C4, int T, const float4* __restrict__ x,
                                                            const float4* __restrict__ token, float4* __restrict__ out) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  const long long row = i / C4;
  const int q = (int)(i - row * C4), t = (int)(row % T);
  const long long b = row / T;
  out[i] = t == 0 ? token[q] : x[(b * (T - 1) + t - 1) * C4 + q];
}

// dx (B, G, C) = dout[:, 1:]; the first C4 threads also write dtoken[c] = sum_b dout[b, 0, c] (b ascending)
__global__ __launch_bounds__(256) void prepend_token_grad_kernel(long long n4, int B, int C4, int T,
                                                                 const float4* __restrict__ dout, float4* __restrict__ dx,
                                                                 float4* __restrict__ dtoken) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < C4) {
    float4 s = dout[i];
    for (int b = 1; b < B; ++b) {
      const float4 v = dout[(long long)b * T * C4 + i];
      s.x += v.x, s.y += v.y, s.z += v.z, s.w += v.w;
    }
    dtoken[i] = s;
  }
  if (i >= n4) return;
  const long long row = i / C4;                          // row of dx
  const int q = (int)(i - row * C4), t = (int)(row % (T - 1));
  const long long b = row / (T - 1);
  dx[i] = dout[(b * T + t + 1) * C4 + q];
}

// thread per (b, c): out[b][c] = x[b][0][c], out[b][C + c] = max_{t >= 1} x[b][t][c], arg = first t attaining it
// (finite inputs: a NaN row is passed over where torch.max would return NaN)
__global__ __launch_bounds__(256) void cls_max_concat_kernel(int B, int T, int C, const float* __restrict__ x,
                                                             float* __restrict__ out, unsigned char* __restrict__ arg) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= B * C) return;
  const int b = i / C, c = i - b * C;
  const float* xb = x + (size_t)b * T * C + c;
  float m = xb[C];
  int a = 1;
  for (int t = 2; t < T; ++t) {
    const float v = xb[(size_t)t * C];
    if (v > m) m = v, a = t;
  }
  out[(size_t)b * 2 * C + c] = xb[0];
  out[(size_t)b * 2 * C + C + c] = m;
  arg[i] = (unsigned char)a;
}

// dx (B, T, C) dense: row 0 gets the cls half of dout, the arg-max row the max half, every other row 0
__global__ __launch_bounds__(256) void cls_max_concat_grad_kernel(long long n, int T, int C, const float* __restrict__ dout,
                                                                  const unsigned char* __restrict__ arg, float* __restrict__ dx) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const long long row = i / C;
  const int c = (int)(i - row * C), t = (int)(row % T);
  const long long b = row / T;
  float v = 0.f;
  if (t == 0) v = dout[b * 2 * C + c];
  else if (arg[b * C + c] == t) v = dout[b * 2 * C + C + c];
  dx[i] = v;
}

// thread per column n of y (B, N).  Training: fp64 mean and biased variance over the B rows (two passes), the running
// estimates with the unbiased variance (nn.BatchNorm1d), mean / invstd saved for the backward; eval: the running
// estimates, also written to mean / invstd when those are given (the eval-mode backward reads them); the host passes u
// in eval mode only for a frozen BatchNorm under a live Dropout (the entry's training = 2).
// out = act((y - mean) gamma invstd + beta) * (u >= p ? 1 / (1 - p) : 0); u null: no dropout.
// act = relu, or (LEAKY) LeakyReLU: max(v, 0) + slope min(v, 0) -- one of the two terms is 0, so it is torch's
// `v > 0 ? v : v * slope` with a +0 (never -0) for v <= 0 at slope 0, as fmaxf(v, 0) gives.  The two activations keep
// separate expressions: LEAKY at slope 0 gives the ReLU instantiation's bits through that signed-zero argument
template <bool LEAKY>
__global__ __launch_bounds__(256) void bn_act_dropout_kernel(int B, int N, const float* __restrict__ y,
                                                             const float* __restrict__ gamma, const float* __restrict__ beta,
                                                             float eps, float momentum, float* __restrict__ rmean,
                                                             float* __restrict__ rvar, long long* __restrict__ counter,
                                                             int training, float p, float slope,
                                                             const float* __restrict__ u, float* __restrict__ out,
                                                             float* __restrict__ mean, float* __restrict__ invstd) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (training && n == 0 && counter) *counter += 1;
  if (n >= N) return;
  float m, is;
  if (training) {
    double s1 = 0.0;
    for (int r = 0; r < B; ++r) s1 += (double)y[(size_t)r * N + n];
    const double mu = s1 / B;
    double s2 = 0.0;
    for (int r = 0; r < B; ++r) {
      const double d = (double)y[(size_t)r * N + n] - mu;
      s2 += d * d;
    }
    const double var = s2 / B;
    m = (float)mu;
    is = 1.0f / sqrtf((float)var + eps);
    if (rmean) rmean[n] = (1.0f - momentum) * rmean[n] + momentum * m;
    if (rvar) rvar[n] = (1.0f - momentum) * rvar[n] + momentum * (float)(s2 / (B - 1));
    mean[n] = m;
    invstd[n] = is;
  } else {
    m = rmean[n];
    is = 1.0f / sqrtf(rvar[n] + eps);
    if (mean) mean[n] = m;                            // (for the eval-mode backward)
    if (invstd) invstd[n] = is;
  }
  const float sc = gamma[n] * is, be = beta[n];
  const float keep_scale = 1.0f / (1.0f - p);
  for (int r = 0; r < B; ++r) {
    const size_t k = (size_t)r * N + n;
    const float z = (y[k] - m) * sc + be;             // centred first: no cancellation when the variance is small
    float v;
    if constexpr (LEAKY) v = fmaxf(z, 0.f) + slope * fminf(z, 0.f);
    else v = fmaxf(z, 0.f);
    if (u) v = u[k] >= p ? v * keep_scale : 0.f;
    out[k] = v;
  }
}

// dout times the activation's derivative at z = the forward's pre-activation (same arithmetic): 1 for z > 0, else 0
// (ReLU) or slope (LEAKY; `+ 0.f` turns slope * dout = -0 into +0, so that slope 0 gives ReLU's bits)
template <bool LEAKY>
__device__ __forceinline__ float act_grad(float z, const float* __restrict__ dout, float slope) {
  if constexpr (LEAKY) return z > 0.f ? *dout : slope * *dout + 0.f;
  else return z > 0.f ? *dout : 0.f;
}

// backward of the forward, thread per column: g = dout * dropout mask * act'(.); dbeta = sum g,
// dgamma = sum g xhat (fp64, rows in order); BATCH (training-mode BatchNorm): dy = gamma invstd (g - dbeta / B -
// xhat dgamma / B); else (the running estimates: mean and invstd are constants) dy = gamma invstd g
template <bool LEAKY, bool BATCH>
__global__ __launch_bounds__(256) void bn_act_dropout_grad_kernel(int B, int N, const float* __restrict__ y,
                                                                  const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                  const float* __restrict__ mean, const float* __restrict__ invstd,
                                                                  float slope, float p, const float* __restrict__ u,
                                                                  const float* __restrict__ dout, float* __restrict__ dy,
                                                                  float* __restrict__ dgamma, float* __restrict__ dbeta) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  const float m = mean[n], is = invstd[n], ga = gamma[n];
  const float sc = ga * is, be = beta[n];
  const float keep_scale = 1.0f / (1.0f - p);
  double sg = 0.0, sgx = 0.0;
  for (int r = 0; r < B; ++r) {
    const size_t k = (size_t)r * N + n;
    const float x = y[k];
    float g = act_grad<LEAKY>((x - m) * sc + be, dout + k, slope);
    if (u) g = u[k] >= p ? g * keep_scale : 0.f;
    sg += (double)g;
    sgx += (double)g * (double)((x - m) * is);
  }
  dbeta[n] = (float)sg;
  dgamma[n] = (float)sgx;
  const float c1 = (float)(sg / B), c2 = (float)(sgx / B);
  for (int r = 0; r < B; ++r) {
    const size_t k = (size_t)r * N + n;
    const float x = y[k];
    float g = act_grad<LEAKY>((x - m) * sc + be, dout + k, slope);
    if (u) g = u[k] >= p ? g * keep_scale : 0.f;
    if constexpr (BATCH) dy[k] = sc * (g - c1 - (x - m) * is * c2);
    else dy[k] = sc * g;
  }
}

__device__ __forceinline__ float wave_max(float v) {
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ float wave_sum(float v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// one wave per row (lane = class, K <= 64): lse = max + log sum exp(x - max); loss_r = lse - (the target term);
// hit_r = argmax == label (ties: the lowest class).  Row results in shared memory, added in row order by thread 0.
// The target term is x[label] (nn.CrossEntropyLoss), or (SMOOTH) sum_k t_k x_k against the smoothed target
// t_k = k == label ? on : off (the lane products added by the wave's butterfly); at eps = 0 that sum is x[label]
// plus zeros: the plain instantiation's bits
constexpr int XENT_MAX_B = 4096;
template <bool SMOOTH>
__global__ __launch_bounds__(256) void softmax_xent_kernel(int B, int K, float on, float off,
                                                           const float* __restrict__ logits,
                                                           const int64_t* __restrict__ labels, float* __restrict__ loss,
                                                           float* __restrict__ correct) {
  __shared__ float rl[XENT_MAX_B];
  __shared__ unsigned char rh[XENT_MAX_B];
  const int lane = lane_id(), w = threadIdx.x / kWave;
  for (int r = w; r < B; r += 4) {
    const float x = lane < K ? logits[(size_t)r * K + lane] : -INFINITY;
    const float mx = wave_max(x);
    const float s = wave_sum(lane < K ? expf(x - mx) : 0.f);
    const int64_t lab = labels[r];
    const bool ok = lab >= 0 && lab < K;
    float tx;
    if constexpr (SMOOTH) tx = wave_sum(lane < K ? (lane == lab ? on : off) * x : 0.f);
    else tx = __shfl(x, ok ? (int)lab : 0);
    // the first lane holding the maximum
    const unsigned long long at = __ballot(lane < K && x == mx);
    const int am = __ffsll((long long)at) - 1;
    if (lane == 0) {
      rl[r] = ok ? (mx + logf(s)) - tx : NAN;
      rh[r] = ok && am == lab;
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = 0.f, h = 0.f;
    for (int r = 0; r < B; ++r) t += rl[r], h += rh[r];
    *loss = t / B;
    *correct = h;
  }
}

// dlogits[r][k] = (softmax(x_r)[k] - t_k) * dloss / B, one wave per row; t = the one-hot label, or (SMOOTH) on / off
template <bool SMOOTH>
__global__ __launch_bounds__(256) void softmax_xent_grad_kernel(int B, int K, float on, float off,
                                                                const float* __restrict__ logits,
                                                                const int64_t* __restrict__ labels,
                                                                const float* __restrict__ dloss, float* __restrict__ dlogits) {
  const int lane = lane_id();
  const int r = blockIdx.x * 4 + threadIdx.x / kWave;
  if (r >= B) return;
  const float x = lane < K ? logits[(size_t)r * K + lane] : -INFINITY;
  const float mx = wave_max(x);
  const float e = lane < K ? expf(x - mx) : 0.f;
  const float s = wave_sum(e);
  const float scale = *dloss / (float)B;
  if (lane < K)
    dlogits[(size_t)r * K + lane] = (e / s - (labels[r] == lane ? (SMOOTH ? on : 1.f) : (SMOOTH ? off : 0.f))) * scale;
}

// per-block partial sums of squares of g (float4 grid-stride; each thread adds its squares in fp32 groups of 4, the
// block adds the threads in a fixed tree, fp64); block 0 also takes the n % 4 tail
constexpr int GN_BLOCKS = 2048;
__global__ __launch_bounds__(256) void grad_sqnorm_partials_kernel(long long n, const float4* __restrict__ g,
                                                                   double* __restrict__ part) {
  __shared__ double red[256];
  const long long n4 = n / 4;
  double acc = 0.0;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
    const float4 v = g[i];
    acc += (double)(v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w);
  }
  if (blockIdx.x == 0 && threadIdx.x < n - n4 * 4) {
    const float v = reinterpret_cast<const float*>(g)[n4 * 4 + threadIdx.x];
    acc += (double)(v * v);
  }
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) part[blockIdx.x] = red[0];
}

// one block: the P partials in a fixed order -> norm, coef = min(1, max_norm / (norm + 1e-6)) (clip_grad_norm_, fp32 tail)
__global__ __launch_bounds__(256) void grad_norm_finish_kernel(int P, const double* __restrict__ part, float max_norm,
                                                               float* __restrict__ norm, float* __restrict__ coef) {
  __shared__ double red[256];
  double acc = 0.0;
  for (int i = threadIdx.x; i < P; i += 256) acc += part[i];
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const float nf = (float)sqrt(red[0]);
    if (norm) *norm = nf;
    const float c = max_norm / (nf + 1e-6f);
    *coef = c < 1.0f ? c : 1.0f;
  }
}

static unsigned blocks_for(long long n) { return (unsigned)((n + 255) / 256); }

}  // namespace pdae

using namespace pdae;

extern "C" int pdae_prepend_token(int B, int G, int C, const float* x, const float* token, float* out, pdae_stream_t stream) {
  if (B < 1 || G < 0 || C < 4 || C % 4) return bad_arg("prepend_token: B >= 1, G >= 0 and C % 4 == 0 required");
  if (!x || !token || !out) return bad_arg("prepend_token: null pointer");
  if (reinterpret_cast<uintptr_t>(x) % 16 || reinterpret_cast<uintptr_t>(token) % 16 || reinterpret_cast<uintptr_t>(out) % 16)
    return bad_arg("prepend_token: buffers must be 16-byte aligned");
  const long long n4 = (long long)B * (G + 1) * (C / 4);
  hipLaunchKernelGGL(prepend_token_kernel, dim3(blocks_for(n4)), dim3(256), 0, as_stream(stream), n4, C / 4, G + 1,
                     reinterpret_cast<const float4*>(x), reinterpret_cast<const float4*>(token), reinterpret_cast<float4*>(out));
  return check_launch("prepend_token");
}

extern "C" int pdae_prepend_token_grad(int B, int G, int C, const float* dout, float* dx, float* dtoken, pdae_stream_t stream) {
  if (B < 1 || G < 0 || C < 4 || C % 4) return bad_arg("prepend_token_grad: B >= 1, G >= 0 and C % 4 == 0 required");
  if (!dout || !dtoken || (G && !dx)) return bad_arg("prepend_token_grad: null pointer");
  if (reinterpret_cast<uintptr_t>(dout) % 16 || reinterpret_cast<uintptr_t>(dx) % 16 || reinterpret_cast<uintptr_t>(dtoken) % 16)
    return bad_arg("prepend_token_grad: buffers must be 16-byte aligned");
  const long long n4 = (long long)B * G * (C / 4);
  const long long threads = n4 > C / 4 ? n4 : C / 4;
  hipLaunchKernelGGL(prepend_token_grad_kernel, dim3(blocks_for(threads)), dim3(256), 0, as_stream(stream), n4, B, C / 4,
                     G + 1, reinterpret_cast<const float4*>(dout), reinterpret_cast<float4*>(dx),
                     reinterpret_cast<float4*>(dtoken));
  return check_launch("prepend_token_grad");
}

extern "C" int pdae_cls_max_concat(int B, int T, int C, const float* x, float* out, unsigned char* arg, pdae_stream_t stream) {
  if (B < 1 || C < 1) return bad_arg("cls_max_concat: B >= 1 and C >= 1 required");
  if (T < 2 || T > 256) return unsupported("cls_max_concat: 2 <= T <= 256 (uint8 arg)");
  if (!x || !out || !arg) return bad_arg("cls_max_concat: null pointer");
  hipLaunchKernelGGL(cls_max_concat_kernel, dim3(blocks_for((long long)B * C)), dim3(256), 0, as_stream(stream), B, T, C, x,
                     out, arg);
  return check_launch("cls_max_concat");
}

extern "C" int pdae_cls_max_concat_grad(int B, int T, int C, const float* dout, const unsigned char* arg, float* dx,
                                        pdae_stream_t stream) {
  if (B < 1 || C < 1) return bad_arg("cls_max_concat_grad: B >= 1 and C >= 1 required");
  if (T < 2 || T > 256) return unsupported("cls_max_concat_grad: 2 <= T <= 256 (uint8 arg)");
  if (!dout || !arg || !dx) return bad_arg("cls_max_concat_grad: null pointer");
  const long long n = (long long)B * T * C;
  hipLaunchKernelGGL(cls_max_concat_grad_kernel, dim3(blocks_for(n)), dim3(256), 0, as_stream(stream), n, T, C, dout, arg, dx);
  return check_launch("cls_max_concat_grad");
}

// "<what>: <msg>" through bad_arg or unsupported: the entry's error text and status
static int fail(int (*status)(const char*), const char* what, const char* msg) {
  return status((std::string(what) + ": " + msg).c_str());
}

// the checks and the launch behind pdae_bn_relu_dropout and (LEAKY) pdae_bn_lrelu_dropout
template <bool LEAKY>
static int bn_act_dropout(const char* what, int B, int N, const float* y, const float* gamma, const float* beta, float eps,
                          float momentum, float* running_mean, float* running_var, long long* num_batches_tracked,
                          int training, float slope, float p, const float* u, float* out, float* mean, float* invstd,
                          pdae_stream_t stream) {
  if (B < 1 || N < 1) return fail(bad_arg, what, "B >= 1 and N >= 1 required");
  if (!y || !gamma || !beta || !out) return fail(bad_arg, what, "null pointer");
  if (LEAKY && !(slope >= 0.f && slope < 1.f)) return fail(bad_arg, what, "0 <= negative_slope < 1 required");
  if (training != 0 && training != 1 && training != 2) return fail(bad_arg, what, "training must be 0, 1 or 2");
  if (training == 1) {
    if (B < 2) return fail(bad_arg, what, "training-mode batch statistics need B >= 2");
    if (!mean || !invstd) return fail(bad_arg, what, "training mode writes mean and invstd");
    if (!(p >= 0.f && p < 1.f)) return fail(bad_arg, what, "0 <= p < 1 required");
  } else {                                            // 0: eval; 2: a frozen BatchNorm under a live Dropout
    if (!running_mean || !running_var) return fail(bad_arg, what, "eval mode reads the running estimates");
    if (training == 0) u = nullptr;
    else if (!(p >= 0.f && p < 1.f)) return fail(bad_arg, what, "0 <= p < 1 required");
  }
  hipLaunchKernelGGL(bn_act_dropout_kernel<LEAKY>, dim3(blocks_for(N)), dim3(256), 0, as_stream(stream), B, N, y, gamma,
                     beta, eps, momentum, running_mean, running_var, num_batches_tracked, training == 1, p, slope, u, out,
                     mean, invstd);
  return check_launch(what);
}

template <bool LEAKY, bool BATCH = true>
static int bn_act_dropout_grad(const char* what, int B, int N, const float* y, const float* gamma, const float* beta,
                               const float* mean, const float* invstd, float slope, float p, const float* u,
                               const float* dout, float* dy, float* dgamma, float* dbeta, pdae_stream_t stream) {
  if (BATCH && (B < 2 || N < 1)) return fail(bad_arg, what, "B >= 2 and N >= 1 required");
  if (!BATCH && (B < 1 || N < 1)) return fail(bad_arg, what, "B >= 1 and N >= 1 required");
  if (LEAKY && !(slope >= 0.f && slope < 1.f)) return fail(bad_arg, what, "0 <= negative_slope < 1 required");
  if (!(p >= 0.f && p < 1.f)) return fail(bad_arg, what, "0 <= p < 1 required");
  if (!y || !gamma || !beta || !mean || !invstd || !dout || !dy || !dgamma || !dbeta) return fail(bad_arg, what, "null pointer");
  hipLaunchKernelGGL((bn_act_dropout_grad_kernel<LEAKY, BATCH>), dim3(blocks_for(N)), dim3(256), 0, as_stream(stream), B, N, y,
                     gamma, beta, mean, invstd, slope, p, u, dout, dy, dgamma, dbeta);
  return check_launch(what);
}

extern "C" int pdae_bn_relu_dropout(int B, int N, const float* y, const float* gamma, const float* beta, float eps,
                                    float momentum, float* running_mean, float* running_var, long long* num_batches_tracked,
                                    int training, float p, const float* u, float* out, float* mean, float* invstd,
                                    pdae_stream_t stream) {
  return bn_act_dropout<false>("bn_relu_dropout", B, N, y, gamma, beta, eps, momentum, running_mean, running_var,
                               num_batches_tracked, training, 0.f, p, u, out, mean, invstd, stream);
}

extern "C" int pdae_bn_relu_dropout_grad(int B, int N, const float* y, const float* gamma, const float* beta,
                                         const float* mean, const float* invstd, float p, const float* u,
                                         const float* dout, float* dy, float* dgamma, float* dbeta, pdae_stream_t stream) {
  return bn_act_dropout_grad<false>("bn_relu_dropout_grad", B, N, y, gamma, beta, mean, invstd, 0.f, p, u, dout, dy,
                                    dgamma, dbeta, stream);
}

extern "C" int pdae_bn_relu_dropout_eval_grad(int B, int N, const float* y, const float* gamma, const float* beta,
                                              const float* mean, const float* invstd, float p, const float* u,
                                              const float* dout, float* dy, float* dgamma, float* dbeta,
                                              pdae_stream_t stream) {
  return bn_act_dropout_grad<false, false>("bn_relu_dropout_eval_grad", B, N, y, gamma, beta, mean, invstd, 0.f, p, u,
                                           dout, dy, dgamma, dbeta, stream);
}

extern "C" int pdae_bn_lrelu_dropout(int B, int N, const float* y, const float* gamma, const float* beta, float eps,
                                     float momentum, float* running_mean, float* running_var, long long* num_batches_tracked,
                                     int training, float negative_slope, float p, const float* u, float* out, float* mean,
                                     float* invstd, pdae_stream_t stream) {
  return bn_act_dropout<true>("bn_lrelu_dropout", B, N, y, gamma, beta, eps, momentum, running_mean, running_var,
                              num_batches_tracked, training, negative_slope, p, u, out, mean, invstd, stream);
}

extern "C" int pdae_bn_lrelu_dropout_grad(int B, int N, const float* y, const float* gamma, const float* beta,
                                          const float* mean, const float* invstd, float negative_slope, float p,
                                          const float* u, const float* dout, float* dy, float* dgamma, float* dbeta,
                                          pdae_stream_t stream) {
  return bn_act_dropout_grad<true>("bn_lrelu_dropout_grad", B, N, y, gamma, beta, mean, invstd, negative_slope, p, u,
                                   dout, dy, dgamma, dbeta, stream);
}

extern "C" int pdae_bn_lrelu_dropout_eval_grad(int B, int N, const float* y, const float* gamma, const float* beta,
                                               const float* mean, const float* invstd, float negative_slope, float p,
                                               const float* u, const float* dout, float* dy, float* dgamma,
                                               float* dbeta, pdae_stream_t stream) {
  return bn_act_dropout_grad<true, false>("bn_lrelu_dropout_eval_grad", B, N, y, gamma, beta, mean, invstd,
                                          negative_slope, p, u, dout, dy, dgamma, dbeta, stream);
}

// the checks of the cross-entropy entries (have_ptrs: no null pointer among them); SMOOTH: one text for the shape and
// eps checks, and the target's two values as the reference forms them in fp32: one_hot * (1 - eps) + (1 - one_hot) *
// eps / (K - 1).  The plain loss takes K = 1, the smoothed one needs K >= 2
template <bool SMOOTH>
static int xent_args(const char* what, int B, int K, float eps, bool have_ptrs, float* on, float* off) {
  if (SMOOTH) {
    const char* req = "B in [1, 4096], K in [2, 64] and eps in [0, 1] required";
    if (B < 1 || K < 2) return fail(bad_arg, what, req);
    if (K > kWave || B > XENT_MAX_B) return fail(unsupported, what, req);
    if (!(eps >= 0.f && eps <= 1.f)) return fail(bad_arg, what, req);
    *on = 1.0f - eps;
    *off = eps / (float)(K - 1);
  } else {
    if (B < 1 || K < 1) return fail(bad_arg, what, "B >= 1 and K >= 1 required");
    if (K > kWave || B > XENT_MAX_B) return fail(unsupported, what, "K <= 64 classes and B <= 4096 rows");
  }
  if (!have_ptrs) return fail(bad_arg, what, "null pointer");
  return PDAE_OK;
}

template <bool SMOOTH>
static int softmax_xent(const char* what, int B, int K, float eps, const float* logits, const int64_t* labels, float* loss,
                        float* correct, pdae_stream_t stream) {
  float on = 0.f, off = 0.f;
  if (const int st = xent_args<SMOOTH>(what, B, K, eps, logits && labels && loss && correct, &on, &off)) return st;
  hipLaunchKernelGGL(softmax_xent_kernel<SMOOTH>, dim3(1), dim3(256), 0, as_stream(stream), B, K, on, off, logits, labels,
                     loss, correct);
  return check_launch(what);
}

template <bool SMOOTH>
static int softmax_xent_grad(const char* what, int B, int K, float eps, const float* logits, const int64_t* labels,
                             const float* dloss, float* dlogits, pdae_stream_t stream) {
  float on = 0.f, off = 0.f;
  if (const int st = xent_args<SMOOTH>(what, B, K, eps, logits && labels && dloss && dlogits, &on, &off)) return st;
  hipLaunchKernelGGL(softmax_xent_grad_kernel<SMOOTH>, dim3((B + 3) / 4), dim3(256), 0, as_stream(stream), B, K, on, off,
                     logits, labels, dloss, dlogits);
  return check_launch(what);
}

extern "C" int pdae_softmax_xent(int B, int K, const float* logits, const int64_t* labels, float* loss, float* correct,
                                 pdae_stream_t stream) {
  return softmax_xent<false>("softmax_xent", B, K, 0.f, logits, labels, loss, correct, stream);
}

extern "C" int pdae_softmax_xent_grad(int B, int K, const float* logits, const int64_t* labels, const float* dloss,
                                      float* dlogits, pdae_stream_t stream) {
  return softmax_xent_grad<false>("softmax_xent_grad", B, K, 0.f, logits, labels, dloss, dlogits, stream);
}

extern "C" int pdae_softmax_xent_smooth(int B, int K, float eps, const float* logits, const int64_t* labels, float* loss,
                                        float* correct, pdae_stream_t stream) {
  return softmax_xent<true>("softmax_xent_smooth", B, K, eps, logits, labels, loss, correct, stream);
}

extern "C" int pdae_softmax_xent_smooth_grad(int B, int K, float eps, const float* logits, const int64_t* labels,
                                             const float* dloss, float* dlogits, pdae_stream_t stream) {
  return softmax_xent_grad<true>("softmax_xent_smooth_grad", B, K, eps, logits, labels, dloss, dlogits, stream);
}

extern "C" int pdae_grad_norm_parts(long long n) {
  if (n <= 0) return 1;
  const long long want = (n / 4 + 255) / 256;
  return (int)(want < 1 ? 1 : want > GN_BLOCKS ? GN_BLOCKS : want);
}

extern "C" int pdae_grad_norm_clip(long long n, const float* grad, float max_norm, double* partials, float* norm, float* coef,
                                   pdae_stream_t stream) {
  if (n < 1) return bad_arg("grad_norm_clip: n >= 1 required");
  if (!grad || !partials || !coef) return bad_arg("grad_norm_clip: null pointer");
  if (reinterpret_cast<uintptr_t>(grad) % 16) return bad_arg("grad_norm_clip: the gradient must be 16-byte aligned");
  const int P = pdae_grad_norm_parts(n);
  hipStream_t s = as_stream(stream);
  hipLaunchKernelGGL(grad_sqnorm_partials_kernel, dim3(P), dim3(256), 0, s, n, reinterpret_cast<const float4*>(grad), partials);
  hipLaunchKernelGGL(grad_norm_finish_kernel, dim3(1), dim3(256), 0, s, P, partials, max_norm, norm, coef);
  return check_launch("grad_norm_clip");
}
