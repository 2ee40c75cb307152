// affinity.hip -- the task-affinity protocol's linear probe (tools/runner_finetune.py:1198-1269 of the reference:
// nn.Linear(feat_dim, num_class) trained for 300 epochs of batches of 64 with AdamW(lr 1e-3, weight decay 0.05) under
// CosineAnnealingLR, then the mean cross-entropy and the accuracy on the test features) on gfx950.
//
// Training.  The probe is epochs * floor(n / 64) strictly sequential steps of ~14 MFLOP each (D = 1024, K = 55): as
// framework ops a step is well over a dozen launches, here it is ONE.  The D columns are cut into S = ceil(D / 64)
// slices; workgroup s owns columns [64 s, 64 s + 64) of W and of both moments, nobody else reads or writes them.  The
// launch of step t, in every workgroup:
//   1. logits (64, K) of batch t = the S partial-logit tiles of batch t added in slice order, + b      (all of it, redundantly)
//   2. g = (softmax(logits) - onehot) / 64 in LDS                                                       (redundantly)
//   3. its slice of dW = g^T x (rows in batch order) and AdamW on that slice; workgroup 0 also db = column sums of g
//      (16 rows per wave in row order, the four waves in order) and AdamW on b
//   4. its partial logits of batch t + 1 from the slice it has just updated.
// The dot products of 3 and 4 are fused multiply-adds (one rounding per term), written out: the library is built with
// -ffp-contract=off.
// The kernel boundary is the only grid-wide synchronisation: no workgroup ever waits for another inside a kernel, the
// dependency between steps is the launch order on one stream.  The partial tiles and b are double-buffered by the
// parity of t, because one workgroup writes batch t + 1's values while another still reads batch t's.  A prologue launch
// writes the partials of the first batch.  The rows of a batch are gathered through the epoch's permutation; X is
// never copied.  Every sum has a fixed order (slices ascending, rows ascending, columns ascending, xor butterflies) and
// there are no atomics: two identical calls give identical bits.
//
// The update is torch.optim.AdamW's in the order of adamw.hip: p *= 1 - lr wd; m = b1 m + (1 - b1) g;
// v = b2 v + (1 - b2) g^2; p -= (lr / (1 - b1^t)) m / (sqrt(v) / sqrt(1 - b2^t) + eps), W and b alike (the reference
// passes net.parameters(): no no-decay group).  The scalars of a step are formed on the host in fp64 and rounded once:
// 1 - lr wd, lr / (1 - b1^t) and sqrt(1 - b2^t) from the epoch's fp64 learning rate and the global step t (an fp32 pow
// would be off at t ~ 2e5), and 1 - b1, 1 - b2 as torch rounds them (1.f - 0.999f is 4.7e-5 away from 1e-3: v, and with
// it every step, would be off by 2e-5 against bias corrections taken from the exact b2).  They travel as kernel arguments.
//
// Evaluation.  One wave per test row: the K logits by lane-strided dot products (butterfly sums), the row's fp32
// cross-entropy and its argmax (ties to the lowest class); a one-workgroup pass then adds the row losses in fp64 and
// counts the correct rows, both in a fixed order.
#include <math.h>

#include "common.h"

namespace pdae {
namespace {

constexpr int PB = PDAE_PROBE_BATCH;            // rows of a batch
constexpr int PW = 64;                          // columns of a slice
constexpr int PT = 256;                         // threads of a workgroup
constexpr int PWAVES = PT / kWave;
constexpr int PK = PDAE_PROBE_MAX_CLASSES;      // class slots (the g tile's stride)
constexpr int PR = PK / PWAVES;                 // classes (step 3) / rows (step 4) of a thread: 16
constexpr int XS = PW + 1;                      // stride of the x tile: lanes along the rows read it without conflicts
constexpr int WS = PK + 4;                      // stride of the transposed W tile: 16-byte aligned rows, staggered banks
static_assert(PB == 64 && PK == 64 && PR % 4 == 0, "the thread maps below are written for 64 x 64 tiles");

struct ProbeStep {          // the scalars of one AdamW step (host, fp64 -> fp32)
  float decay, step, bc2_sqrt, beta1, beta2, omb1, omb2, eps;
};

__device__ __forceinline__ float wave_sum_f32(float v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, kWave);
  return v;
}
__device__ __forceinline__ float wave_max_f32(float v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, kWave));
  return v;
}

__device__ __forceinline__ void adamw_one(float& p, float& m, float& v, float g, const ProbeStep& a) {
  p *= a.decay;
  m = a.beta1 * m + a.omb1 * g;
  v = a.beta2 * v + a.omb2 * g * g;
  p -= a.step * (m / (sqrtf(v) / a.bc2_sqrt + a.eps));
}

constexpr int PE = PB * PW / PT;                // elements of a 64 x 64 tile per thread: 16

// s_x[r][c] = X[perm[r]][c0 + c] for the slice's cw columns, zero behind them (the 16 gathers of a thread are independent)
__device__ __forceinline__ void stage_rows(float* s_x, const float* __restrict__ X, int ld, const int* __restrict__ perm,
                                           int c0, int cw) {
#pragma unroll
  for (int j = 0; j < PE; ++j) {
    const int i = threadIdx.x + j * PT, r = i / PW, c = i - r * PW;
    s_x[r * XS + c] = c < cw ? X[(size_t)perm[r] * ld + c0 + c] : 0.f;
  }
}

// out[r][k] = sum over the slice's columns (ascending, fused multiply-adds) of s_x[r][c] * s_wt[c][k]; a thread: row =
// lane, 16 classes
__device__ __forceinline__ void write_partials(const float* s_x, const float* s_wt, int cw, int K, float* __restrict__ out) {
  const int r = threadIdx.x & (kWave - 1), k0 = (threadIdx.x / kWave) * PR;
  float acc[PR];
#pragma unroll
  for (int j = 0; j < PR; ++j) acc[j] = 0.f;
#pragma unroll 4
  for (int c = 0; c < cw; ++c) {
    const float x = s_x[r * XS + c];
#pragma unroll
    for (int q = 0; q < PR / 4; ++q) {
      const float4 w = *reinterpret_cast<const float4*>(&s_wt[c * WS + k0 + 4 * q]);
      acc[4 * q + 0] = __builtin_fmaf(x, w.x, acc[4 * q + 0]);
      acc[4 * q + 1] = __builtin_fmaf(x, w.y, acc[4 * q + 1]);
      acc[4 * q + 2] = __builtin_fmaf(x, w.z, acc[4 * q + 2]);
      acc[4 * q + 3] = __builtin_fmaf(x, w.w, acc[4 * q + 3]);
    }
  }
#pragma unroll
  for (int j = 0; j < PR; ++j)
    if (k0 + j < K) out[(size_t)r * K + k0 + j] = acc[j];
}

// the partial logits of the FIRST batch from the initial W, and b into the buffer step 1 reads
__global__ __launch_bounds__(PT) void probe_prologue_kernel(int D, int ld, int K, const float* __restrict__ X,
                                                            const int* __restrict__ perm, const float* __restrict__ W,
                                                            const float* __restrict__ b, float* __restrict__ part,
                                                            float* __restrict__ b_buf) {
  __shared__ float s_x[PB * XS];
  __shared__ __attribute__((aligned(16))) float s_wt[PW * WS];
  const int tid = threadIdx.x, s = blockIdx.x, c0 = s * PW, cw = min(PW, D - c0);
  for (int i = tid; i < PK * PW; i += PT) {
    const int k = i / PW, c = i - k * PW;
    s_wt[c * WS + k] = (k < K && c < cw) ? W[(size_t)k * D + c0 + c] : 0.f;
  }
  if (s == 0 && tid < K) b_buf[tid] = b[tid];
  stage_rows(s_x, X, ld, perm, c0, cw);
  __syncthreads();
  write_partials(s_x, s_wt, cw, K, part + (size_t)s * PB * K);
}

// One step.  The launch is latency-bound (16 workgroups, a chain of dependent phases), so every global read that does not
// depend on this launch's arithmetic is issued before the first barrier: the batch's x tile, the NEXT batch's x tile (kept
// in registers until step 3 is through with the LDS tile), the slice of W and of both moments, and the partial tiles, 16
// independent loads per slice.
__global__ __launch_bounds__(PT) void probe_step_kernel(int D, int ld, int K, int S, const float* __restrict__ X,
                                                        const int* __restrict__ labels, const int* __restrict__ perm_cur,
                                                        const int* __restrict__ perm_next, float* __restrict__ W,
                                                        float* __restrict__ mW, float* __restrict__ vW,
                                                        float* __restrict__ mb, float* __restrict__ vb,
                                                        const float* __restrict__ part_cur, float* __restrict__ part_next,
                                                        const float* __restrict__ b_cur, float* __restrict__ b_next,
                                                        ProbeStep a) {
  __shared__ float s_x[PB * XS];
  __shared__ __attribute__((aligned(16))) float s_g[PB * PK];
  __shared__ __attribute__((aligned(16))) float s_wt[PW * WS];
  __shared__ float s_db[PWAVES * PK];
  __shared__ int s_lab[PB];
  const int tid = threadIdx.x, wave = tid / kWave, lane = tid & (kWave - 1);
  const int s = blockIdx.x, c0 = s * PW, cw = min(PW, D - c0), k0 = wave * PR;
  const int tile = PB * K;
  if (tid < PB) s_lab[tid] = labels[perm_cur[tid]];
  float xn[PE];                          // this thread's elements of the next batch's x tile
#pragma unroll
  for (int j = 0; j < PE; ++j) {
    const int i = tid + j * PT, r = i / PW, c = i - r * PW;
    xn[j] = (perm_next && c < cw) ? X[(size_t)perm_next[r] * ld + c0 + c] : 0.f;
  }
  float pw[PR], pm[PR], pv[PR];          // column c0 + lane of W, m, v for the classes k0 .. k0 + 15
#pragma unroll
  for (int j = 0; j < PR; ++j) {
    const bool in = k0 + j < K && lane < cw;
    const size_t o = in ? (size_t)(k0 + j) * D + c0 + lane : 0;
    pw[j] = in ? W[o] : 0.f;
    pm[j] = in ? mW[o] : 0.f;
    pv[j] = in ? vW[o] : 0.f;
  }
  const bool bias = s == 0 && tid < K;   // workgroup 0 also owns b
  float pb = bias ? b_cur[tid] : 0.f, pmb = bias ? mb[tid] : 0.f, pvb = bias ? vb[tid] : 0.f;
  stage_rows(s_x, X, ld, perm_cur, c0, cw);
  // 1. the logits: the S partial tiles in slice order, then the bias
  {
    float acc[PE];
#pragma unroll
    for (int j = 0; j < PE; ++j) {
      const int e = tid + j * PT;
      acc[j] = e < tile ? part_cur[e] : 0.f;
    }
#pragma unroll 4
    for (int sp = 1; sp < S; ++sp) {
      const float* __restrict__ ps = part_cur + (size_t)sp * tile;
#pragma unroll
      for (int j = 0; j < PE; ++j) {
        const int e = tid + j * PT;
        if (e < tile) acc[j] += ps[e];
      }
    }
#pragma unroll
    for (int j = 0; j < PE; ++j) {
      const int e = tid + j * PT;
      if (e < tile) {
        const int r = e / K, k = e - r * K;
        s_g[r * PK + k] = acc[j] + b_cur[k];
      }
    }
  }
  __syncthreads();
  // 2. g = (softmax - onehot) / 64, a wave per row, a lane per class (every lane touches only its own slot); the 16 rows
  //    of a wave are independent, so their butterflies are unrolled side by side.  The lane also adds its class's g over
  //    the wave's rows in row order: the bias gradient's four partial sums.
  {
    float colsum = 0.f;
#pragma unroll
    for (int i = 0; i < PB / PWAVES; ++i) {
      const int r = wave * (PB / PWAVES) + i;
      const float v = lane < K ? s_g[r * PK + lane] : -__builtin_huge_valf();
      const float mx = wave_max_f32(v);
      const float ex = lane < K ? expf(v - mx) : 0.f;
      const float sum = wave_sum_f32(ex);
      const float g = lane < K ? (ex / sum - (lane == s_lab[r] ? 1.f : 0.f)) * (1.f / PB) : 0.f;
      s_g[r * PK + lane] = g;
      colsum += g;
    }
    s_db[wave * PK + lane] = colsum;
  }
  __syncthreads();
  // 3. the slice of dW = g^T x over the rows in batch order (fused multiply-adds), then AdamW; a thread: column = lane,
  //    classes k0 .. k0 + 15
  {
    float dw[PR];
#pragma unroll
    for (int j = 0; j < PR; ++j) dw[j] = 0.f;
#pragma unroll 4
    for (int r = 0; r < PB; ++r) {
      const float x = s_x[r * XS + lane];
#pragma unroll
      for (int q = 0; q < PR / 4; ++q) {
        const float4 g = *reinterpret_cast<const float4*>(&s_g[r * PK + k0 + 4 * q]);
        dw[4 * q + 0] = __builtin_fmaf(g.x, x, dw[4 * q + 0]);
        dw[4 * q + 1] = __builtin_fmaf(g.y, x, dw[4 * q + 1]);
        dw[4 * q + 2] = __builtin_fmaf(g.z, x, dw[4 * q + 2]);
        dw[4 * q + 3] = __builtin_fmaf(g.w, x, dw[4 * q + 3]);
      }
    }
#pragma unroll
    for (int j = 0; j < PR; ++j) {
      const int k = k0 + j;
      if (k < K && lane < cw) {
        const size_t o = (size_t)k * D + c0 + lane;
        adamw_one(pw[j], pm[j], pv[j], dw[j], a);
        W[o] = pw[j];
        mW[o] = pm[j];
        vW[o] = pv[j];
      }
      s_wt[lane * WS + k] = pw[j];       // the updated slice, transposed, for step 4 (zero outside the slice)
    }
  }
  if (bias) {                            // column sums of g: the four waves' partial sums of step 2, in wave order
    float db = s_db[tid];
#pragma unroll
    for (int w = 1; w < PWAVES; ++w) db += s_db[w * PK + tid];
    adamw_one(pb, pmb, pvb, db, a);
    b_next[tid] = pb;
    mb[tid] = pmb;
    vb[tid] = pvb;
  }
  if (!perm_next) return;                // the last step: no batch follows (uniform over the grid)
  __syncthreads();                       // step 3 has read the x tile
#pragma unroll
  for (int j = 0; j < PE; ++j) {
    const int i = tid + j * PT, r = i / PW, c = i - r * PW;
    s_x[r * XS + c] = xn[j];
  }
  __syncthreads();
  // 4. the partial logits of batch t + 1 with the updated slice
  write_partials(s_x, s_wt, cw, K, part_next + (size_t)s * tile);
}

// one wave per row: logits, fp32 cross-entropy, argmax (ties to the lowest class)
__global__ __launch_bounds__(PT) void probe_eval_rows_kernel(int m, int D, int ld, int K, const float* __restrict__ X,
                                                             const int* __restrict__ labels, const float* __restrict__ W,
                                                             const float* __restrict__ b, float* __restrict__ row_loss,
                                                             int* __restrict__ row_pred, float* __restrict__ logits) {
  const int lane = threadIdx.x & (kWave - 1);
  const long long row = (long long)blockIdx.x * PWAVES + threadIdx.x / kWave;
  if (row >= m) return;
  const float* __restrict__ x = X + (size_t)row * ld;
  float mine = -__builtin_huge_valf();   // the logit of class `lane`
  for (int k = 0; k < K; ++k) {
    const float* __restrict__ w = W + (size_t)k * D;
    float acc = 0.f;
    for (int c = lane; c < D; c += kWave) acc = __builtin_fmaf(x[c], w[c], acc);
    acc = wave_sum_f32(acc);
    if (lane == k) mine = acc + b[k];
  }
  float best = mine;
  int arg = lane;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const float ov = __shfl_xor(best, o, kWave);
    const int oa = __shfl_xor(arg, o, kWave);
    if (ov > best || (ov == best && oa < arg)) best = ov, arg = oa;
  }
  const float sum = wave_sum_f32(lane < K ? expf(mine - best) : 0.f);
  const float at_label = __shfl(mine, labels[row], kWave);
  if (lane == 0) {
    row_loss[row] = -((at_label - best) - logf(sum));
    row_pred[row] = arg;
  }
  if (logits && lane < K) logits[(size_t)row * K + lane] = mine;
}

// the fp64 sum of the row losses and the count of correct rows: thread-strided partial sums, then the threads in order
__global__ __launch_bounds__(PT) void probe_eval_reduce_kernel(int m, const float* __restrict__ row_loss,
                                                               const int* __restrict__ row_pred,
                                                               const int* __restrict__ labels, double* __restrict__ loss_sum,
                                                               int* __restrict__ correct) {
  __shared__ double s_sum[PT];
  __shared__ int s_cnt[PT];
  double sum = 0.0;
  int cnt = 0;
  for (int r = threadIdx.x; r < m; r += PT) {
    sum += (double)row_loss[r];
    cnt += row_pred[r] == labels[r] ? 1 : 0;
  }
  s_sum[threadIdx.x] = sum;
  s_cnt[threadIdx.x] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int t = 1; t < PT; ++t) sum += s_sum[t], cnt += s_cnt[t];
    *loss_sum = sum;
    *correct = cnt;
  }
}

inline int slices(int D) { return (D + PW - 1) / PW; }

}  // namespace
}  // namespace pdae

using namespace pdae;

extern "C" int pdae_linear_probe_supported(int n, int D, int ld, int K) {
  if (n < 0) return bad_arg("linear_probe: n >= 0 required");
  if (D < 1 || ld < D) return bad_arg("linear_probe: D >= 1 and ld >= D required");
  if (K < 2) return bad_arg("linear_probe: the number of classes has to be greater than one");
  if (K > PK) return unsupported("linear_probe: more than PDAE_PROBE_MAX_CLASSES (64) classes");
  return PDAE_OK;
}

extern "C" long long pdae_linear_probe_workspace(int D, int K) {
  if (D < 1 || K < 1) return 0;
  return 2LL * K * D + 4LL * K + 2LL * slices(D) * PB * K;
}

extern "C" int pdae_linear_probe_train(int n, int D, int ld, int K, int epochs, const float* X, const int32_t* labels,
                                       const int32_t* perm, float* W, float* b, const double* lr, double beta1, double beta2,
                                       double eps, double weight_decay, float* workspace, pdae_stream_t stream) {
  const int ok = pdae_linear_probe_supported(n, D, ld, K);
  if (ok != PDAE_OK) return ok;
  if (epochs < 0) return bad_arg("linear_probe_train: epochs >= 0 required");
  const int nb = n / PB;
  if (nb == 0 || epochs == 0) return PDAE_OK;          // nothing to train: W and b keep their initial values
  if (!X || !labels || !perm || !W || !b || !lr || !workspace) return bad_arg("linear_probe_train: null pointer");
  if (!(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0)) return bad_arg("linear_probe_train: 0 <= beta < 1 required");
  const long long total = (long long)epochs * nb;
  if (total > 0x7fffffffLL) return unsupported("linear_probe_train: more than 2^31 - 1 steps");
  hipStream_t s = as_stream(stream);
  const int S = slices(D);
  const size_t KD = (size_t)K * D, tile = (size_t)S * PB * K;
  float *mW = workspace, *vW = mW + KD, *mb = vW + KD, *vb = mb + K, *b_buf = vb + K, *part = b_buf + 2 * K;
  if (hipMemsetAsync(mW, 0, (2 * KD + 2 * (size_t)K) * sizeof(float), s) != hipSuccess) {
    (void)hipGetLastError();
    set_error("linear_probe_train: hipMemsetAsync failed");
    return PDAE_ERR_LAUNCH;
  }
  // step t (1-based) reads the buffers of parity t & 1 and writes the others; the last step writes b itself
  hipLaunchKernelGGL(probe_prologue_kernel, dim3(S), dim3(PT), 0, s, D, ld, K, X, perm, W, b, part + tile, b_buf + K);
  int rc = check_launch("linear_probe_train");
  if (rc != PDAE_OK) return rc;
  long long t = 0;
  for (int e = 0; e < epochs; ++e) {
    const int32_t* pe = perm + (size_t)e * n;
    for (int i = 0; i < nb; ++i) {
      ++t;
      const double bc1 = 1.0 - pow(beta1, (double)t), bc2 = 1.0 - pow(beta2, (double)t);
      ProbeStep a;
      a.decay = (float)(1.0 - lr[e] * weight_decay);
      a.step = (float)(lr[e] / bc1);
      a.bc2_sqrt = (float)sqrt(bc2);
      a.beta1 = (float)beta1;
      a.beta2 = (float)beta2;
      a.omb1 = (float)(1.0 - beta1);
      a.omb2 = (float)(1.0 - beta2);
      a.eps = (float)eps;
      const int cur = (int)(t & 1), nxt = cur ^ 1;
      const int32_t* next = t == total ? nullptr : (i + 1 < nb ? pe + (size_t)(i + 1) * PB : pe + n);
      hipLaunchKernelGGL(probe_step_kernel, dim3(S), dim3(PT), 0, s, D, ld, K, S, X, labels, pe + (size_t)i * PB, next, W,
                         mW, vW, mb, vb, part + cur * tile, part + nxt * tile, b_buf + cur * K,
                         t == total ? b : b_buf + nxt * K, a);
    }
    rc = check_launch("linear_probe_train");
    if (rc != PDAE_OK) return rc;
  }
  return PDAE_OK;
}

extern "C" int pdae_linear_probe_eval(int m, int D, int ld, int K, const float* X, const int32_t* labels, const float* W,
                                      const float* b, float* row_loss, int32_t* row_pred, float* logits, double* loss_sum,
                                      int32_t* correct, pdae_stream_t stream) {
  const int ok = pdae_linear_probe_supported(m, D, ld, K);
  if (ok != PDAE_OK) return ok;
  if (m < 1) return bad_arg("linear_probe_eval: m >= 1 required");
  if (!X || !labels || !W || !b || !row_loss || !row_pred || !loss_sum || !correct)
    return bad_arg("linear_probe_eval: null pointer");
  hipStream_t s = as_stream(stream);
  hipLaunchKernelGGL(probe_eval_rows_kernel, dim3((m + PWAVES - 1) / PWAVES), dim3(PT), 0, s, m, D, ld, K, X, labels, W, b,
                     row_loss, row_pred, logits);
  hipLaunchKernelGGL(probe_eval_reduce_kernel, dim3(1), dim3(PT), 0, s, m, row_loss, row_pred, labels, loss_sum, correct);
  return check_launch("linear_probe_eval");
}
