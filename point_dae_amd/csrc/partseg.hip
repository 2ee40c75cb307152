// partseg.hip -- the part-segmentation head of PointTransformerPartSeg in evaluation mode, forward only.
//
// Reference: segmentation/models/pt.py:301-333 (get_model.forward) on segmentation/models/pointnet2_utils.py:262-312
// (PointNetFeaturePropagation) and the metric of segmentation/main.py:246-295, with every BatchNorm on its running
// estimates (scale_l = gamma / sqrt(var + eps), shift_l = beta - mean * scale_l).
//
// The propagation layer's first conv is linear in the interpolated token features, and the three interpolation weights
// sum to one, so its feature columns run once per TOKEN (T = F W0f^T + b0 on the row GEMM, G rows per cloud) and
//
//   partseg_propagate   a0[b, n, :] = relu(s0 (sum_k w_k T[b, idx_k, :] + W0x p) + t0)
//
// finds the three nearest of the cloud's G centres per point (centres in LDS, squared distances as direct differences
// ((dx dx + dy dy) + dz dz), strict `<` insertion: ties keep the lower index), forms w_k = r_k / (r_0 + r_1 + r_2) with
// r_k = 1 / (d_k + 1e-8) -- a point that IS a centre has d = 0 and gets 1e8 / (1e8 + ..), no special case -- and writes
// the (B N, C) activation the next row GEMM reads.  A block owns 32 consecutive points of ONE cloud: one wave picks their
// neighbours, then all four waves sweep the 32 x C outputs four channels per lane (coalesced 16-byte loads of T, which
// is 768 KB per cloud and stays in L2, and coalesced 16-byte stores).
//
//   partseg_token_pool        [max_G F | mean_G F] per cloud, the two halves the head concatenates separately
//   partseg_cloud_bias_relu   y[b, n, :] = relu(y[b, n, :] + gbias[b, :]) in place: the per-cloud global term of convs1
//   partseg_tail              one pass over the 256-wide output of convs2 per point: affine + ReLU, the 50 x 256 last
//                             layer (W3 in LDS, read as wave-wide broadcasts; a row's activation streams through a
//                             padded LDS tile in chunks of 16 channels; 50 fp32 accumulators per lane, k ascending,
//                             fused multiply-adds), log-softmax as (x - max) - log sum exp(x - max), the argmax over
//                             the shape's own part range (first index on ties) and the metric's integer counts: LDS
//                             integer atomics per block, one global integer atomic per touched counter.  Integer sums
//                             are exact in any order: two runs give the same bits.
#include "common.h"

namespace pdae {
namespace {

constexpr int PS_MAXG = 256;     // centres per cloud the propagate kernel keeps in LDS
constexpr int PS_PTS = 32;       // points per block of the propagate kernel
constexpr int TL_ROWS = 128;     // points per block of the tail kernel (one per lane)
constexpr int TL_K = 256;        // the tail's input width
constexpr int TL_P = 50;         // part labels
constexpr int TL_KC = 16;        // channels per staged chunk

// grid (ceil(C / 256), B)
__global__ __launch_bounds__(256) void partseg_token_pool_kernel(int G, int C, const float* __restrict__ F,
                                                                 float* __restrict__ out) {
  const int c = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (c >= C) return;
  const float* f = F + (size_t)b * G * C + c;
  float m = f[0], s = f[0];
  for (int g = 1; g < G; ++g) {
    const float v = f[(size_t)g * C];
    m = fmaxf(m, v);
    s += v;
  }
  out[(size_t)b * 2 * C + c] = m;
  out[(size_t)b * 2 * C + C + c] = s / (float)G;
}

// grid (ceil(N / 32), B), block 256
__global__ __launch_bounds__(256) void partseg_propagate_kernel(int N, int G, int C, const float* __restrict__ pts,
                                                                const float* __restrict__ ctr, const float* __restrict__ T,
                                                                const float* __restrict__ W0x, const float* __restrict__ s0,
                                                                const float* __restrict__ t0, float* __restrict__ out,
                                                                int* __restrict__ idx3) {
  __shared__ float Cs[PS_MAXG * 3];
  __shared__ float Ws[PS_PTS * 4];       // the three weights
  __shared__ float Ps[PS_PTS * 4];       // the point
  __shared__ int Is[PS_PTS * 4];         // the three token rows (b * G + idx)
  const int b = blockIdx.y, n0 = blockIdx.x * PS_PTS;
  for (int i = threadIdx.x; i < G * 3; i += 256) Cs[i] = ctr[(size_t)b * G * 3 + i];
  __syncthreads();

  if (threadIdx.x < PS_PTS && n0 + (int)threadIdx.x < N) {
    const size_t row = (size_t)b * N + n0 + threadIdx.x;
    const float px = pts[row * 3], py = pts[row * 3 + 1], pz = pts[row * 3 + 2];
    float d0 = INFINITY, d1 = INFINITY, d2 = INFINITY;
    int i0 = 0, i1 = 0, i2 = 0;
    for (int g = 0; g < G; ++g) {
      const float d = sqdist(px, py, pz, Cs[g * 3], Cs[g * 3 + 1], Cs[g * 3 + 2]);
      if (d < d0) {
        d2 = d1, i2 = i1, d1 = d0, i1 = i0, d0 = d, i0 = g;
      } else if (d < d1) {
        d2 = d1, i2 = i1, d1 = d, i1 = g;
      } else if (d < d2) {
        d2 = d, i2 = g;
      }
    }
    const float r0 = 1.0f / (d0 + 1e-8f), r1 = 1.0f / (d1 + 1e-8f), r2 = 1.0f / (d2 + 1e-8f);
    const float norm = (r0 + r1) + r2;
    const int t = threadIdx.x * 4;
    Ws[t] = r0 / norm, Ws[t + 1] = r1 / norm, Ws[t + 2] = r2 / norm;
    Ps[t] = px, Ps[t + 1] = py, Ps[t + 2] = pz;
    Is[t] = b * G + i0, Is[t + 1] = b * G + i1, Is[t + 2] = b * G + i2;
    if (idx3) idx3[row * 3] = i0, idx3[row * 3 + 1] = i1, idx3[row * 3 + 2] = i2;
  }
  __syncthreads();

  const int Q = C / 4, rows = min(PS_PTS, N - n0);
  for (int i = threadIdx.x; i < rows * Q; i += 256) {
    const int row = i / Q, c = (i % Q) * 4, t = row * 4;
    const float w0 = Ws[t], w1 = Ws[t + 1], w2 = Ws[t + 2];
    const float px = Ps[t], py = Ps[t + 1], pz = Ps[t + 2];
    const float4 a = *reinterpret_cast<const float4*>(T + (size_t)Is[t] * C + c);
    const float4 bq = *reinterpret_cast<const float4*>(T + (size_t)Is[t + 1] * C + c);
    const float4 cq = *reinterpret_cast<const float4*>(T + (size_t)Is[t + 2] * C + c);
    const float4 sc = *reinterpret_cast<const float4*>(s0 + c), sh = *reinterpret_cast<const float4*>(t0 + c);
    const float av[4] = {a.x, a.y, a.z, a.w}, bv[4] = {bq.x, bq.y, bq.z, bq.w}, cv[4] = {cq.x, cq.y, cq.z, cq.w};
    const float scv[4] = {sc.x, sc.y, sc.z, sc.w}, shv[4] = {sh.x, sh.y, sh.z, sh.w};
    float o[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float* wx = W0x + (size_t)(c + q) * 3;
      const float f = __builtin_fmaf(w2, cv[q], __builtin_fmaf(w1, bv[q], w0 * av[q]));
      const float y = __builtin_fmaf(wx[2], pz, __builtin_fmaf(wx[1], py, __builtin_fmaf(wx[0], px, f)));
      o[q] = fmaxf(y * scv[q] + shv[q], 0.f);
    }
    *reinterpret_cast<float4*>(out + ((size_t)b * N + n0 + row) * C + c) = make_float4(o[0], o[1], o[2], o[3]);
  }
}

// total = B * N * C / 4 quads; grid-stride
__global__ __launch_bounds__(256) void partseg_cloud_bias_relu_kernel(long long total, int N, int C, float* __restrict__ y,
                                                                      const float* __restrict__ gbias) {
  const int Q = C / 4;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const long long row = i / Q;
    const int c = (int)(i % Q) * 4, b = (int)(row / N);
    float4 v = *reinterpret_cast<float4*>(y + row * C + c);
    const float4 g = *reinterpret_cast<const float4*>(gbias + (size_t)b * C + c);
    v.x = fmaxf(v.x + g.x, 0.f), v.y = fmaxf(v.y + g.y, 0.f), v.z = fmaxf(v.z + g.z, 0.f), v.w = fmaxf(v.w + g.w, 0.f);
    *reinterpret_cast<float4*>(y + row * C + c) = v;
  }
}

// grid (ceil(N / 128), S), block 128: a block's points belong to ONE shape
__global__ __launch_bounds__(TL_ROWS) void partseg_tail_kernel(int N, const float* __restrict__ y, const float* __restrict__ sc,
                                                               const float* __restrict__ sh, const float* __restrict__ W3,
                                                               const float* __restrict__ b3, const int* __restrict__ seg,
                                                               const int* __restrict__ lo_, const int* __restrict__ hi_,
                                                               float* __restrict__ logp, int* __restrict__ pred,
                                                               int* __restrict__ shape_iu, int* __restrict__ shape_correct,
                                                               int* __restrict__ part_seen, int* __restrict__ part_correct) {
  __shared__ float Wsm[TL_P * TL_K];
  __shared__ float Hs[TL_ROWS * (TL_KC + 1)];
  __shared__ int cnt[4 * TL_P + 1];            // intersection, union, seen, correct per label; the shape's correct points
  const int s = blockIdx.y, n0 = blockIdx.x * TL_ROWS, tid = threadIdx.x;
  const int rows = min(TL_ROWS, N - n0);
  for (int i = tid; i < TL_P * TL_K / 4; i += TL_ROWS)
    reinterpret_cast<float4*>(Wsm)[i] = reinterpret_cast<const float4*>(W3)[i];
  for (int i = tid; i < 4 * TL_P + 1; i += TL_ROWS) cnt[i] = 0;

  float acc[TL_P];
#pragma unroll
  for (int c = 0; c < TL_P; ++c) acc[c] = b3[c];
  const size_t base = (size_t)s * N + n0;
  for (int kc = 0; kc < TL_K; kc += TL_KC) {
    __syncthreads();                             // the previous chunk has been read (first pass: Wsm and cnt are written)
#pragma unroll
    for (int j = 0; j < TL_KC / 4; ++j) {
      const int i = tid + TL_ROWS * j, row = i / (TL_KC / 4), q = (i % (TL_KC / 4)) * 4;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (row < rows) {
        v = *reinterpret_cast<const float4*>(y + (base + row) * TL_K + kc + q);
        const float4 a = *reinterpret_cast<const float4*>(sc + kc + q), d = *reinterpret_cast<const float4*>(sh + kc + q);
        v.x = fmaxf(v.x * a.x + d.x, 0.f), v.y = fmaxf(v.y * a.y + d.y, 0.f);
        v.z = fmaxf(v.z * a.z + d.z, 0.f), v.w = fmaxf(v.w * a.w + d.w, 0.f);
      }
      float* h = Hs + row * (TL_KC + 1) + q;
      h[0] = v.x, h[1] = v.y, h[2] = v.z, h[3] = v.w;
    }
    __syncthreads();
#pragma unroll
    for (int k4 = 0; k4 < TL_KC; k4 += 4) {
      const float* h = Hs + tid * (TL_KC + 1) + k4;
      const float a0 = h[0], a1 = h[1], a2 = h[2], a3 = h[3];
#pragma unroll
      for (int c = 0; c < TL_P; ++c) {
        const float4 w = *reinterpret_cast<const float4*>(Wsm + c * TL_K + kc + k4);      // one address per wave: a broadcast
        acc[c] = __builtin_fmaf(a3, w.w, __builtin_fmaf(a2, w.z, __builtin_fmaf(a1, w.y, __builtin_fmaf(a0, w.x, acc[c]))));
      }
    }
  }

  if (tid < rows) {
    const size_t r = base + tid;
    float m = acc[0];
#pragma unroll
    for (int c = 1; c < TL_P; ++c) m = fmaxf(m, acc[c]);
    float sum = 0.f;
#pragma unroll
    for (int c = 0; c < TL_P; ++c) sum += expf(acc[c] - m);
    const float lse = logf(sum);
    int lo = lo_ ? lo_[s] : 0, hi = hi_ ? hi_[s] : TL_P - 1;
    lo = min(max(lo, 0), TL_P - 1), hi = min(hi, TL_P - 1);
    float best = -INFINITY;
    int arg = lo;
#pragma unroll
    for (int c = 0; c < TL_P; ++c) {
      const float lp = (acc[c] - m) - lse;
      logp[r * TL_P + c] = lp;
      if (c >= lo && c <= hi && lp > best) best = lp, arg = c;
    }
    pred[r] = arg;
    if (seg) {
      const int g = seg[r];
      const bool known = g >= 0 && g < TL_P;
      atomicAdd(&cnt[TL_P + arg], 1);                                    // union: the predicted label
      if (g == arg) {
        atomicAdd(&cnt[arg], 1);
        atomicAdd(&cnt[3 * TL_P + arg], 1);
        atomicAdd(&cnt[4 * TL_P], 1);
      } else if (known && g >= lo && g <= hi) {
        atomicAdd(&cnt[TL_P + g], 1);                                    // union: the true label, inside the shape's range
      }
      if (known) atomicAdd(&cnt[2 * TL_P + g], 1);
    }
  }
  if (!seg) return;                                                      // (uniform over the launch)
  __syncthreads();
  if (tid < TL_P) {
    if (cnt[tid]) atomicAdd(shape_iu + ((size_t)s * 2) * TL_P + tid, cnt[tid]);
    if (cnt[TL_P + tid]) atomicAdd(shape_iu + ((size_t)s * 2 + 1) * TL_P + tid, cnt[TL_P + tid]);
    if (cnt[2 * TL_P + tid]) atomicAdd(part_seen + tid, cnt[2 * TL_P + tid]);
    if (cnt[3 * TL_P + tid]) atomicAdd(part_correct + tid, cnt[3 * TL_P + tid]);
  }
  if (tid == 0 && cnt[4 * TL_P]) atomicAdd(shape_correct + s, cnt[4 * TL_P]);
}

}  // namespace
}  // namespace pdae

using namespace pdae;

extern "C" int pdae_partseg_supported(int G, int C, int K, int P) {
  return G >= 3 && G <= PS_MAXG && C >= 4 && C % 4 == 0 && K == TL_K && P == TL_P ? 1 : 0;
}

extern "C" int pdae_partseg_token_pool(int B, int G, int C, const float* F, float* out, pdae_stream_t stream) {
  if (B < 0 || G <= 0 || C <= 0) return bad_arg("partseg_token_pool: bad size");
  if (B > 65535) return unsupported("partseg_token_pool: more than 65535 clouds");
  if (B == 0) return PDAE_OK;
  if (!F || !out) return bad_arg("partseg_token_pool: null pointer");
  hipLaunchKernelGGL(partseg_token_pool_kernel, dim3((unsigned)((C + 255) / 256), (unsigned)B), dim3(256), 0,
                     as_stream(stream), G, C, F, out);
  return check_launch("partseg_token_pool");
}

extern "C" int pdae_partseg_propagate(int B, int N, int G, int C, const float* pts, const float* centres, const float* T,
                                      const float* W0x, const float* scale0, const float* shift0, float* a0, int32_t* idx3,
                                      pdae_stream_t stream) {
  if (B < 0 || N <= 0 || G <= 0 || C <= 0) return bad_arg("partseg_propagate: bad size");
  if (!pdae_partseg_supported(G, C, TL_K, TL_P))
    return unsupported("partseg_propagate: 3 to 256 centres per cloud and a width that is a multiple of 4 required");
  if ((long long)B * N >= (1LL << 31) || (long long)B * G >= (1LL << 31) || B > 65535)
    return unsupported("partseg_propagate: too many points");
  if (B == 0) return PDAE_OK;
  if (!pts || !centres || !T || !W0x || !scale0 || !shift0 || !a0) return bad_arg("partseg_propagate: null pointer");
  if (((uintptr_t)T | (uintptr_t)scale0 | (uintptr_t)shift0 | (uintptr_t)a0) & 15)
    return bad_arg("partseg_propagate: T, scale0, shift0 and a0 must be 16-byte aligned");
  hipLaunchKernelGGL(partseg_propagate_kernel, dim3((unsigned)((N + PS_PTS - 1) / PS_PTS), (unsigned)B), dim3(256), 0,
                     as_stream(stream), N, G, C, pts, centres, T, W0x, scale0, shift0, a0, idx3);
  return check_launch("partseg_propagate");
}

extern "C" int pdae_partseg_cloud_bias_relu(int B, int N, int C, float* y, const float* gbias, pdae_stream_t stream) {
  if (B < 0 || N <= 0 || C <= 0) return bad_arg("partseg_cloud_bias_relu: bad size");
  if (C % 4 != 0) return unsupported("partseg_cloud_bias_relu: a width that is a multiple of 4 required");
  if (B == 0) return PDAE_OK;
  if (!y || !gbias) return bad_arg("partseg_cloud_bias_relu: null pointer");
  if (((uintptr_t)y | (uintptr_t)gbias) & 15) return bad_arg("partseg_cloud_bias_relu: y and gbias must be 16-byte aligned");
  const long long total = (long long)B * N * (C / 4);
  const long long blocks = (total + 255) / 256;
  hipLaunchKernelGGL(partseg_cloud_bias_relu_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0,
                     as_stream(stream), total, N, C, y, gbias);
  return check_launch("partseg_cloud_bias_relu");
}

extern "C" int pdae_partseg_tail(int S, int N, int K, int P, const float* y, const float* scale, const float* shift,
                                 const float* W3, const float* b3, const int32_t* seg, const int32_t* lo, const int32_t* hi,
                                 float* logp, int32_t* pred, int32_t* shape_iu, int32_t* shape_correct, int32_t* part_seen,
                                 int32_t* part_correct, pdae_stream_t stream) {
  if (S < 0 || N <= 0 || K <= 0 || P <= 0) return bad_arg("partseg_tail: bad size");
  if (K != TL_K || P != TL_P) return unsupported("partseg_tail: a 256-wide input and 50 part labels required");
  if ((long long)S * N >= (1LL << 31) / TL_K || S > 65535) return unsupported("partseg_tail: too many points");
  if (S == 0) return PDAE_OK;
  if (!y || !scale || !shift || !W3 || !b3 || !logp || !pred) return bad_arg("partseg_tail: null pointer");
  if (seg && (!shape_iu || !shape_correct || !part_seen || !part_correct))
    return bad_arg("partseg_tail: the counts go with seg");
  if (((uintptr_t)y | (uintptr_t)scale | (uintptr_t)shift | (uintptr_t)W3) & 15)
    return bad_arg("partseg_tail: y, scale, shift and W3 must be 16-byte aligned");
  hipLaunchKernelGGL(partseg_tail_kernel, dim3((unsigned)((N + TL_ROWS - 1) / TL_ROWS), (unsigned)S), dim3(TL_ROWS), 0,
                     as_stream(stream), N, y, scale, shift, W3, b3, seg, lo, hi, logp, pred, shape_iu, shape_correct,
                     part_seen, part_correct);
  return check_launch("partseg_tail");
}

// ---- the DGCNN part-segmentation head (segmentation/models/dgcnn_partseg.py:124-140) -----------------------------------
//   partseg_cloud_bias_lrelu   y[b, n, :] = lrelu(y[b, n, :] + gbias[b, :]) in place: conv8's 1088 per-cloud columns
//                              [global feature | label feature] as a per-cloud bias behind the 192 per-point columns
//   partseg_logits_tail        one pass over the 128-wide output of conv10 per point: bn10's affine + LeakyReLU, the
//                              50 x 128 conv11 (as partseg_tail: W in LDS read as wave-wide broadcasts, the activation
//                              through a padded LDS tile in chunks of 16 channels, 50 accumulators per lane, k ascending,
//                              fused multiply-adds), the RAW logits (the DGCNN returns no log-softmax), the argmax of the
//                              stored logits over the shape's part range and partseg_tail's counts.
namespace pdae {
namespace {

constexpr int LT_K = 128;        // the logits tail's input width

// total = B * N * C / 4 quads; grid-stride
__global__ __launch_bounds__(256) void partseg_cloud_bias_lrelu_kernel(long long total, int N, int C, float slope,
                                                                       float* __restrict__ y,
                                                                       const float* __restrict__ gbias) {
  const int Q = C / 4;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const long long row = i / Q;
    const int c = (int)(i % Q) * 4, b = (int)(row / N);
    float4 v = *reinterpret_cast<float4*>(y + row * C + c);
    const float4 g = *reinterpret_cast<const float4*>(gbias + (size_t)b * C + c);
    v.x += g.x, v.y += g.y, v.z += g.z, v.w += g.w;
    v.x = v.x > 0.f ? v.x : slope * v.x, v.y = v.y > 0.f ? v.y : slope * v.y;
    v.z = v.z > 0.f ? v.z : slope * v.z, v.w = v.w > 0.f ? v.w : slope * v.w;
    *reinterpret_cast<float4*>(y + row * C + c) = v;
  }
}

// grid (ceil(N / 128), S), block 128: a block's points belong to ONE shape
__global__ __launch_bounds__(TL_ROWS) void partseg_logits_tail_kernel(
    int N, const float* __restrict__ y, const float* __restrict__ sc, const float* __restrict__ sh, float slope,
    const float* __restrict__ W, const float* __restrict__ bias, const int* __restrict__ seg, const int* __restrict__ lo_,
    const int* __restrict__ hi_, float* __restrict__ logits, int* __restrict__ pred, int* __restrict__ shape_iu,
    int* __restrict__ shape_correct, int* __restrict__ part_seen, int* __restrict__ part_correct) {
  __shared__ float Wsm[TL_P * LT_K];
  __shared__ float Hs[TL_ROWS * (TL_KC + 1)];
  __shared__ int cnt[4 * TL_P + 1];            // intersection, union, seen, correct per label; the shape's correct points
  const int s = blockIdx.y, n0 = blockIdx.x * TL_ROWS, tid = threadIdx.x;
  const int rows = min(TL_ROWS, N - n0);
  for (int i = tid; i < TL_P * LT_K / 4; i += TL_ROWS)
    reinterpret_cast<float4*>(Wsm)[i] = reinterpret_cast<const float4*>(W)[i];
  for (int i = tid; i < 4 * TL_P + 1; i += TL_ROWS) cnt[i] = 0;

  float acc[TL_P];
#pragma unroll
  for (int c = 0; c < TL_P; ++c) acc[c] = bias ? bias[c] : 0.f;
  const size_t base = (size_t)s * N + n0;
  for (int kc = 0; kc < LT_K; kc += TL_KC) {
    __syncthreads();                             // the previous chunk has been read (first pass: Wsm and cnt are written)
#pragma unroll
    for (int j = 0; j < TL_KC / 4; ++j) {
      const int i = tid + TL_ROWS * j, row = i / (TL_KC / 4), q = (i % (TL_KC / 4)) * 4;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (row < rows) {
        v = *reinterpret_cast<const float4*>(y + (base + row) * LT_K + kc + q);
        const float4 a = *reinterpret_cast<const float4*>(sc + kc + q), d = *reinterpret_cast<const float4*>(sh + kc + q);
        v.x = v.x * a.x + d.x, v.y = v.y * a.y + d.y, v.z = v.z * a.z + d.z, v.w = v.w * a.w + d.w;
        v.x = v.x > 0.f ? v.x : slope * v.x, v.y = v.y > 0.f ? v.y : slope * v.y;
        v.z = v.z > 0.f ? v.z : slope * v.z, v.w = v.w > 0.f ? v.w : slope * v.w;
      }
      float* h = Hs + row * (TL_KC + 1) + q;
      h[0] = v.x, h[1] = v.y, h[2] = v.z, h[3] = v.w;
    }
    __syncthreads();
#pragma unroll
    for (int k4 = 0; k4 < TL_KC; k4 += 4) {
      const float* h = Hs + tid * (TL_KC + 1) + k4;
      const float a0 = h[0], a1 = h[1], a2 = h[2], a3 = h[3];
#pragma unroll
      for (int c = 0; c < TL_P; ++c) {
        const float4 w = *reinterpret_cast<const float4*>(Wsm + c * LT_K + kc + k4);      // one address per wave: a broadcast
        acc[c] = __builtin_fmaf(a3, w.w, __builtin_fmaf(a2, w.z, __builtin_fmaf(a1, w.y, __builtin_fmaf(a0, w.x, acc[c]))));
      }
    }
  }

  if (tid < rows) {
    const size_t r = base + tid;
    int lo = lo_ ? lo_[s] : 0, hi = hi_ ? hi_[s] : TL_P - 1;
    lo = min(max(lo, 0), TL_P - 1), hi = min(hi, TL_P - 1);
    float best = -INFINITY;
    int arg = lo;
#pragma unroll
    for (int c = 0; c < TL_P; ++c) {
      logits[r * TL_P + c] = acc[c];
      if (c >= lo && c <= hi && acc[c] > best) best = acc[c], arg = c;
    }
    pred[r] = arg;
    if (seg) {
      const int g = seg[r];
      const bool known = g >= 0 && g < TL_P;
      atomicAdd(&cnt[TL_P + arg], 1);                                    // union: the predicted label
      if (g == arg) {
        atomicAdd(&cnt[arg], 1);
        atomicAdd(&cnt[3 * TL_P + arg], 1);
        atomicAdd(&cnt[4 * TL_P], 1);
      } else if (known && g >= lo && g <= hi) {
        atomicAdd(&cnt[TL_P + g], 1);                                    // union: the true label, inside the shape's range
      }
      if (known) atomicAdd(&cnt[2 * TL_P + g], 1);
    }
  }
  if (!seg) return;                                                      // (uniform over the launch)
  __syncthreads();
  if (tid < TL_P) {
    if (cnt[tid]) atomicAdd(shape_iu + ((size_t)s * 2) * TL_P + tid, cnt[tid]);
    if (cnt[TL_P + tid]) atomicAdd(shape_iu + ((size_t)s * 2 + 1) * TL_P + tid, cnt[TL_P + tid]);
    if (cnt[2 * TL_P + tid]) atomicAdd(part_seen + tid, cnt[2 * TL_P + tid]);
    if (cnt[3 * TL_P + tid]) atomicAdd(part_correct + tid, cnt[3 * TL_P + tid]);
  }
  if (tid == 0 && cnt[4 * TL_P]) atomicAdd(shape_correct + s, cnt[4 * TL_P]);
}

}  // namespace
}  // namespace pdae

extern "C" int pdae_partseg_cloud_bias_lrelu(int B, int N, int C, float* y, const float* gbias, float slope,
                                             pdae_stream_t stream) {
  if (B < 0 || N <= 0 || C <= 0) return bad_arg("partseg_cloud_bias_lrelu: bad size");
  if (C % 4 != 0) return unsupported("partseg_cloud_bias_lrelu: a width that is a multiple of 4 required");
  if (B == 0) return PDAE_OK;
  if (!y || !gbias) return bad_arg("partseg_cloud_bias_lrelu: null pointer");
  if (((uintptr_t)y | (uintptr_t)gbias) & 15) return bad_arg("partseg_cloud_bias_lrelu: y and gbias must be 16-byte aligned");
  const long long total = (long long)B * N * (C / 4);
  const long long blocks = (total + 255) / 256;
  hipLaunchKernelGGL(partseg_cloud_bias_lrelu_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0,
                     as_stream(stream), total, N, C, slope, y, gbias);
  return check_launch("partseg_cloud_bias_lrelu");
}

extern "C" int pdae_partseg_logits_tail(int S, int N, int K, int P, const float* y, const float* scale, const float* shift,
                                        float slope, const float* W, const float* bias, const int32_t* seg,
                                        const int32_t* lo, const int32_t* hi, float* logits, int32_t* pred,
                                        int32_t* shape_iu, int32_t* shape_correct, int32_t* part_seen,
                                        int32_t* part_correct, pdae_stream_t stream) {
  if (S < 0 || N <= 0 || K <= 0 || P <= 0) return bad_arg("partseg_logits_tail: bad size");
  if (K != LT_K || P != TL_P) return unsupported("partseg_logits_tail: a 128-wide input and 50 part labels required");
  if ((long long)S * N >= (1LL << 31) / LT_K || S > 65535) return unsupported("partseg_logits_tail: too many points");
  if (S == 0) return PDAE_OK;
  if (!y || !scale || !shift || !W || !logits || !pred) return bad_arg("partseg_logits_tail: null pointer");
  if (seg && (!shape_iu || !shape_correct || !part_seen || !part_correct))
    return bad_arg("partseg_logits_tail: the counts go with seg");
  if (((uintptr_t)y | (uintptr_t)scale | (uintptr_t)shift | (uintptr_t)W) & 15)
    return bad_arg("partseg_logits_tail: y, scale, shift and W must be 16-byte aligned");
  hipLaunchKernelGGL(partseg_logits_tail_kernel, dim3((unsigned)((N + TL_ROWS - 1) / TL_ROWS), (unsigned)S), dim3(TL_ROWS), 0,
                     as_stream(stream), N, y, scale, shift, slope, W, bias, seg, lo, hi, logits, pred, shape_iu,
                     shape_correct, part_seen, part_correct);
  return check_launch("partseg_logits_tail");
}
