// edge2_eval.hip -- a TWO-layer EdgeConv of the DGCNN part-segmentation encoder in evaluation mode as ONE forward-only
// kernel.
//
// Reference: segmentation/models/dgcnn_util.py:140-193 (dgcnn_encoder_partseg: conv1 + conv2 and conv3 + conv4, each pair
// Conv2d 1x1 (no bias) -> BatchNorm2d -> LeakyReLU(0.2) twice, then the max over the 20 neighbours), with every BatchNorm
// on its running estimates: scale_l = gamma / sqrt(var + eps), shift_l = beta - mean * scale_l.
//
//   out[r, c] = max_j lrelu(scale2[c] (W2[c, :] . h[r][j][:]) + shift2[c])
//   h[r][j][:] = lrelu(scale1 (p[idx[r][j]] + q[r]) + shift1)
//
// [p | q] = x [W1; W2 - W1]^T is the first layer per POINT (conv([x_j - x_i, x_i]) = p[j] + q[i], one row GEMM by the
// caller); the second layer is per EDGE, so the one-layer trick (the winner by the sign of gamma) does not apply.
//
// Block shape: 256 threads (four waves) own E2_ROWS = 128 edge rows = floor(128 / k) consecutive points with their k
// rows each, packed densely (k = 20: six points, 120 rows; the rows behind them are zero padding).  A point never
// straddles two blocks, a block may straddle two clouds (the cloud of a point is row / n), the last block may hold
// fewer points.  The block gathers the rows' p entries (256-byte rows that stay in L2: a cloud's p is 512 KB) and forms
// h in LDS, 128 x 64 with rows padded by 4 floats (conflict-free ds_read_b128).  The 64 x 64 product is fp32-input
// v_mfma_f32_32x32x2_f32 tiles -- bit for bit ONE fp32 fma chain per output, one rounding per product, in the fixed order
// k = 0, 4, 1, 5, 2, 6, 3, 7 within every eight (a lane half loads four consecutive k as one float4, and MFMA i of a group
// takes element i of both halves; A and B use the same map) --, A from LDS, B straight from W2 in global
// memory (16 KB: L2 / L1 resident).  Wave w owns row tile w and both column tiles, so it reads and later overwrites only
// its own 32 rows of the buffer: layer 2's activation lrelu(scale2 acc + shift2) replaces h in place.  Then every thread
// owns one channel of one point at a time and takes the max over that point's k rows of the buffer, starting from the
// FIRST edge (LeakyReLU outputs are negative: never from 0), j ascending: padding rows and the next point's rows are
// never read.  No atomics; the same bits every run.  Only (b n, 64) is written (twice with out2: the concatenation).
//
// LDS per block: 128 x 68 x 4 = 34,816 B (h / layer-2 activation) + 512 B (source rows) = 35,328 B -> four blocks per CU
// (160 KB / 35,328 = 4.6), 16 waves per CU.
#include "common.h"

namespace pdae {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int E2_ROWS = 128;     // edge rows per block
constexpr int E2_C = 64;         // C1 = C2
constexpr int E2_LD = E2_C + 4;  // leading dimension of the LDS buffer
constexpr int E2_MAXK = 32;
constexpr float E2_SLOPE = 0.2f;

__device__ __forceinline__ float e2_lrelu(float v) { return v > 0.f ? v : E2_SLOPE * v; }
// the accumulator layout of the 32x32 MFMAs: lane (r = lane & 31, h = lane >> 5) holds column r, register e row:
__device__ __forceinline__ int e2_arow(int e, int h) { return (e & 3) + 8 * (e >> 2) + 4 * h; }

// grid ceil(R / ppb), block 256; R = b n points, ppb = 128 / k points per block.
__global__ __launch_bounds__(256) void edge2_eval_kernel(int R, int n, int k, int ppb, const float* __restrict__ pq,
                                                         const int* __restrict__ idx, const float* __restrict__ s1,
                                                         const float* __restrict__ t1, const float* __restrict__ W2,
                                                         const float* __restrict__ s2, const float* __restrict__ t2,
                                                         float* __restrict__ out, float* __restrict__ out2, int ld2) {
  __shared__ float Hs[E2_ROWS * E2_LD];
  __shared__ int Is[E2_ROWS];              // the rows' source rows of pq (b * n + idx); -1: a padding row
  const int pt0 = blockIdx.x * ppb;
  const int pts = min(ppb, R - pt0);       // points of this block (>= 1)
  const int rows = pts * k;                // valid edge rows (<= 128)
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;

  if (threadIdx.x < E2_ROWS) {
    int src = -1;
    if ((int)threadIdx.x < rows) {
      const int g = pt0 + threadIdx.x / k;                   // the point (< R)
      int j = idx[(size_t)g * k + threadIdx.x % k];
      j = j < 0 ? 0 : (j >= n ? n - 1 : j);                  // (an index outside the cloud is not followed)
      src = (g / n) * n + j;
    }
    Is[threadIdx.x] = src;
  }
  __syncthreads();

  {   // layer 1: h = lrelu(s1 (p[src] + q[g]) + t1), four channels per item; padding rows are zero
    constexpr int Q = E2_C / 4;
    for (int i = threadIdx.x; i < E2_ROWS * Q; i += 256) {
      const int row = i / Q, c = (i % Q) * 4;
      const int src = Is[row];
      float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
      if (src >= 0) {
        const int g = pt0 + row / k;
        const float4 p = *reinterpret_cast<const float4*>(pq + (size_t)src * (2 * E2_C) + c);
        const float4 q = *reinterpret_cast<const float4*>(pq + (size_t)g * (2 * E2_C) + E2_C + c);
        const float4 sc = *reinterpret_cast<const float4*>(s1 + c), sh = *reinterpret_cast<const float4*>(t1 + c);
        o.x = e2_lrelu((p.x + q.x) * sc.x + sh.x), o.y = e2_lrelu((p.y + q.y) * sc.y + sh.y);
        o.z = e2_lrelu((p.z + q.z) * sc.z + sh.z), o.w = e2_lrelu((p.w + q.w) * sc.w + sh.w);
      }
      *reinterpret_cast<float4*>(Hs + row * E2_LD + c) = o;
    }
  }
  __syncthreads();

  {   // layer 2 on this wave's row tile, both column tiles; its activation replaces h in the wave's own rows
    f32x16 acc[2];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[j][e] = 0.f;
    if (w * 32 < rows) {                                     // (wave-uniform: a tile of padding rows alone is skipped)
#pragma unroll 2
      for (int s = 0; s < E2_C / 8; ++s) {
        const float4 a = *reinterpret_cast<const float4*>(Hs + (w * 32 + r) * E2_LD + s * 8 + 4 * h);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const float4 bw = *reinterpret_cast<const float4*>(W2 + (size_t)(j * 32 + r) * E2_C + s * 8 + 4 * h);
          acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, bw.x, acc[j], 0, 0, 0);
          acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, bw.y, acc[j], 0, 0, 0);
          acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, bw.z, acc[j], 0, 0, 0);
          acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, bw.w, acc[j], 0, 0, 0);
        }
      }
    }
    __syncthreads();                                         // every read of h is done
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int c = j * 32 + r;
      const float sc = s2[c], sh = t2[c];
#pragma unroll
      for (int e = 0; e < 16; ++e) Hs[(w * 32 + e2_arow(e, h)) * E2_LD + c] = e2_lrelu(acc[j][e] * sc + sh);
    }
  }
  __syncthreads();

  // the max over each point's k rows, from its first edge, j ascending
  for (int i = threadIdx.x; i < pts * E2_C; i += 256) {
    const int pl = i / E2_C, c = i % E2_C;
    const float* col = Hs + (pl * k) * E2_LD + c;
    float m = col[0];
    for (int j = 1; j < k; ++j) m = fmaxf(m, col[j * E2_LD]);
    const size_t g = (size_t)(pt0 + pl);
    out[g * E2_C + c] = m;
    if (out2) out2[g * ld2 + c] = m;
  }
}

}  // namespace
}  // namespace pdae

using namespace pdae;

extern "C" int pdae_edge2_eval_supported(int k, int C1, int C2) {
  return k >= 1 && k <= E2_MAXK && C1 == E2_C && C2 == E2_C ? 1 : 0;
}

extern "C" int pdae_edge2_eval_forward(int b, int n, int k, int C1, int C2, const float* pq, const int32_t* idx,
                                       const float* scale1, const float* shift1, const float* W2, const float* scale2,
                                       const float* shift2, float* out, float* out2, int ld2, pdae_stream_t stream) {
  if (b < 0 || n <= 0 || k <= 0 || C1 <= 0 || C2 <= 0) return bad_arg("edge2_eval: bad size");
  if (!pdae_edge2_eval_supported(k, C1, C2))
    return unsupported("edge2_eval: 1 to 32 neighbours and layer widths (64, 64) required");
  const long long R = (long long)b * n;
  if (R * k >= (1LL << 31)) return unsupported("edge2_eval: too many edges");
  if (b == 0) return PDAE_OK;
  if (!pq || !idx || !scale1 || !shift1 || !W2 || !scale2 || !shift2 || !out) return bad_arg("edge2_eval: null pointer");
  if (out2 && ld2 < C2) return bad_arg("edge2_eval: ld2 is the row stride of out2, at least C2");
  if (((uintptr_t)pq | (uintptr_t)scale1 | (uintptr_t)shift1 | (uintptr_t)W2) & 15)
    return bad_arg("edge2_eval: pq, scale1, shift1 and W2 must be 16-byte aligned");
  const int ppb = E2_ROWS / k;
  const dim3 grid((unsigned)((R + ppb - 1) / ppb));
  hipLaunchKernelGGL(edge2_eval_kernel, grid, dim3(256), 0, as_stream(stream), (int)R, n, k, ppb, pq, idx, scale1, shift1,
                     W2, scale2, shift2, out, out2, ld2);
  return check_launch("edge2_eval_forward");
}
