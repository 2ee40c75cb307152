// sa_eval.hip -- one PointNet++ set-abstraction level in evaluation mode as ONE forward-only kernel.
//
// Reference: extensions/pointnet2/pointnet2_modules.py:31-72,124-158 (PointnetSAModule: QueryAndGroup, a SharedMLP of three
// Conv2d 1x1 (no bias) -> BatchNorm2d -> ReLU layers, F.max_pool2d over nsample), with every BatchNorm on its running
// estimates: scale_l = gamma / sqrt(var + eps), shift_l = beta - mean * scale_l.
//
//   out[b, p, :] = max_s relu(s2 (W2 relu(s1 (W1 relu(s0 (P[idx[b,p,s]] + W0x (xyz[idx[b,p,s]] - new_xyz[b,p])) + t0)) + t1)) + t2)
//
// P = features W0f^T is the feature half of the first layer, computed once per SOURCE point by the caller (a row GEMM);
// the coordinate half stays per (centre, sample): three FMAs on the centred difference, which is not split into
// W0x xyz - W0x centre (that would cancel against the ball radius).
//
// A block of four waves owns 64 consecutive rows (centre, sample): two centres of 32 samples or one of 64.  It gathers
// the rows' P entries and coordinates and forms layer 0's activation in LDS (64 x C1, rows padded by 4 floats:
// conflict-free ds_read_b128).  Layers 1 and 2 are fp32-input v_mfma_f32_32x32x2_f32 tiles, A from LDS, B straight from
// the weight in global memory (W1 and W2 are at most 192 KB together: they stay in L2 across blocks; LDS holds the ONE
// activation buffer, 33 KB at 128 channels, so four blocks share a CU).  Layer 1's output tiles wait in the accumulators
// until every wave has finished reading layer 0's activation, then replace it in the same buffer.  Layer 2's output never
// reaches LDS: in the accumulator layout a lane owns a channel and its registers the rows, so affine + ReLU + the max over
// a centre's rows is 16 register maxima and one cross-half shuffle, in a fixed order.  Only (B np, C3) is written; no
// atomics.
#include "common.h"

namespace pdae {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int SE_ROWS = 64;      // rows (centre, sample) per block

__device__ __forceinline__ int se_arow(int e, int h) { return (e & 3) + 8 * (e >> 2) + 4 * h; }

// How the four waves share a layer's (2 row tiles) x (N / 32 column tiles): with four or more column tiles a wave takes
// column tiles w, w + 4, .. and both row tiles (the weight operand is loaded once for both); with two, one tile each.
template <int N>
struct SeSplit {
  static constexpr int NT = N / 32;
  static constexpr int RT = NT >= 4 ? 2 : 1;           // row tiles per wave
  static constexpr int CPW = NT >= 4 ? NT / 4 : 1;     // column tiles per wave
  static_assert(NT == 2 || NT == 4 || NT == 8, "sa_eval: 64, 128 or 256 output channels");
  __device__ static int col_tile(int w, int j) { return NT >= 4 ? w + 4 * j : w % NT; }
  __device__ static int row_tile(int w, int t) { return NT >= 4 ? t : w / NT; }
};

// acc[j][t] = Hs (64, K; leading dimension K + 4) . W (N, K)^T on this wave's tiles
template <int K, int N>
__device__ __forceinline__ void se_layer(const float* Hs, const float* __restrict__ W, int w, int r, int h,
                                         f32x16 (&acc)[SeSplit<N>::CPW][SeSplit<N>::RT]) {
  using S = SeSplit<N>;
  constexpr int LD = K + 4;
#pragma unroll
  for (int j = 0; j < S::CPW; ++j)
#pragma unroll
    for (int t = 0; t < S::RT; ++t)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[j][t][e] = 0.f;
#pragma unroll 2
  for (int s = 0; s < K / 8; ++s) {
    float4 a[S::RT];
#pragma unroll
    for (int t = 0; t < S::RT; ++t)
      a[t] = *reinterpret_cast<const float4*>(Hs + (S::row_tile(w, t) * 32 + r) * LD + s * 8 + 4 * h);
#pragma unroll
    for (int j = 0; j < S::CPW; ++j) {
      const float4 bw = *reinterpret_cast<const float4*>(W + (size_t)(S::col_tile(w, j) * 32 + r) * K + s * 8 + 4 * h);
#pragma unroll
      for (int t = 0; t < S::RT; ++t) {
        acc[j][t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[t].x, bw.x, acc[j][t], 0, 0, 0);
        acc[j][t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[t].y, bw.y, acc[j][t], 0, 0, 0);
        acc[j][t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[t].z, bw.z, acc[j][t], 0, 0, 0);
        acc[j][t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[t].w, bw.w, acc[j][t], 0, 0, 0);
      }
    }
  }
}

// grid ceil(R / 64), block 256; R = B * np * ns rows, ns 32 or 64.
template <int C1, int C2, int C3>
__global__ __launch_bounds__(256) void sa_eval_kernel(int R, int N, int np, int ns, const float* __restrict__ xyz,
                                                      const float* __restrict__ new_xyz, const int* __restrict__ idx,
                                                      const float* __restrict__ P, const float* __restrict__ W0x,
                                                      const float* __restrict__ s0, const float* __restrict__ t0,
                                                      const float* __restrict__ W1, const float* __restrict__ s1,
                                                      const float* __restrict__ t1, const float* __restrict__ W2,
                                                      const float* __restrict__ s2, const float* __restrict__ t2,
                                                      float* __restrict__ out) {
  constexpr int CM = C1 > C2 ? C1 : C2;
  static_assert(SeSplit<C3>::RT == 2, "sa_eval: the last layer keeps a centre's two row tiles in one wave");
  __shared__ float Hs[SE_ROWS * (CM + 4)];
  __shared__ float Ds[SE_ROWS * 4];        // the rows' centred coordinates
  __shared__ int Is[SE_ROWS];              // the rows' source rows of P (b * N + idx)
  const int row0 = blockIdx.x * SE_ROWS;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;

  if (threadIdx.x < SE_ROWS) {
    const int row = row0 + threadIdx.x;
    float dx = 0.f, dy = 0.f, dz = 0.f;
    int src = 0;
    if (row < R) {
      const int g = row / ns, b = g / np;                    // centre (b, p) = g
      int j = idx[row];
      j = j < 0 ? 0 : (j >= N ? N - 1 : j);                  // (an index outside the cloud is not followed)
      src = b * N + j;
      dx = xyz[(size_t)src * 3] - new_xyz[(size_t)g * 3];
      dy = xyz[(size_t)src * 3 + 1] - new_xyz[(size_t)g * 3 + 1];
      dz = xyz[(size_t)src * 3 + 2] - new_xyz[(size_t)g * 3 + 2];
    }
    Ds[threadIdx.x * 4] = dx, Ds[threadIdx.x * 4 + 1] = dy, Ds[threadIdx.x * 4 + 2] = dz;
    Is[threadIdx.x] = src;
  }
  __syncthreads();

  {   // layer 0: relu(s0 (P[src] + W0x d) + t0), four channels per item
    constexpr int LD = C1 + 4, Q = C1 / 4;
    for (int i = threadIdx.x; i < SE_ROWS * Q; i += 256) {
      const int row = i / Q, c = (i % Q) * 4;
      const float dx = Ds[row * 4], dy = Ds[row * 4 + 1], dz = Ds[row * 4 + 2];
      float p[4] = {0.f, 0.f, 0.f, 0.f};
      if (P) {
        const float4 v = *reinterpret_cast<const float4*>(P + (size_t)Is[row] * C1 + c);
        p[0] = v.x, p[1] = v.y, p[2] = v.z, p[3] = v.w;
      }
      const float4 sc = *reinterpret_cast<const float4*>(s0 + c), sh = *reinterpret_cast<const float4*>(t0 + c);
      const float scv[4] = {sc.x, sc.y, sc.z, sc.w}, shv[4] = {sh.x, sh.y, sh.z, sh.w};
      float o[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float* wx = W0x + (size_t)(c + q) * 3;
        const float y = __builtin_fmaf(wx[2], dz, __builtin_fmaf(wx[1], dy, __builtin_fmaf(wx[0], dx, p[q])));
        o[q] = fmaxf(y * scv[q] + shv[q], 0.f);
      }
      *reinterpret_cast<float4*>(Hs + row * LD + c) = make_float4(o[0], o[1], o[2], o[3]);
    }
  }
  __syncthreads();

  {   // layer 1 -> the same buffer
    using S = SeSplit<C2>;
    constexpr int LD = C2 + 4;
    f32x16 acc[S::CPW][S::RT];
    se_layer<C1, C2>(Hs, W1, w, r, h, acc);
    __syncthreads();                         // every wave has read layer 0's activation
#pragma unroll
    for (int j = 0; j < S::CPW; ++j) {
      const int c = S::col_tile(w, j) * 32 + r;
      const float sc = s1[c], sh = t1[c];
#pragma unroll
      for (int t = 0; t < S::RT; ++t)
#pragma unroll
        for (int e = 0; e < 16; ++e)
          Hs[(S::row_tile(w, t) * 32 + se_arow(e, h)) * LD + c] = fmaxf(acc[j][t][e] * sc + sh, 0.f);
    }
  }
  __syncthreads();

  {   // layer 2, affine + ReLU, max over each centre's rows in the accumulators
    using S = SeSplit<C3>;
    f32x16 acc[S::CPW][2];
    se_layer<C2, C3>(Hs, W2, w, r, h, acc);
#pragma unroll
    for (int j = 0; j < S::CPW; ++j) {
      const int c = S::col_tile(w, j) * 32 + r;
      const float sc = s2[c], sh = t2[c];
      float m[2];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        float v = fmaxf(acc[j][t][0] * sc + sh, 0.f);
#pragma unroll
        for (int e = 1; e < 16; ++e) v = fmaxf(v, fmaxf(acc[j][t][e] * sc + sh, 0.f));
        m[t] = fmaxf(v, __shfl_xor(v, 32, kWave));
      }
      if (h == 0) {
        if (ns == 64) {
          if (row0 < R) out[(size_t)(row0 / 64) * C3 + c] = fmaxf(m[0], m[1]);
        } else {
#pragma unroll
          for (int t = 0; t < 2; ++t)
            if (row0 + t * 32 < R) out[(size_t)(row0 / 32 + t) * C3 + c] = m[t];
        }
      }
    }
  }
}

bool se_widths(int C1, int C2, int C3) {
  return (C1 == 64 && C2 == 64 && C3 == 128) || (C1 == 128 && C2 == 128 && C3 == 256);
}

}  // namespace
}  // namespace pdae

using namespace pdae;

extern "C" int pdae_sa_eval_supported(int ns, int C0, int C1, int C2, int C3) {
  return (ns == 32 || ns == 64) && C0 >= 0 && se_widths(C1, C2, C3) ? 1 : 0;
}

extern "C" int pdae_sa_eval_forward(int B, int N, int np, int ns, int C0, int C1, int C2, int C3, const float* xyz,
                                    const float* new_xyz, const int32_t* idx, const float* P, const float* W0x,
                                    const float* scale0, const float* shift0, const float* W1, const float* scale1,
                                    const float* shift1, const float* W2, const float* scale2, const float* shift2,
                                    float* out, pdae_stream_t stream) {
  if (B < 0 || N <= 0 || np <= 0 || ns <= 0 || C0 < 0 || C1 <= 0 || C2 <= 0 || C3 <= 0) return bad_arg("sa_eval: bad size");
  if (!pdae_sa_eval_supported(ns, C0, C1, C2, C3))
    return unsupported("sa_eval: nsample 32 or 64 and layer widths (64, 64, 128) or (128, 128, 256) required");
  const long long R = (long long)B * np * ns;
  if (R >= (1LL << 31) || (long long)B * N >= (1LL << 31)) return unsupported("sa_eval: too many rows");
  if (B == 0) return PDAE_OK;
  if ((C0 > 0) != (P != nullptr)) return bad_arg("sa_eval: P goes with C0 > 0");
  if (!xyz || !new_xyz || !idx || !W0x || !scale0 || !shift0 || !W1 || !scale1 || !shift1 || !W2 || !scale2 || !shift2 || !out)
    return bad_arg("sa_eval: null pointer");
  const uintptr_t al = (uintptr_t)P | (uintptr_t)scale0 | (uintptr_t)shift0 | (uintptr_t)W1 | (uintptr_t)W2;
  if (al & 15) return bad_arg("sa_eval: P, scale0, shift0, W1 and W2 must be 16-byte aligned");
  const dim3 grid((unsigned)((R + SE_ROWS - 1) / SE_ROWS));
  hipStream_t s = as_stream(stream);
  if (C1 == 64)
    hipLaunchKernelGGL((sa_eval_kernel<64, 64, 128>), grid, dim3(256), 0, s, (int)R, N, np, ns, xyz, new_xyz, idx, P, W0x,
                       scale0, shift0, W1, scale1, shift1, W2, scale2, shift2, out);
  else
    hipLaunchKernelGGL((sa_eval_kernel<128, 128, 256>), grid, dim3(256), 0, s, (int)R, N, np, ns, xyz, new_xyz, idx, P, W0x,
                       scale0, shift0, W1, scale1, shift1, W2, scale2, shift2, out);
  return check_launch("sa_eval_forward");
}
