// sa_train.hip -- the first layer of a PointNet++ set-abstraction level in TRAINING mode, split by source point.
//
// Reference: extensions/pointnet2/pointnet2_modules.py:31-72,124-158 (PointnetSAModule: QueryAndGroup, then a SharedMLP of
// Conv2d 1x1 (no bias) -> BatchNorm2d -> ReLU layers).  The grouped form (sa_mlp.SharedMLPMaxFunction) materialises the
// rows [xyz - centre | 0 | features] and runs the first layer's whole product per (centre, sample) row.  The feature half
// of that product is linear in the SOURCE point, so, as csrc/sa_eval.hip does in evaluation mode,
//
//   y0[row, :] = P[b N + idx[row], :] + W0x (xyz[b, idx[row]] - new_xyz[centre(row)])        P = features W0f^T
//
// with P computed once per source point by the caller (a row GEMM on B N rows instead of B np ns).  The coordinate half
// stays per row: three FMAs on the centred difference, formed BEFORE the product (W0x xyz - W0x centre would cancel
// against the ball radius).  The same identity serves the backward:
//
//   dP[b N + j, :] = sum of dy0[row, :] over the rows whose source is j, in ascending row order
//   dW0x[c, k]     = sum over the rows of dy0[row, c] * d[row, k]
//
// after which dW0f = dP^T features and dfeatures = dP W0f are products on B N rows (the caller's row GEMMs).
//
// Every reduction has a fixed order: block partials are plain stores, added by sa_ordered_sum_kernel in block order.  No
// atomics on floats anywhere; the integer atomics of the per-cloud counting sort only place rows, and a stable ranking
// pass behind them makes the order of a point's rows ascending whatever the order of arrival was.
#include "common.h"

namespace pdae {
namespace {

constexpr int ST_ROWS = 64;          // forward: rows (centre, sample) per tile
constexpr int ST_MAX_BLOCKS = 1024;  // forward: blocks (= statistics partials) at the most
constexpr int ST_WROWS = 1024;       // dW0x: rows per block
constexpr int ST_SLOTS = 8;          // partial sets handed to bn_finalize (pdae_conv_stats leaves eight as well)
constexpr int ST_SPLIT = 4;          // dP: blocks per cloud

__device__ __forceinline__ int st_clamp(int j, int N) { return j < 0 ? 0 : (j >= N ? N - 1 : j); }

// The centred difference of a row and its source row of P (b N + j).
__device__ __forceinline__ size_t st_row(int row, int N, int np, int ns, const float* __restrict__ xyz,
                                         const float* __restrict__ new_xyz, const int* __restrict__ idx, float& dx,
                                         float& dy, float& dz) {
  const int g = row / ns, b = g / np;                        // centre (b, p) = g
  const size_t src = (size_t)b * N + st_clamp(idx[row], N);  // (an index outside the cloud is not followed)
  dx = xyz[src * 3] - new_xyz[(size_t)g * 3];
  dy = xyz[src * 3 + 1] - new_xyz[(size_t)g * 3 + 1];
  dz = xyz[src * 3 + 2] - new_xyz[(size_t)g * 3 + 2];
  return src;
}

// grid min(tiles, ST_MAX_BLOCKS), block 256.  A thread owns one channel quad (C1 / 4 of them side by side, 256 / (C1 / 4)
// rows in flight) for the whole launch, so the quad's W0x rows and its column sums stay in registers; the row phases meet
// in LDS in phase order and every block stores ONE partial [2][C1].
__global__ __launch_bounds__(256) void sa_first_forward_kernel(int R, int tiles, int N, int np, int ns, int C1,
                                                               const float* __restrict__ xyz,
                                                               const float* __restrict__ new_xyz,
                                                               const int* __restrict__ idx, const float* __restrict__ P,
                                                               const float* __restrict__ W0x, float* __restrict__ y0,
                                                               float* __restrict__ part) {
  __shared__ float red[256 * 8];
  const int Q = C1 / 4, PH = 256 / Q;
  const int q = threadIdx.x % Q, ph = threadIdx.x / Q, c = 4 * q;
  float wx[4][3];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int k = 0; k < 3; ++k) wx[i][k] = W0x[(c + i) * 3 + k];
  float s[4] = {0.f, 0.f, 0.f, 0.f}, ss[4] = {0.f, 0.f, 0.f, 0.f};
  for (int t = blockIdx.x; t < tiles; t += gridDim.x) {
    for (int rr = ph; rr < ST_ROWS; rr += PH) {
      const int row = t * ST_ROWS + rr;
      if (row >= R) break;
      float dx, dy, dz;
      const size_t src = st_row(row, N, np, ns, xyz, new_xyz, idx, dx, dy, dz);
      float p[4] = {0.f, 0.f, 0.f, 0.f};
      if (P) {
        const float4 v = *reinterpret_cast<const float4*>(P + src * C1 + c);
        p[0] = v.x, p[1] = v.y, p[2] = v.z, p[3] = v.w;
      }
      float y[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        y[i] = __builtin_fmaf(wx[i][2], dz, __builtin_fmaf(wx[i][1], dy, __builtin_fmaf(wx[i][0], dx, p[i])));
        s[i] += y[i];
        ss[i] += y[i] * y[i];
      }
      *reinterpret_cast<float4*>(y0 + (size_t)row * C1 + c) = make_float4(y[0], y[1], y[2], y[3]);
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) red[threadIdx.x * 8 + i] = s[i], red[threadIdx.x * 8 + 4 + i] = ss[i];
  __syncthreads();
  if (ph == 0) {
    for (int o = 1; o < PH; ++o)
#pragma unroll
      for (int i = 0; i < 4; ++i) s[i] += red[(o * Q + q) * 8 + i], ss[i] += red[(o * Q + q) * 8 + 4 + i];
    float* dst = part + (size_t)blockIdx.x * 2 * C1;
    *reinterpret_cast<float4*>(dst + c) = make_float4(s[0], s[1], s[2], s[3]);
    *reinterpret_cast<float4*>(dst + C1 + c) = make_float4(ss[0], ss[1], ss[2], ss[3]);
  }
}

// part [P][width] -> FINAL: out[c] = the sum over p; else out[l][c] = the sum over the p = l (mod ST_SLOTS), l < ST_SLOTS.
// grid ceil(width / 32), block 32 columns x 8 lanes; a lane adds its partials in ascending order in fp64, FINAL adds the
// lanes in lane order: the same bits on every run.
template <bool FINAL>
__global__ __launch_bounds__(256) void sa_ordered_sum_kernel(int P, int width, const float* __restrict__ part,
                                                             float* __restrict__ out) {
  __shared__ double red[ST_SLOTS][32];
  const int cl = threadIdx.x & 31, l = threadIdx.x >> 5;
  const int c = blockIdx.x * 32 + cl;
  double t = 0.0;
  if (c < width) {
    int p = l;
    for (; p + 3 * ST_SLOTS < P; p += 4 * ST_SLOTS) {
      float v[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] = part[(size_t)(p + k * ST_SLOTS) * width + c];
#pragma unroll
      for (int k = 0; k < 4; ++k) t += (double)v[k];
    }
    for (; p < P; p += ST_SLOTS) t += (double)part[(size_t)p * width + c];
  }
  if (!FINAL) {
    if (c < width) out[(size_t)l * width + c] = (float)t;
    return;
  }
  red[l][cl] = t;
  __syncthreads();
  if (l == 0 && c < width) {
#pragma unroll
    for (int k = 1; k < ST_SLOTS; ++k) t += red[k][cl];
    out[c] = (float)t;
  }
}

// dW0x: grid ceil(R / ST_WROWS), block 256; a thread owns a channel quad of a row phase and walks its rows, the phases
// meet in LDS in phase order, every block stores one partial [C1][3].
__global__ __launch_bounds__(256) void sa_first_wx_kernel(int R, int N, int np, int ns, int C1,
                                                          const float* __restrict__ xyz, const float* __restrict__ new_xyz,
                                                          const int* __restrict__ idx, const float* __restrict__ dy0,
                                                          float* __restrict__ part) {
  __shared__ float red[256 * 12];
  const int Q = C1 / 4, PH = 256 / Q;
  const int q = threadIdx.x % Q, ph = threadIdx.x / Q, c = 4 * q;
  float a[4][3];
#pragma unroll
  for (int i = 0; i < 4; ++i) a[i][0] = a[i][1] = a[i][2] = 0.f;
  const long long r0 = (long long)blockIdx.x * ST_WROWS;
  const int r1 = (int)(r0 + ST_WROWS < R ? r0 + ST_WROWS : R);
#pragma unroll 2
  for (int row = (int)r0 + ph; row < r1; row += PH) {
    float d[3];
    (void)st_row(row, N, np, ns, xyz, new_xyz, idx, d[0], d[1], d[2]);
    const float4 g4 = *reinterpret_cast<const float4*>(dy0 + (size_t)row * C1 + c);
    const float g[4] = {g4.x, g4.y, g4.z, g4.w};
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int k = 0; k < 3; ++k) a[i][k] += g[i] * d[k];
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int k = 0; k < 3; ++k) red[threadIdx.x * 12 + i * 3 + k] = a[i][k];
  __syncthreads();
  if (ph == 0) {
    for (int o = 1; o < PH; ++o)
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int k = 0; k < 3; ++k) a[i][k] += red[(o * Q + q) * 12 + i * 3 + k];
    float* dst = part + (size_t)blockIdx.x * 3 * C1 + 3 * c;      // [c .. c + 3][3]: twelve consecutive floats
    *reinterpret_cast<float4*>(dst) = make_float4(a[0][0], a[0][1], a[0][2], a[1][0]);
    *reinterpret_cast<float4*>(dst + 4) = make_float4(a[1][1], a[1][2], a[2][0], a[2][1]);
    *reinterpret_cast<float4*>(dst + 8) = make_float4(a[2][2], a[3][0], a[3][1], a[3][2]);
  }
}

// dP: the recipe of ball_group.hip's sa_group_rows_grad_kernel -- a cloud's rows ordered by source point with a counting
// sort in LDS, then every point's rows summed in registers by one sub-group reading whole rows of dy0 -- with one more
// pass: the sort places a point's rows in their order of arrival, so each row is then RANKED among its point's rows and
// moved to that place.  A point's sum is taken in ascending row order, the same bits on every run.  ST_SPLIT blocks per
// cloud share the (cheap) sort and take a range of points each.
__global__ __launch_bounds__(256) void sa_first_dp_kernel(int N, int rows, int C, const int32_t* __restrict__ idx,
                                                          const float* __restrict__ dy0, float* __restrict__ dP) {
  extern __shared__ int st_lds[];                // cnt[N] | off[N + 1] | list[rows] | sorted[rows]
  int* cnt = st_lds;
  int* off = st_lds + N;
  int* list = off + N + 1;
  int* sorted = list + rows;
  const int b = blockIdx.x / ST_SPLIT, part = blockIdx.x % ST_SPLIT;
  const int tid = threadIdx.x;
  const int32_t* ib = idx + (long long)b * rows;
  for (int i = tid; i < N; i += 256) cnt[i] = 0;
  __syncthreads();
  for (int r = tid; r < rows; r += 256) atomicAdd(&cnt[st_clamp(ib[r], N)], 1);
  __syncthreads();
  // exclusive prefix sum of cnt (N <= 4096): one wave, N / 64 entries per lane + a shuffle scan of the lane totals
  if (tid < 64) {
    const int per = (N + 63) / 64, j0 = tid * per;
    int sum = 0;
    for (int k = 0; k < per; ++k)
      if (j0 + k < N) sum += cnt[j0 + k];
    int incl = sum;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int t = __shfl_up(incl, d, 64);
      if (tid >= d) incl += t;
    }
    int run = incl - sum;
    for (int k = 0; k < per; ++k)
      if (j0 + k < N) {
        off[j0 + k] = run;
        run += cnt[j0 + k];
      }
    if (tid == 63) off[N] = incl;
  }
  __syncthreads();
  for (int i = tid; i < N; i += 256) cnt[i] = off[i];           // cnt becomes the scatter cursor
  __syncthreads();
  for (int r = tid; r < rows; r += 256) list[atomicAdd(&cnt[st_clamp(ib[r], N)], 1)] = r;
  __syncthreads();
  // stable order: a row's place among its point's rows is the number of them that come before it
  for (int k = tid; k < rows; k += 256) {
    const int r = list[k];
    const int j = st_clamp(ib[r], N);
    const int k0 = off[j], k1 = off[j + 1];
    int rank = 0;
    for (int k2 = k0; k2 < k1; ++k2) rank += list[k2] < r ? 1 : 0;
    sorted[k0 + rank] = r;
  }
  __syncthreads();
  // ---- sums: LPR lanes (one channel quad each) per point, SUBS points in flight
  const int LPR = C / 4, SUBS = 256 / LPR;
  const int lane = tid % LPR, sub = tid / LPR;
  const int jbeg = (int)((long long)N * part / ST_SPLIT), jend = (int)((long long)N * (part + 1) / ST_SPLIT);
  const float* base = dy0 + (long long)b * rows * C + 4 * lane;
  constexpr int UN = 8;
  for (int j = jbeg + sub; j < jend; j += SUBS) {
    const int k0 = off[j], k1 = off[j + 1];
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int k = k0; k < k1; k += UN) {
      float4 v[UN];
#pragma unroll
      for (int u = 0; u < UN; ++u) v[u] = *reinterpret_cast<const float4*>(base + (long long)sorted[min(k + u, k1 - 1)] * C);
#pragma unroll
      for (int u = 0; u < UN; ++u)
        if (k + u < k1) s.x += v[u].x, s.y += v[u].y, s.z += v[u].z, s.w += v[u].w;
    }
    *reinterpret_cast<float4*>(dP + ((long long)b * N + j) * C + 4 * lane) = s;
  }
}

size_t st_dp_lds(int N, long long rows) { return sizeof(int) * ((size_t)2 * N + 1 + 2 * (size_t)rows); }

int st_forward_blocks(long long R) {
  const long long tiles = (R + ST_ROWS - 1) / ST_ROWS;
  return (int)(tiles < ST_MAX_BLOCKS ? tiles : ST_MAX_BLOCKS);
}

}  // namespace
}  // namespace pdae

using namespace pdae;

extern "C" int pdae_sa_first_supported(int B, int N, int np, int ns, int C0, int C1) {
  if (B < 0 || N <= 0 || np <= 0 || (ns != 32 && ns != 64) || C0 < 0 || C1 <= 0) return 0;
  if (C0 % 4 != 0 || C1 % 4 != 0 || C1 > 1024 || 256 % (C1 / 4) != 0) return 0;
  if ((long long)B * np * ns >= (1LL << 31) || (long long)B * N >= (1LL << 31) / 4) return 0;
  if ((long long)B * ST_SPLIT > 0x7fffffffLL) return 0;
  // the backward's sort of a cloud lives in LDS (only a level with features has a dP to sort for)
  if (C0 > 0 && (N > 4096 || st_dp_lds(N, (long long)np * ns) > 150 * 1024)) return 0;
  return 1;
}

extern "C" long long pdae_sa_first_forward_workspace(long long R, int C1) {
  if (R <= 0 || C1 <= 0) return 0;
  return (long long)st_forward_blocks(R) * 2 * C1;
}

extern "C" long long pdae_sa_first_backward_workspace(long long R, int C1) {
  if (R <= 0 || C1 <= 0) return 0;
  return ((R + ST_WROWS - 1) / ST_WROWS) * 3 * C1;
}

extern "C" int pdae_sa_first_forward(int B, int N, int np, int ns, int C0, int C1, const float* xyz, const float* new_xyz,
                                     const int32_t* idx, const float* P, const float* W0x, float* y0, float* stats,
                                     float* workspace, pdae_stream_t stream) {
  if (!pdae_sa_first_supported(B, N, np, ns, C0, C1))
    return unsupported("sa_first: nsample 32 or 64, widths multiples of 4, C1 / 4 a divisor of 256, a cloud's sort within LDS");
  if (B == 0) return PDAE_OK;
  if ((C0 > 0) != (P != nullptr)) return bad_arg("sa_first_forward: P goes with C0 > 0");
  if (!xyz || !new_xyz || !idx || !W0x || !y0 || !stats || !workspace) return bad_arg("sa_first_forward: null pointer");
  if (((uintptr_t)P | (uintptr_t)y0 | (uintptr_t)workspace) & 15)
    return bad_arg("sa_first_forward: P, y0 and the workspace must be 16-byte aligned");
  const long long R = (long long)B * np * ns;
  const int tiles = (int)((R + ST_ROWS - 1) / ST_ROWS), blocks = st_forward_blocks(R);
  hipStream_t s = as_stream(stream);
  hipLaunchKernelGGL(sa_first_forward_kernel, dim3(blocks), dim3(256), 0, s, (int)R, tiles, N, np, ns, C1, xyz, new_xyz, idx,
                     P, W0x, y0, workspace);
  hipLaunchKernelGGL(sa_ordered_sum_kernel<false>, dim3((2 * C1 + 31) / 32), dim3(256), 0, s, blocks, 2 * C1, workspace,
                     stats);
  return check_launch("sa_first_forward");
}

extern "C" int pdae_sa_first_backward(int B, int N, int np, int ns, int C0, int C1, const float* xyz, const float* new_xyz,
                                      const int32_t* idx, const float* dy0, float* dP, float* dW0x, float* workspace,
                                      pdae_stream_t stream) {
  if (!pdae_sa_first_supported(B, N, np, ns, C0, C1))
    return unsupported("sa_first: nsample 32 or 64, widths multiples of 4, C1 / 4 a divisor of 256, a cloud's sort within LDS");
  if (!dW0x) return bad_arg("sa_first_backward: null pointer");
  hipStream_t s = as_stream(stream);
  if (B == 0) {
    (void)hipMemsetAsync(dW0x, 0, sizeof(float) * 3 * (size_t)C1, s);
    return check_launch("sa_first_backward");
  }
  if ((C0 > 0) != (dP != nullptr)) return bad_arg("sa_first_backward: dP goes with C0 > 0");
  if (!xyz || !new_xyz || !idx || !dy0 || !workspace) return bad_arg("sa_first_backward: null pointer");
  if (((uintptr_t)dP | (uintptr_t)dy0 | (uintptr_t)workspace) & 15)
    return bad_arg("sa_first_backward: dy0, dP and the workspace must be 16-byte aligned");
  const long long R = (long long)B * np * ns;
  const int blocks = (int)((R + ST_WROWS - 1) / ST_WROWS);
  hipLaunchKernelGGL(sa_first_wx_kernel, dim3(blocks), dim3(256), 0, s, (int)R, N, np, ns, C1, xyz, new_xyz, idx, dy0,
                     workspace);
  hipLaunchKernelGGL(sa_ordered_sum_kernel<true>, dim3((3 * C1 + 31) / 32), dim3(256), 0, s, blocks, 3 * C1, workspace, dW0x);
  if (dP) {
    const long long rows = (long long)np * ns;
    static bool once = false;
    if (!once) {
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(sa_first_dp_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                150 * 1024);
      once = true;
    }
    hipLaunchKernelGGL(sa_first_dp_kernel, dim3(B * ST_SPLIT), dim3(256), st_dp_lds(N, rows), s, N, (int)rows, C1, idx, dy0, dP);
  }
  return check_launch("sa_first_backward");
}
