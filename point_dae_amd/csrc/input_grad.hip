// input_grad.hip -- the two data-only backward steps that end at point coordinates (include/pdae.h, "Input-point
// gradients"): Group.forward's backward (kNN gather + centre subtraction) and the 3-input Linear's data gradient.
//
//   group_points_backward  one thread owns a point of a cloud and scans the cloud's G*k neighbour indices, staged
//                          through LDS in chunks and read four at a time (every lane reads the same address: a
//                          broadcast); a match adds that entry's gradient.  Then the G centre indices the same way.
//                          The order of a point's additions is fixed by the scan: no atomics, same bits every run.
//   rows_contract3         (M, C) x (C, 3): 32 lanes share a row, float4 loads, the weight transposed in LDS.
#include "common.h"

namespace pdae {

constexpr int GPB_THREADS = 256;
constexpr int GPB_CHUNK = 4096;     // indices staged per pass (16 KB of LDS)

__global__ __launch_bounds__(GPB_THREADS) void group_points_backward_kernel(
    int N, int G, int k, const float* __restrict__ d_nbr, const float* __restrict__ d_center,
    const long long* __restrict__ knn_idx, const int* __restrict__ fps_idx, float* __restrict__ d_xyz) {
  __shared__ int4 s_idx4[GPB_CHUNK / 4];
  int* s_idx = reinterpret_cast<int*>(s_idx4);
  const int b = blockIdx.y;
  const int n = blockIdx.x * GPB_THREADS + threadIdx.x;       // (n >= N: the thread only helps staging)
  const int E = G * k;
  const long long* idx = knn_idx + (size_t)b * E;
  const float* dn = d_nbr + (size_t)b * E * 3;
  float ax = 0.f, ay = 0.f, az = 0.f;
  // ---- neighbour terms, ascending (g, j)
  for (int e0 = 0; e0 < E; e0 += GPB_CHUNK) {
    const int cnt = min(GPB_CHUNK, E - e0);
    const int cnt4 = (cnt + 3) & ~3;
    __syncthreads();
    for (int i = threadIdx.x; i < cnt4; i += GPB_THREADS) {
      int v = -1;                                              // (the padding and any index outside the cloud: no point)
      if (i < cnt) {
        const long long t = idx[e0 + i];
        if (t >= 0 && t < N) v = (int)t;
      }
      s_idx[i] = v;
    }
    __syncthreads();
    if (n < N) {
      for (int i = 0; i < cnt4; i += 4) {
        const int4 q = s_idx4[i >> 2];
        if (q.x == n) { const float* p = dn + (size_t)(e0 + i) * 3;     ax += p[0], ay += p[1], az += p[2]; }
        if (q.y == n) { const float* p = dn + (size_t)(e0 + i + 1) * 3; ax += p[0], ay += p[1], az += p[2]; }
        if (q.z == n) { const float* p = dn + (size_t)(e0 + i + 2) * 3; ax += p[0], ay += p[1], az += p[2]; }
        if (q.w == n) { const float* p = dn + (size_t)(e0 + i + 3) * 3; ax += p[0], ay += p[1], az += p[2]; }
      }
    }
  }
  // ---- centre terms, ascending g: d_center[g] - (the group's d_nbr, ascending j)
  const int* fidx = fps_idx + (size_t)b * G;
  for (int g0 = 0; g0 < G; g0 += GPB_CHUNK) {
    const int cnt = min(GPB_CHUNK, G - g0);
    __syncthreads();
    for (int i = threadIdx.x; i < cnt; i += GPB_THREADS) {
      const int t = fidx[g0 + i];
      s_idx[i] = (t >= 0 && t < N) ? t : -1;
    }
    __syncthreads();
    if (n < N) {
      for (int i = 0; i < cnt; ++i) {
        if (s_idx[i] != n) continue;
        const int g = g0 + i;
        const float* p = dn + (size_t)g * k * 3;
        float sx = 0.f, sy = 0.f, sz = 0.f;
        for (int j = 0; j < k; ++j) sx += p[3 * j], sy += p[3 * j + 1], sz += p[3 * j + 2];
        float cx = 0.f, cy = 0.f, cz = 0.f;
        if (d_center) {
          const float* c = d_center + ((size_t)b * G + g) * 3;
          cx = c[0], cy = c[1], cz = c[2];
        }
        ax += cx - sx, ay += cy - sy, az += cz - sz;
      }
    }
  }
  if (n < N) {
    float* o = d_xyz + ((size_t)b * N + n) * 3;
    o[0] = ax, o[1] = ay, o[2] = az;
  }
}

constexpr int RC3_MAX_C = 1024;
constexpr int RC3_ROWS = 8;         // rows per block pass: 32 lanes each

__global__ __launch_bounds__(256) void rows_contract3_kernel(int M, int C, const float* __restrict__ d,
                                                             const float* __restrict__ w,
                                                             const long long* __restrict__ row_ids, int n_out,
                                                             float* __restrict__ dx) {
  __shared__ float sw[3 * RC3_MAX_C];                          // [j][c]
  for (int i = threadIdx.x; i < 3 * C; i += 256) {
    const int c = i / 3, j = i - 3 * c;
    sw[j * C + c] = w[i];
  }
  __syncthreads();
  const int sub = threadIdx.x & 31, rloc = threadIdx.x >> 5;
  const int passes = (M + gridDim.x * RC3_ROWS - 1) / (gridDim.x * RC3_ROWS);     // (the same trip count for every lane)
  for (int it = 0; it < passes; ++it) {
    const long long m = ((long long)it * gridDim.x + blockIdx.x) * RC3_ROWS + rloc;
    const bool live = m < M;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
    if (live) {
      const float* row = d + (size_t)m * C;
      for (int c = sub * 4; c < C; c += 128) {
        const float4 v = *reinterpret_cast<const float4*>(row + c);
        a0 += v.x * sw[c], a1 += v.x * sw[C + c], a2 += v.x * sw[2 * C + c];
        a0 += v.y * sw[c + 1], a1 += v.y * sw[C + c + 1], a2 += v.y * sw[2 * C + c + 1];
        a0 += v.z * sw[c + 2], a1 += v.z * sw[C + c + 2], a2 += v.z * sw[2 * C + c + 2];
        a0 += v.w * sw[c + 3], a1 += v.w * sw[C + c + 3], a2 += v.w * sw[2 * C + c + 3];
      }
    }
#pragma unroll
    for (int o = 16; o >= 1; o >>= 1) {                        // (offsets below 32: the two rows of a wave stay apart)
      a0 += __shfl_xor(a0, o, kWave);
      a1 += __shfl_xor(a1, o, kWave);
      a2 += __shfl_xor(a2, o, kWave);
    }
    if (live && sub == 0) {
      const long long r = row_ids ? row_ids[m] : m;
      if (r >= 0 && r < n_out) {
        float* o = dx + (size_t)r * 3;
        o[0] = a0, o[1] = a1, o[2] = a2;
      }
    }
  }
}

}  // namespace pdae

using namespace pdae;

extern "C" int pdae_group_points_backward(int b, int n, int g, int k, const float* d_nbr, const float* d_center,
                                          const int64_t* knn_idx, const int32_t* fps_idx, float* d_xyz,
                                          pdae_stream_t stream) {
  if (b < 0 || n < 0 || g <= 0 || k <= 0) return bad_arg("group_points_backward: bad size");
  if ((long long)g * k > (1ll << 30)) return bad_arg("group_points_backward: g * k too large");
  if (b == 0 || n == 0) return PDAE_OK;
  if (!d_nbr || !knn_idx || !fps_idx || !d_xyz) return bad_arg("group_points_backward: null pointer");
  if (b > 65535) return unsupported("group_points_backward: more than 65535 clouds in one launch");
  hipLaunchKernelGGL(group_points_backward_kernel, dim3((n + GPB_THREADS - 1) / GPB_THREADS, b), dim3(GPB_THREADS), 0,
                     as_stream(stream), n, g, k, d_nbr, d_center, reinterpret_cast<const long long*>(knn_idx), fps_idx,
                     d_xyz);
  return check_launch("group_points_backward");
}

extern "C" int pdae_rows_contract3(int m, int c, const float* d, const float* w, const int64_t* row_ids, int n_out,
                                   float* dx, pdae_stream_t stream) {
  if (m < 0 || n_out < 0 || c <= 0 || c % 4 != 0 || c > RC3_MAX_C)
    return bad_arg("rows_contract3: c must be a positive multiple of 4, at most 1024");
  if (!row_ids && n_out != m) return bad_arg("rows_contract3: without row_ids n_out must equal m");
  if (m == 0) return PDAE_OK;
  if (!d || !w || !dx) return bad_arg("rows_contract3: null pointer");
  int blocks = (m + RC3_ROWS - 1) / RC3_ROWS;
  if (blocks > 2048) blocks = 2048;                            // (grid-stride: the weight is staged once per block)
  hipLaunchKernelGGL(rows_contract3_kernel, dim3(blocks), dim3(256), 0, as_stream(stream), m, c, d, w,
                     reinterpret_cast<const long long*>(row_ids), n_out, dx);
  return check_launch("rows_contract3");
}
