// resample.hip -- the fine-tuning runner's batch preparation behind FPS as ONE launch (runner_finetune.py:415-420 of the
// reference): the subset of the FPS order the host drew, the gather, and the per-cloud map of a train / test transform
// (datasets/data_transforms.py: PointcloudRotate, PointcloudScaleAndTranslate)
//   out[b][n][j] = sum_i raw[b][fps_idx[b][choice[n]]][i] * A[b][i][j] + t[b][j]          i, j in 0..2
// where the framework path was a slice copy, index_select, two transposing copies around gather_points and, for the
// transform, a host-to-device copy + matmul + strided write-back PER CLOUD.  Memory-trivial: one thread per output point,
// the 12 map floats of the block's cloud staged in LDS.
#include "common.h"

namespace pdae {

// has_a / has_t are launch-uniform.  Neither: the coordinates are moved, not computed on (bit for bit, signed zeros
// included).  With a map: ((x A0j + y A1j) + z A2j) + tj, each operation rounded (-ffp-contract=off).
// An index outside its array (a corrupt choice / fps_idx) is not followed: that point comes out as NaN.
__global__ __launch_bounds__(256) void resample_affine_kernel(int P, int C, int point_all, int npoints, int chunks,
                                                              const float* __restrict__ raw, const int32_t* __restrict__ fps_idx,
                                                              const int32_t* __restrict__ choice, const float* __restrict__ A,
                                                              const float* __restrict__ t, float* __restrict__ out) {
  __shared__ float m[12];
  const int b = blockIdx.x / chunks;                       // block-uniform: one cloud per block
  const int n = (blockIdx.x - b * chunks) * 256 + threadIdx.x;
  if (threadIdx.x < 9) m[threadIdx.x] = A ? A[(size_t)b * 9 + threadIdx.x] : 0.f;
  else if (threadIdx.x < 12) m[threadIdx.x] = t ? t[(size_t)b * 3 + (threadIdx.x - 9)] : 0.f;
  __syncthreads();
  if (n >= npoints) return;
  const int c = choice[n];
  float x = __builtin_nanf(""), y = x, z = x;
  bool ok = (unsigned)c < (unsigned)point_all;
  if (ok) {
    const int i = fps_idx[(size_t)b * point_all + c];
    ok = (unsigned)i < (unsigned)P;
    if (ok) {
      const float* src = raw + ((size_t)b * P + i) * C;
      x = src[0], y = src[1], z = src[2];
    }
  }
  float* dst = out + ((size_t)b * npoints + n) * 3;
  if (ok && A) {
    const float u = x * m[0] + y * m[3] + z * m[6];
    const float v = x * m[1] + y * m[4] + z * m[7];
    const float w = x * m[2] + y * m[5] + z * m[8];
    x = u, y = v, z = w;
  }
  if (ok && t) x += m[9], y += m[10], z += m[11];
  dst[0] = x, dst[1] = y, dst[2] = z;
}

}  // namespace pdae

using namespace pdae;

extern "C" int pdae_resample_affine(int b, int p, int c, int point_all, int npoints, const float* raw, const int32_t* fps_idx,
                                    const int32_t* choice, const float* A, const float* t, float* out, pdae_stream_t stream) {
  if (b <= 0 || p <= 0 || c <= 0 || point_all <= 0 || npoints <= 0) return bad_arg("resample_affine: sizes must be positive");
  if (c < 3) return bad_arg("resample_affine: c >= 3 (the first three channels are the coordinates)");
  if (npoints > point_all) return bad_arg("resample_affine: npoints > point_all");
  if (!raw || !fps_idx || !choice || !out) return bad_arg("resample_affine: null pointer");
  const int chunks = (npoints + 255) / 256;
  if ((long long)b * chunks > 0x7fffffffLL) return unsupported("resample_affine: too many points for one launch");
  hipLaunchKernelGGL(resample_affine_kernel, dim3((unsigned)(b * chunks)), dim3(256), 0, as_stream(stream), p, c, point_all,
                     npoints, chunks, raw, fps_idx, choice, A, t, out);
  return check_launch("resample_affine");
}
