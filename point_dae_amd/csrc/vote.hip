// vote.hip -- the voted evaluation of a fine-tuned classifier (tools/runner_finetune.py:835-899 test_vote of the reference:
// per test batch `times` subsets of the FPS order, each through test_transforms and the model; the mean of the logits,
// its argmax, the accuracy) around the forward: ONE launch prepares the point sets of all votes, ONE launch reduces their
// logits and counts the hits on the device.  Both are memory-trivial.
//   vote_resample  resample.hip's kernel with a vote axis: one thread per output point, the 12 map floats of the block's
//                  (vote, cloud) staged in LDS.
//   vote_reduce    one workgroup, a wave per row, a lane per class (k <= 64): the lane adds its class over the votes in
//                  order, the wave takes the argmax by a butterfly on a total order, lane 0 counts.
#include "common.h"

namespace pdae {

// resample_affine_kernel (resample.hip) for the votes k = 0 .. v-1 of a batch: the same statements on the same values,
// so the same bits.  has_a / has_t are launch-uniform.  Neither: the coordinates are moved, not computed on.  With a map:
// ((x A0j + y A1j) + z A2j) + tj, each operation rounded (-ffp-contract=off).  An index outside its array (a corrupt
// choice / fps_idx) is not followed: that point comes out as NaN.
__global__ __launch_bounds__(256) void vote_resample_kernel(int B, int P, int C, int point_all, int npoints, int chunks,
                                                            const float* __restrict__ raw, const int32_t* __restrict__ fps_idx,
                                                            const int32_t* __restrict__ choice, const float* __restrict__ A,
                                                            const float* __restrict__ t, float* __restrict__ out) {
  __shared__ float m[12];
  const int kb = blockIdx.x / chunks;                      // block-uniform: one (vote, cloud) per block
  const int k = kb / B, b = kb - k * B;
  const int n = (blockIdx.x - kb * chunks) * 256 + threadIdx.x;
  if (threadIdx.x < 9) m[threadIdx.x] = A ? A[(size_t)kb * 9 + threadIdx.x] : 0.f;
  else if (threadIdx.x < 12) m[threadIdx.x] = t ? t[(size_t)kb * 3 + (threadIdx.x - 9)] : 0.f;
  __syncthreads();
  if (n >= npoints) return;
  const int c = choice[(size_t)k * npoints + n];
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
  float* dst = out + ((size_t)kb * npoints + n) * 3;
  if (ok && A) {
    const float u = x * m[0] + y * m[3] + z * m[6];
    const float v = x * m[1] + y * m[4] + z * m[7];
    const float w = x * m[2] + y * m[5] + z * m[8];
    x = u, y = v, z = w;
  }
  if (ok && t) x += m[9], y += m[10], z += m[11];
  dst[0] = x, dst[1] = y, dst[2] = z;
}

constexpr int VOTE_THREADS = 256;
constexpr int VOTE_WAVES = VOTE_THREADS / kWave;

// Row r belongs to wave r % 4; lane c < K holds class c.  The argmax is a butterfly on the total order (larger value
// first, then the lower class), so its result does not depend on the butterfly's shape; +0 and -0 tie, as they do for
// torch.max.  The lanes c >= K carry -inf under the classes 64 + c, which lose every tie against a real class.
__global__ __launch_bounds__(VOTE_THREADS) void vote_reduce_kernel(int V, int B, int K, const float* __restrict__ logits,
                                                                   const int64_t* __restrict__ labels,
                                                                   float* __restrict__ mean_out, int64_t* __restrict__ pred_out,
                                                                   int32_t* __restrict__ correct) {
  __shared__ int s_hits[VOTE_WAVES];
  const int wave = threadIdx.x / kWave, lane = lane_id();
  const float fv = (float)V;
  int hits = 0;                                            // (counted by lane 0 of each wave)
  for (int r = wave; r < B; r += VOTE_WAVES) {
    float val = -__builtin_huge_valf();
    int cls = kWave + lane;
    bool nan = false;
    if (lane < K) {
      float s = logits[(size_t)r * K + lane];
      for (int k = 1; k < V; ++k) s += logits[((size_t)k * B + r) * K + lane];
      val = s / fv;
      cls = lane;
      nan = val != val;
      if (mean_out) mean_out[(size_t)r * K + lane] = val;
    }
    const bool any_nan = __any(nan);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      const float ov = __shfl_xor(val, o, kWave);
      const int oc = __shfl_xor(cls, o, kWave);
      if (ov > val || (ov == val && oc < cls)) val = ov, cls = oc;
    }
    const int64_t pred = any_nan ? -1 : (int64_t)cls;
    if (lane == 0) {
      pred_out[r] = pred;
      hits += pred >= 0 && pred == labels[r] ? 1 : 0;
    }
  }
  if (lane == 0) s_hits[wave] = hits;
  __syncthreads();
  if (threadIdx.x == 0) {
    int total = s_hits[0];
    for (int w = 1; w < VOTE_WAVES; ++w) total += s_hits[w];
    *correct = *correct + total;                           // the only writer: one workgroup, stream order between launches
  }
}

}  // namespace pdae

using namespace pdae;

extern "C" int pdae_vote_resample(int v, int b, int p, int c, int point_all, int npoints, const float* raw,
                                  const int32_t* fps_idx, const int32_t* choice, const float* A, const float* t, float* out,
                                  pdae_stream_t stream) {
  if (v <= 0 || b <= 0 || p <= 0 || c <= 0 || point_all <= 0 || npoints <= 0)
    return bad_arg("vote_resample: sizes must be positive");
  if (c < 3) return bad_arg("vote_resample: c >= 3 (the first three channels are the coordinates)");
  if (npoints > point_all) return bad_arg("vote_resample: npoints > point_all");
  if (!raw || !fps_idx || !choice || !out) return bad_arg("vote_resample: null pointer");
  const int chunks = (npoints + 255) / 256;
  if ((long long)v * b * chunks > 0x7fffffffLL) return unsupported("vote_resample: too many points for one launch");
  hipLaunchKernelGGL(vote_resample_kernel, dim3((unsigned)(v * b * chunks)), dim3(256), 0, as_stream(stream), b, p, c,
                     point_all, npoints, chunks, raw, fps_idx, choice, A, t, out);
  return check_launch("vote_resample");
}

extern "C" int pdae_vote_reduce(int v, int b, int k, const float* logits, const int64_t* labels, float* mean_out,
                                int64_t* pred_out, int32_t* correct, pdae_stream_t stream) {
  if (v < 1 || b < 1 || k < 1) return bad_arg("vote_reduce: v, b and k must be positive");
  if (!logits || !labels || !pred_out || !correct) return bad_arg("vote_reduce: null pointer");
  if (k > PDAE_VOTE_MAX_CLASSES) return unsupported("vote_reduce: more than PDAE_VOTE_MAX_CLASSES (64) classes");
  hipLaunchKernelGGL(vote_reduce_kernel, dim3(1), dim3(VOTE_THREADS), 0, as_stream(stream), v, b, k, logits, labels, mean_out,
                     pred_out, correct);
  return check_launch("vote_reduce");
}
