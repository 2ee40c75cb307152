// fewshot.hip -- the training batch of a few-shot episode (datasets/ModelNetDatasetFewShot.py:59-71 of the reference: the
// item, a fresh shuffle of its points on every access; tools/runner_finetune.py:158-176: FPS to point_all points, a host
// draw of npoints of them, the gather) in ONE launch from the resident episode to the step's input.
//
// The loop is fps.hip's: one workgroup per batch row, the cloud and the running minima in registers, the cloud staged in
// LDS for the centre read, the 64-bit key maximum with one barrier per iteration; the key, the skipped-point rule and the
// tie order are restated from there (the rank of a point is that of its position k in the SHUFFLED cloud).  What differs:
//   * lane slot k loads set[item[b]][perm[b][k]], so the shuffled cloud exists only in registers and LDS;
//   * the picked positions are kept in LDS and the results leave in one parallel sweep behind the loop (out through
//     `slot`, idx through `perm`): the serial loop stores nothing to memory and waits for no load.
// The body is a kernel of its own and not a template parameter of fps_kernel: with the results leaving behind the loop
// it is no longer the same loop (fps_kernel's thread 0 stores idxs / centres every iteration), and fps_kernel's
// instantiations -- the pretraining step's FPS -- stay the code they were (few-shot).
//
// pdae_resident_batch (the augmented ModelNet40 training batch from the resident set: datasets/ModelNetDataset.py:127-158,
// augment_data's per-access maps in front of the shuffle) is this kernel with the compile-time flag MAPS; both entries
// share the argument checks and the ladder (fewshot_dispatch), and pdae_fewshot_batch launches MAPS = false.
#include <cmath>
#include <cstdio>

#include "common.h"

namespace pdae {

// MAPS (pdae_resident_batch): row b's point is sent through its nmaps[b] <= 3 affine maps y = x M + t, one after the other
// with norm_affine_kernel's arithmetic (pipeline.hip), between the load and everything that looks at the coordinates --
// the skipped-point rule, the registers, the LDS copy.  The maps are block-uniform values read in the load phase only: the
// serial loop below is the same code in both instantiations.
template <int T, int P, bool MAPS>
__global__ __launch_bounds__(T) void fewshot_batch_kernel(int s, int p, int c, int m, int npoints, int bs_log2, int cols,
                                                          const float* __restrict__ set, const int32_t* __restrict__ item,
                                                          const int32_t* __restrict__ perm, const int32_t* __restrict__ nmaps,
                                                          const float* __restrict__ maps, const int32_t* __restrict__ slot,
                                                          float* __restrict__ out, int32_t* __restrict__ idx) {
  constexpr int W = T / kWave;
  extern __shared__ float lds_xyz[];  // p*3 floats, then m picked positions (int)
  __shared__ unsigned long long slots[2][W > 1 ? W : 1];
  int* picked = reinterpret_cast<int*>(lds_xyz + (size_t)p * 3);

  const int tid = threadIdx.x;
  const int b = blockIdx.x;
  const int it = item[b];
  out += (size_t)b * npoints * 3;
  if (idx) idx += (size_t)b * m;
  const int nm = MAPS ? nmaps[b] : 0;
  // block-uniform, in front of every barrier: the row is marked, nothing is read
  if ((unsigned)it >= (unsigned)s || (MAPS && (unsigned)nm > 3u)) {
    const float nan = __builtin_nanf("");
    for (int i = tid; i < npoints * 3; i += T) out[i] = nan;
    if (idx)
      for (int j = tid; j < m; j += T) idx[j] = -1;
    return;
  }
  const float* cloud = set + (size_t)it * p * c;
  if (perm) perm += (size_t)b * p;

  float px[P], py[P], pz[P], temp[P];
  unsigned low[P];
  const int bs_mask = (1 << bs_log2) - 1;
#pragma unroll
  for (int i = 0; i < P; ++i) {
    const int k = tid + i * T;
    float x = 0.f, y = 0.f, z = 0.f;
    bool valid = false;
    if (k < p) {
      const int src = perm ? perm[k] : k;
      if ((unsigned)src < (unsigned)p) {  // an entry outside the cloud is not followed: the position reads as (0,0,0)
        const float* q = cloud + (size_t)src * c;
        x = q[0];
        y = q[1];
        z = q[2];
        if (MAPS) {
          for (int a = 0; a < nm; ++a) {
            const float* M = maps + ((size_t)b * 3 + a) * 12;
            const float x0 = x, y0 = y, z0 = z;
            x = ((x0 * M[0] + y0 * M[3]) + z0 * M[6]) + M[9];  // row vector times matrix, then t: norm_affine_kernel's order
            y = ((x0 * M[1] + y0 * M[4]) + z0 * M[7]) + M[10];
            z = ((x0 * M[2] + y0 * M[5]) + z0 * M[8]) + M[11];
          }
        }
        const float mag = (x * x) + (y * y) + (z * z);
        valid = !((double)mag <= 1e-3);
      }
      lds_xyz[k * 3 + 0] = x;
      lds_xyz[k * 3 + 1] = y;
      lds_xyz[k * 3 + 2] = z;
    }
    px[i] = x;
    py[i] = y;
    pz[i] = z;
    // skipped / padded points: temp = 0 keeps d2 = +0 and low = 0 -> key 0
    temp[i] = valid ? 1e10f : 0.f;
    const unsigned rev = bs_log2 ? (__brev((unsigned)(k & bs_mask)) >> (32 - bs_log2)) : 0u;
    const unsigned rank = rev * (unsigned)cols + (unsigned)(k >> bs_log2);
    low[i] = valid ? (((0xFFFFu - rank) << 16) | (unsigned)k) : 0u;
  }
  int old = 0;
  if (tid == 0) picked[0] = 0;
  __syncthreads();

  for (int j = 1; j < m; ++j) {
    const float x1 = lds_xyz[old * 3 + 0];
    const float y1 = lds_xyz[old * 3 + 1];
    const float z1 = lds_xyz[old * 3 + 2];
    unsigned long long best = 0;
#pragma unroll
    for (int i = 0; i < P; ++i) {
      const float d = sqdist(px[i], py[i], pz[i], x1, y1, z1);
      const float d2 = fminf(d, temp[i]);
      temp[i] = d2;
      const unsigned long long key = ((unsigned long long)__float_as_uint(d2) << 32) | low[i];
      best = max_u64(best, key);
    }
    best = wave_max_u64(best);
    if (W > 1) {
      if (lane_id() == 0) slots[j & 1][tid / kWave] = best;
      __syncthreads();
      unsigned long long r = 0;
#pragma unroll
      for (int w = 0; w < W; ++w) r = max_u64(r, slots[j & 1][w]);
      best = r;
    }
    old = (int)(best & 0xFFFFull);  // < p: the low 16 bits of a key are 0 or the k < p of a loaded point
    if (tid == 0) picked[j] = old;
  }
  __syncthreads();

  // column j of the FPS order: position picked[j] of the shuffled cloud
  for (int j = tid; j < m; j += T) {
    const int k = picked[j];
    if (idx) idx[j] = perm ? perm[k] : k;
    const int row = slot ? slot[j] : j;
    if ((unsigned)row < (unsigned)npoints) {
      out[row * 3 + 0] = lds_xyz[k * 3 + 0];
      out[row * 3 + 1] = lds_xyz[k * 3 + 1];
      out[row * 3 + 2] = lds_xyz[k * 3 + 2];
    }
  }
}

// cuda_utils.h:15-21 opt_n_threads, as in fps.hip: the reference's block size decides the tie order
static int fewshot_ref_block_size(int work_size) {
  const int pow_2 = (int)(std::log(static_cast<double>(work_size)) / std::log(2.0));
  int v = 1 << pow_2;
  if (v > 512) v = 512;
  if (v < 1) v = 1;
  return v;
}

template <int T, int P>
static void launch_fewshot(int s, int p, int c, int b, int m, int npoints, int bs_log2, int cols, const float* set,
                           const int32_t* item, const int32_t* perm, const int32_t* nmaps, const float* maps,
                           const int32_t* slot, float* out, int32_t* idx, hipStream_t st) {
  const size_t lds_bytes = (size_t)p * 3 * sizeof(float) + (size_t)m * sizeof(int);
  if (nmaps)
    hipLaunchKernelGGL((fewshot_batch_kernel<T, P, true>), dim3(b), dim3(T), lds_bytes, st, s, p, c, m, npoints, bs_log2,
                       cols, set, item, perm, nmaps, maps, slot, out, idx);
  else
    hipLaunchKernelGGL((fewshot_batch_kernel<T, P, false>), dim3(b), dim3(T), lds_bytes, st, s, p, c, m, npoints, bs_log2,
                       cols, set, item, perm, nmaps, maps, slot, out, idx);
}

// the argument checks and the T/P ladder both entries share; `what` prefixes the messages.  nmaps == NULL: no maps.
static int fewshot_dispatch(const char* what, int s, int p, int c, int b, int m, int npoints, const float* set,
                            const int32_t* item, const int32_t* perm, const int32_t* nmaps, const float* maps,
                            const int32_t* slot, float* out, int32_t* idx, pdae_stream_t stream) {
  char msg[160];
#define PDAE_FEWSHOT_FAIL(fn, text) return (snprintf(msg, sizeof msg, "%s: %s", what, text), fn(msg))
  if (s <= 0 || p <= 0 || b < 0 || m < 0 || npoints < 0) PDAE_FEWSHOT_FAIL(bad_arg, "s>0, p>0, b>=0, m>=0, npoints>=0 required");
  if (c < 3) PDAE_FEWSHOT_FAIL(bad_arg, "c >= 3 (the first three channels are the coordinates)");
  if (m > p) PDAE_FEWSHOT_FAIL(bad_arg, "m > p");
  if (!slot && npoints != m) PDAE_FEWSHOT_FAIL(bad_arg, "without slot, npoints must equal m");
  if (nmaps && !maps) PDAE_FEWSHOT_FAIL(bad_arg, "nmaps without maps");
  if (b == 0 || m == 0) return PDAE_OK;
  if (!set || !item || !out) PDAE_FEWSHOT_FAIL(bad_arg, "null pointer");
  if (p > 8192) PDAE_FEWSHOT_FAIL(unsupported, "p > 8192 not implemented (the clouds have 8192 points)");
#undef PDAE_FEWSHOT_FAIL
  const int bs = fewshot_ref_block_size(p);
  int bs_log2 = 0;
  while ((1 << bs_log2) < bs) ++bs_log2;
  const int cols = (p + bs - 1) / bs;
  hipStream_t st = as_stream(stream);
  // the T/P ladder of pdae_furthest_point_sampling
#define PDAE_FEWSHOT_LAUNCH(T, P) \
  launch_fewshot<T, P>(s, p, c, b, m, npoints, bs_log2, cols, set, item, perm, nmaps, maps, slot, out, idx, st)
  if (p <= 64) PDAE_FEWSHOT_LAUNCH(64, 1);
  else if (p <= 128) PDAE_FEWSHOT_LAUNCH(64, 2);
  else if (p <= 256) PDAE_FEWSHOT_LAUNCH(128, 2);
  else if (p <= 512) PDAE_FEWSHOT_LAUNCH(256, 2);
  else if (p <= 1024) PDAE_FEWSHOT_LAUNCH(256, 4);
  else if (p <= 2048) PDAE_FEWSHOT_LAUNCH(512, 4);
  else if (p <= 4096) PDAE_FEWSHOT_LAUNCH(1024, 4);
  else PDAE_FEWSHOT_LAUNCH(1024, 8);
#undef PDAE_FEWSHOT_LAUNCH
  return check_launch(what);
}

}  // namespace pdae

extern "C" int pdae_fewshot_batch(int s, int p, int c, int b, int m, int npoints, const float* set, const int32_t* item,
                                  const int32_t* perm, const int32_t* slot, float* out, int32_t* idx,
                                  pdae_stream_t stream) {
  return pdae::fewshot_dispatch("fewshot_batch", s, p, c, b, m, npoints, set, item, perm, nullptr, nullptr, slot, out, idx,
                                stream);
}

// The augmented training batch of a resident set (datasets.ModelNet on the reference's files): pdae_fewshot_batch with the
// per-row maps of augment_data in front of the FPS.
extern "C" int pdae_resident_batch(int s, int p, int c, int b, int m, int npoints, const float* set, const int32_t* item,
                                   const int32_t* perm, const int32_t* nmaps, const float* maps, const int32_t* slot,
                                   float* out, int32_t* idx, pdae_stream_t stream) {
  return pdae::fewshot_dispatch("resident_batch", s, p, c, b, m, npoints, set, item, perm, nmaps, maps, slot, out, idx,
                                stream);
}
