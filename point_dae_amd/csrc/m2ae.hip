// m2ae.hip -- the forward-only kernels of Point-M2AE's hierarchical encoder in evaluation mode.
//
// Reference: models/Point_M2AE.py:17-180 (H_Encoder.forward with eval=True), models/Point_M2AE_modules.py:169-216
// (Token_Embed) and :269-305 (Attention with the additive visibility / radius mask).
//
//   attention_local_forward   softmax(q k^T * scale + mask * -100000) v per (sample, head) with the mask evaluated in the
//       kernel from the token centres and the per-sample visible length: no (B, T, T) distance matrix or mask exists.
//       One workgroup per (128 queries, head, sample), one wave per 32 queries; the head's keys and values pass through
//       LDS 64 at a time with their centres.  The score tile is S^T = K Q^T on v_mfma_f32_32x32x2_f32 (rows = keys in
//       the 16 accumulator registers, lane = query: csrc/attention.hip's layout), so the softmax statistics are per
//       lane and P^T . V takes the accumulator registers as its A operand.  Two sweeps over the keys: the first finds
//       each query's score maximum, the second recomputes the scores and accumulates exp(s - max) and P V -- no
//       rescaling of O, whose rows (queries) sit in registers, not on lanes.
//   m2ae_compact / m2ae_pack / m2ae_unpack   the visible tokens of each sample, in ascending order, at the front of a
//       zero-padded (B, T_pad) buffer (:136-156) and back into the full token table (:174).
//   m2ae_group_max / m2ae_gather_max / m2ae_gather_add_relu   the per-patch steps of Token_Embed whose dense products
//       run on the row GEMMs (point_dae_amd/point_m2ae.py).
//   m2ae_embed_tail   level 0's second_conv on patches of 4..32 points: relu(F Wl^T + gb[patch]) W4^T, max over the
//       patch; the (R, 512) and (R, C) products live in LDS and accumulators only.
#include "common.h"

namespace pdae {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ int arow(int e, int h) { return (e & 3) + 8 * (e >> 2) + 4 * h; }

__device__ __forceinline__ void zero(f32x16& v) {
#pragma unroll
  for (int e = 0; e < 16; ++e) v[e] = 0.f;
}

constexpr int LKT = 64;      // keys staged per step

}  // namespace

// grid (ceil(T / 128), H, B), block 256.  qkv (B*T, 3*H*D) rows [3][H][D]; cen (B*T, 3); len (B); o (B*T, H*D).
template <int D>
__global__ __launch_bounds__(256) void m2ae_attn_local_kernel(int T, int H, float scale, float radius,
                                                              const float* __restrict__ qkv,
                                                              const float* __restrict__ cen,
                                                              const int* __restrict__ len, float* __restrict__ o) {
  constexpr int LD = D + 4;      // padded LDS row: conflict-free ds_read_b128
  constexpr int ND = (D + 31) / 32;
  __shared__ float Ks[LKT * LD];
  __shared__ float Vs[LKT * LD];
  __shared__ float Cs[LKT * 3];
  const int hd = blockIdx.y, b = blockIdx.z;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
  const int q0 = (blockIdx.x * 4 + w) * 32;
  const int qi = q0 + r;         // this lane's query (a column of S^T)
  const size_t rs = (size_t)3 * H * D;
  const float* base = qkv + (size_t)b * T * rs + hd * D;
  const float* cb = cen + (size_t)b * T * 3;
  const int L = len[b];
  float4 qreg[D / 8];
#pragma unroll
  for (int s = 0; s < D / 8; ++s)
    qreg[s] = qi < T ? *reinterpret_cast<const float4*>(base + (size_t)qi * rs + s * 8 + 4 * h)
                     : make_float4(0.f, 0.f, 0.f, 0.f);
  float cx = 0.f, cy = 0.f, cz = 0.f;
  if (qi < T) cx = cb[qi * 3], cy = cb[qi * 3 + 1], cz = cb[qi * 3 + 2];
  const bool qvalid = qi < L;

  // keys k0 .. k0 + 63 (zero rows past T) with their centres; values only in the second sweep
  auto stage = [&](int k0, bool with_v) {
    for (int i = threadIdx.x; i < LKT * (D / 4); i += 256) {
      const int row = i / (D / 4), c4 = (i % (D / 4)) * 4, key = k0 + row;
      float4 kv = make_float4(0.f, 0.f, 0.f, 0.f), vv = kv;
      if (key < T) {
        kv = *reinterpret_cast<const float4*>(base + (size_t)key * rs + (size_t)H * D + c4);
        if (with_v) vv = *reinterpret_cast<const float4*>(base + (size_t)key * rs + (size_t)2 * H * D + c4);
      }
      *reinterpret_cast<float4*>(Ks + row * LD + c4) = kv;
      if (with_v) *reinterpret_cast<float4*>(Vs + row * LD + c4) = vv;
    }
    if (threadIdx.x < LKT * 3) {
      const int key = k0 + threadIdx.x / 3;
      Cs[threadIdx.x] = key < T ? cb[(size_t)k0 * 3 + threadIdx.x] : 0.f;
    }
  };
  // mask_vis * (dist >= radius) == 0 (Point_M2AE.py:156-163): both tokens valid, or the centres closer than the radius
  auto allowed = [&](int key, int kl) -> bool {
    if (key >= T) return false;
    if (qvalid && key < L) return true;
    if (!(radius > 0.f)) return false;
    return sqrtf(sqdist(cx, cy, cz, Cs[kl * 3], Cs[kl * 3 + 1], Cs[kl * 3 + 2])) < radius;
  };
  auto scores = [&](f32x16& st, int j) {     // S^T of staged keys j*32 .. j*32+31 against this wave's queries
    zero(st);
#pragma unroll
    for (int s = 0; s < D / 8; ++s) {
      const float4 a = *reinterpret_cast<const float4*>(Ks + (j * 32 + r) * LD + s * 8 + 4 * h);
      st = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, qreg[s].x, st, 0, 0, 0);
      st = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, qreg[s].y, st, 0, 0, 0);
      st = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, qreg[s].z, st, 0, 0, 0);
      st = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, qreg[s].w, st, 0, 0, 0);
    }
  };

  float m = -__builtin_huge_valf();
  for (int k0 = 0; k0 < T; k0 += LKT) {
    __syncthreads();
    stage(k0, false);
    __syncthreads();
#pragma unroll
    for (int j = 0; j < LKT / 32; ++j) {
      if (k0 + j * 32 < T) {
        f32x16 st;
        scores(st, j);
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int kl = j * 32 + arow(e, h);
          if (allowed(k0 + kl, kl)) m = fmaxf(m, st[e] * scale);
        }
      }
    }
  }
  m = fmaxf(m, __shfl_xor(m, 32, kWave));

  float l = 0.f;
  f32x16 oa[ND];
#pragma unroll
  for (int dt = 0; dt < ND; ++dt) zero(oa[dt]);
  for (int k0 = 0; k0 < T; k0 += LKT) {
    __syncthreads();
    stage(k0, true);
    __syncthreads();
#pragma unroll
    for (int j = 0; j < LKT / 32; ++j) {
      if (k0 + j * 32 < T) {
        f32x16 st;
        scores(st, j);
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int kl = j * 32 + arow(e, h);
          const float p = allowed(k0 + kl, kl) ? expf(st[e] * scale - m) : 0.f;
          st[e] = p;
          l += p;
        }
#pragma unroll
        for (int dt = 0; dt < ND; ++dt) {
          const int col = dt * 32 + r < D ? dt * 32 + r : D - 1;      // (D = 16: lanes 16..31 repeat a column, unread)
#pragma unroll
          for (int e = 0; e < 16; ++e)
            oa[dt] = __builtin_amdgcn_mfma_f32_32x32x2f32(st[e], Vs[(j * 32 + arow(e, h)) * LD + col], oa[dt], 0, 0, 0);
        }
      }
    }
  }
  l += __shfl_xor(l, 32, kWave);
  const float inv = l > 0.f ? 1.0f / l : 0.f;      // (radius 0: a padded query has no key -- zeros)
  // oa: lane = d column, registers = query rows; the denominator sits on the lane that owns the query
#pragma unroll
  for (int dt = 0; dt < ND; ++dt) {
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int qrow = arow(e, h);
      const float iv = __shfl(inv, qrow, kWave);
      const int q = q0 + qrow, d = dt * 32 + r;
      if (q < T && d < D) o[((size_t)b * T + q) * H * D + hd * D + d] = oa[dt][e] * iv;
    }
  }
}

// One wave per sample: ids[b][0 .. len[b]) = the visible tokens in ascending order, -1 behind them.
__global__ __launch_bounds__(64) void m2ae_compact_kernel(int G, const unsigned char* __restrict__ masked,
                                                          int* __restrict__ len, int* __restrict__ ids) {
  const int b = blockIdx.x, lane = threadIdx.x;
  int count = 0;
  for (int g0 = 0; g0 < G; g0 += 64) {
    const int g = g0 + lane;
    const bool vis = g < G && masked[(size_t)b * G + g] == 0;
    const unsigned long long bal = __ballot(vis);
    if (vis) ids[(size_t)b * G + count + __popcll(bal & ((1ull << lane) - 1ull))] = g;
    count += __popcll(bal);
  }
  for (int i = count + lane; i < G; i += 64) ids[(size_t)b * G + i] = -1;
  if (lane == 0) len[b] = count;
}

// x (B*Tp, C) / cen (B*Tp, 3): row t of sample b = token ids[b][t] of the table, zeros for t >= len[b]
__global__ __launch_bounds__(256) void m2ae_pack_kernel(long long total, int G, int Tp, int C4,
                                                        const int* __restrict__ ids, const int* __restrict__ len,
                                                        const float4* __restrict__ tok, const float* __restrict__ ctr,
                                                        float4* __restrict__ x, float* __restrict__ cen) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const long long row = i / C4;
  const int c = (int)(i % C4), b = (int)(row / Tp), t = (int)(row % Tp);
  const int src = t < len[b] ? ids[(size_t)b * G + t] : -1;
  x[i] = src >= 0 ? tok[((size_t)b * G + src) * C4 + c] : make_float4(0.f, 0.f, 0.f, 0.f);
  if (c == 0) {
#pragma unroll
    for (int j = 0; j < 3; ++j) cen[row * 3 + j] = src >= 0 ? ctr[((size_t)b * G + src) * 3 + j] : 0.f;
  }
}

// the level's valid output rows back into the full token table (rows of dropped tokens keep their content)
__global__ __launch_bounds__(256) void m2ae_unpack_kernel(long long total, int G, int Tp, int C4,
                                                          const int* __restrict__ ids, const int* __restrict__ len,
                                                          const float4* __restrict__ x, float4* __restrict__ tok) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const long long row = i / C4;
  const int c = (int)(i % C4), b = (int)(row / Tp), t = (int)(row % Tp);
  if (t >= len[b]) return;
  const int dst = ids[(size_t)b * G + t];
  tok[((size_t)b * G + dst) * C4 + c] = x[i];
}

// out (P, C) = max over the n consecutive rows of each patch of x (P*n, C)
__global__ __launch_bounds__(256) void m2ae_group_max_kernel(long long total, int n, int C4,
                                                             const float4* __restrict__ x, float4* __restrict__ out) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const long long p = i / C4;
  const int c = (int)(i % C4);
  float4 v = x[(p * n) * C4 + c];
  for (int j = 1; j < n; ++j) {
    const float4 t = x[(p * n + j) * C4 + c];
    v.x = fmaxf(v.x, t.x), v.y = fmaxf(v.y, t.y), v.z = fmaxf(v.z, t.z), v.w = fmaxf(v.w, t.w);
  }
  out[i] = v;
}

// out (P, C) = max over the k rows idx[p][.] of x
__global__ __launch_bounds__(256) void m2ae_gather_max_kernel(long long total, int k, int C4,
                                                              const float4* __restrict__ x,
                                                              const long long* __restrict__ idx,
                                                              float4* __restrict__ out) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const long long p = i / C4;
  const int c = (int)(i % C4);
  float4 v = x[idx[p * k] * C4 + c];
  for (int j = 1; j < k; ++j) {
    const float4 t = x[idx[p * k + j] * C4 + c];
    v.x = fmaxf(v.x, t.x), v.y = fmaxf(v.y, t.y), v.z = fmaxf(v.z, t.z), v.w = fmaxf(v.w, t.w);
  }
  out[i] = v;
}

// out (P*k, C): row (p, j) = relu(x[idx[p][j]] + g[p])
__global__ __launch_bounds__(256) void m2ae_gather_add_relu_kernel(long long total, int k, int C4,
                                                                   const float4* __restrict__ x,
                                                                   const long long* __restrict__ idx,
                                                                   const float4* __restrict__ g,
                                                                   float4* __restrict__ out) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const long long row = i / C4;
  const int c = (int)(i % C4);
  const float4 a = x[idx[row] * C4 + c], t = g[(row / k) * C4 + c];
  out[i] = make_float4(fmaxf(a.x + t.x, 0.f), fmaxf(a.y + t.y, 0.f), fmaxf(a.z + t.z, 0.f), fmaxf(a.w + t.w, 0.f));
}

// tok (R/n, N4) = max over each patch's n rows of relu(F Wl^T + gb[patch]) W4^T, + b4.  32 rows (32 / n patches) per
// block of four waves.  The (32, N3) activation is formed 128 columns at a time (one 32x32 accumulator tile per wave,
// written to LDS with the patch's term and the ReLU) and consumed at once by the second product, whose 32-column
// output tiles stay in the accumulators of waves 0 .. N4/32 - 1 until the patch maxima are taken through LDS.
constexpr int TK = 256;       // widest F row
constexpr int TH = 128;       // activation columns per step
__global__ __launch_bounds__(256) void m2ae_embed_tail_kernel(int R, int n, int K, int N3, int N4,
                                                              const float* __restrict__ F,
                                                              const float* __restrict__ Wl,
                                                              const float* __restrict__ gb,
                                                              const float* __restrict__ W4,
                                                              const float* __restrict__ b4, float* __restrict__ tok) {
  __shared__ float Fs[32 * (TK + 4)];
  __shared__ float Hs[32 * (TH + 4)];
  const int LF = K + 4, LH = TH + 4;
  const int row0 = blockIdx.x * 32;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
  for (int i = threadIdx.x; i < 32 * (K / 4); i += 256) {
    const int row = i / (K / 4), c4 = (i % (K / 4)) * 4;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (row0 + row < R) v = *reinterpret_cast<const float4*>(F + (size_t)(row0 + row) * K + c4);
    *reinterpret_cast<float4*>(Fs + row * LF + c4) = v;
  }
  __syncthreads();
  const bool out_wave = w * 32 < N4;
  f32x16 acc4;
  zero(acc4);
  for (int c0 = 0; c0 < N3; c0 += TH) {
    {   // activation columns c0 + w*32 .. + 31: rows = points in the registers, lane = channel
      f32x16 acc;
      zero(acc);
      const float* wrow = Wl + (size_t)(c0 + w * 32 + r) * K + 4 * h;
      for (int s = 0; s < K / 8; ++s) {
        const float4 a = *reinterpret_cast<const float4*>(Fs + r * LF + s * 8 + 4 * h);
        const float4 bw = *reinterpret_cast<const float4*>(wrow + s * 8);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, bw.x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, bw.y, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, bw.z, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, bw.w, acc, 0, 0, 0);
      }
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int prow = arow(e, h), grow = row0 + prow;
        const float t = grow < R ? gb[(size_t)(grow / n) * N3 + c0 + w * 32 + r] : 0.f;
        Hs[prow * LH + w * 32 + r] = fmaxf(acc[e] + t, 0.f);
      }
    }
    __syncthreads();
    if (out_wave) {
      const float* wrow = W4 + (size_t)(w * 32 + r) * N3 + c0 + 4 * h;
      for (int s = 0; s < TH / 8; ++s) {
        const float4 a = *reinterpret_cast<const float4*>(Hs + r * LH + s * 8 + 4 * h);
        const float4 bw = *reinterpret_cast<const float4*>(wrow + s * 8);
        acc4 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, bw.x, acc4, 0, 0, 0);
        acc4 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, bw.y, acc4, 0, 0, 0);
        acc4 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, bw.z, acc4, 0, 0, 0);
        acc4 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, bw.w, acc4, 0, 0, 0);
      }
    }
    __syncthreads();
  }
  if (out_wave) {
#pragma unroll
    for (int e = 0; e < 16; ++e) Hs[arow(e, h) * LH + w * 32 + r] = acc4[e];
  }
  __syncthreads();
  const int patches = 32 / n;
  for (int i = threadIdx.x; i < patches * N4; i += 256) {
    const int pp = i / N4, c = i % N4;
    const long long g = (long long)(row0 / n) + pp;
    if (g * n >= R) continue;
    float v = Hs[(pp * n) * LH + c];
    for (int j = 1; j < n; ++j) v = fmaxf(v, Hs[(pp * n + j) * LH + c]);
    tok[(size_t)g * N4 + c] = v + b4[c];
  }
}

}  // namespace pdae

using namespace pdae;

static inline unsigned blocks256(long long total) { return (unsigned)((total + 255) / 256); }

extern "C" int pdae_attention_local_forward(int B, int T, int H, int D, float scale, float radius, const float* qkv,
                                            const float* centres, const int32_t* len, float* o, pdae_stream_t stream) {
  if (B < 0 || T <= 0 || H <= 0) return bad_arg("attention_local: bad size");
  if (D != 16 && D != 32 && D != 64) return unsupported("attention_local: head dim must be 16, 32 or 64");
  if (T > 512) return unsupported("attention_local: T > 512 not implemented");
  if (B > 65535 || H > 65535) return unsupported("attention_local: B or H > 65535");
  if (!(radius >= 0.f)) return bad_arg("attention_local: radius >= 0 required");
  if (B == 0) return PDAE_OK;
  if (!qkv || !centres || !len || !o) return bad_arg("attention_local: null pointer");
  hipStream_t s = as_stream(stream);
  const dim3 grid((unsigned)((T + 127) / 128), (unsigned)H, (unsigned)B);
  if (D == 16) hipLaunchKernelGGL(m2ae_attn_local_kernel<16>, grid, dim3(256), 0, s, T, H, scale, radius, qkv, centres, len, o);
  else if (D == 32) hipLaunchKernelGGL(m2ae_attn_local_kernel<32>, grid, dim3(256), 0, s, T, H, scale, radius, qkv, centres, len, o);
  else hipLaunchKernelGGL(m2ae_attn_local_kernel<64>, grid, dim3(256), 0, s, T, H, scale, radius, qkv, centres, len, o);
  return check_launch("attention_local_forward");
}

extern "C" int pdae_m2ae_compact(int B, int G, const uint8_t* masked, int32_t* len, int32_t* ids, pdae_stream_t stream) {
  if (B < 0 || G <= 0) return bad_arg("m2ae_compact: B >= 0, G > 0 required");
  if (B == 0) return PDAE_OK;
  if (!masked || !len || !ids) return bad_arg("m2ae_compact: null pointer");
  hipLaunchKernelGGL(m2ae_compact_kernel, dim3((unsigned)B), dim3(64), 0, as_stream(stream), G, masked, len, ids);
  return check_launch("m2ae_compact");
}

static int pack_args(const char* what, int B, int G, int Tp, int C) {
  if (B < 0 || G <= 0 || Tp <= 0 || Tp > G || C <= 0 || C % 4 != 0) {
    set_error(what);
    return PDAE_ERR_BAD_ARG;
  }
  return PDAE_OK;
}

extern "C" int pdae_m2ae_pack(int B, int G, int Tp, int C, const int32_t* ids, const int32_t* len, const float* tokens,
                              const float* centres, float* x, float* cen, pdae_stream_t stream) {
  if (int rc = pack_args("m2ae_pack: B >= 0, 0 < T_pad <= G, C a positive multiple of 4 required", B, G, Tp, C)) return rc;
  if (B == 0) return PDAE_OK;
  const long long total = (long long)B * Tp * (C / 4);
  if ((total + 255) / 256 > 0x7fffffffLL) return unsupported("m2ae_pack: too many elements");
  if (!ids || !len || !tokens || !centres || !x || !cen) return bad_arg("m2ae_pack: null pointer");
  hipLaunchKernelGGL(m2ae_pack_kernel, dim3(blocks256(total)), dim3(256), 0, as_stream(stream), total, G, Tp, C / 4, ids,
                     len, reinterpret_cast<const float4*>(tokens), centres, reinterpret_cast<float4*>(x), cen);
  return check_launch("m2ae_pack");
}

extern "C" int pdae_m2ae_unpack(int B, int G, int Tp, int C, const int32_t* ids, const int32_t* len, const float* x,
                                float* tokens, pdae_stream_t stream) {
  if (int rc = pack_args("m2ae_unpack: B >= 0, 0 < T_pad <= G, C a positive multiple of 4 required", B, G, Tp, C)) return rc;
  if (B == 0) return PDAE_OK;
  const long long total = (long long)B * Tp * (C / 4);
  if ((total + 255) / 256 > 0x7fffffffLL) return unsupported("m2ae_unpack: too many elements");
  if (!ids || !len || !tokens || !x) return bad_arg("m2ae_unpack: null pointer");
  hipLaunchKernelGGL(m2ae_unpack_kernel, dim3(blocks256(total)), dim3(256), 0, as_stream(stream), total, G, Tp, C / 4, ids,
                     len, reinterpret_cast<const float4*>(x), reinterpret_cast<float4*>(tokens));
  return check_launch("m2ae_unpack");
}

extern "C" int pdae_m2ae_group_max(long long P, int n, int C, const float* x, float* out, pdae_stream_t stream) {
  if (P < 0 || n <= 0 || C <= 0 || C % 4 != 0) return bad_arg("m2ae_group_max: n > 0, C a positive multiple of 4 required");
  if (P == 0) return PDAE_OK;
  if (!x || !out) return bad_arg("m2ae_group_max: null pointer");
  const long long total = P * (C / 4);
  if ((total + 255) / 256 > 0x7fffffffLL) return unsupported("m2ae_group_max: too many elements");
  hipLaunchKernelGGL(m2ae_group_max_kernel, dim3(blocks256(total)), dim3(256), 0, as_stream(stream), total, n, C / 4,
                     reinterpret_cast<const float4*>(x), reinterpret_cast<float4*>(out));
  return check_launch("m2ae_group_max");
}

extern "C" int pdae_m2ae_gather_max(long long P, int k, int C, const float* x, const int64_t* idx, float* out,
                                    pdae_stream_t stream) {
  if (P < 0 || k <= 0 || C <= 0 || C % 4 != 0) return bad_arg("m2ae_gather_max: k > 0, C a positive multiple of 4 required");
  if (P == 0) return PDAE_OK;
  if (!x || !idx || !out) return bad_arg("m2ae_gather_max: null pointer");
  const long long total = P * (C / 4);
  if ((total + 255) / 256 > 0x7fffffffLL) return unsupported("m2ae_gather_max: too many elements");
  hipLaunchKernelGGL(m2ae_gather_max_kernel, dim3(blocks256(total)), dim3(256), 0, as_stream(stream), total, k, C / 4,
                     reinterpret_cast<const float4*>(x), reinterpret_cast<const long long*>(idx),
                     reinterpret_cast<float4*>(out));
  return check_launch("m2ae_gather_max");
}

extern "C" int pdae_m2ae_gather_add_relu(long long P, int k, int C, const float* x, const int64_t* idx, const float* g,
                                         float* out, pdae_stream_t stream) {
  if (P < 0 || k <= 0 || C <= 0 || C % 4 != 0) return bad_arg("m2ae_gather_add_relu: k > 0, C a positive multiple of 4 required");
  if (P == 0) return PDAE_OK;
  if (!x || !idx || !g || !out) return bad_arg("m2ae_gather_add_relu: null pointer");
  const long long total = P * k * (C / 4);
  if ((total + 255) / 256 > 0x7fffffffLL) return unsupported("m2ae_gather_add_relu: too many elements");
  hipLaunchKernelGGL(m2ae_gather_add_relu_kernel, dim3(blocks256(total)), dim3(256), 0, as_stream(stream), total, k, C / 4,
                     reinterpret_cast<const float4*>(x), reinterpret_cast<const long long*>(idx),
                     reinterpret_cast<const float4*>(g), reinterpret_cast<float4*>(out));
  return check_launch("m2ae_gather_add_relu");
}

extern "C" int pdae_m2ae_embed_tail(long long R, int n, int K, int N3, int N4, const float* F, const float* Wl,
                                    const float* gb, const float* W4, const float* b4, float* tok, pdae_stream_t stream) {
  if (R < 0 || (n != 4 && n != 8 && n != 16 && n != 32) || R % n != 0)
    return bad_arg("m2ae_embed_tail: patches of 4, 8, 16 or 32 rows required");
  if (K <= 0 || K > TK || K % 8 != 0 || N3 <= 0 || N3 % TH != 0 || N4 <= 0 || N4 > 128 || N4 % 32 != 0)
    return unsupported("m2ae_embed_tail: K % 8 == 0, K <= 256, N3 % 128 == 0, N4 % 32 == 0, N4 <= 128 required");
  if (R >= (1LL << 31)) return unsupported("m2ae_embed_tail: too many rows");
  if (R == 0) return PDAE_OK;
  if (!F || !Wl || !gb || !W4 || !b4 || !tok) return bad_arg("m2ae_embed_tail: null pointer");
  hipLaunchKernelGGL(m2ae_embed_tail_kernel, dim3((unsigned)((R + 31) / 32)), dim3(256), 0, as_stream(stream), (int)R, n, K,
                     N3, N4, F, Wl, gb, W4, b4, tok);
  return check_launch("m2ae_embed_tail");
}
