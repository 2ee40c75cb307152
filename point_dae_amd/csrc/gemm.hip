// gemm.hip -- the fp32-input NT GEMM on the gfx950 matrix cores (v_mfma_f32_32x32x2_f32) with the producer / epilogue
// fusions of the patch embedder and of the set-abstraction MLPs, and the K = 4 pass of a set-abstraction level's
// first layer.
//
// The entries below are the fused dense layers of the embedder (models/PointCAE_transformer.py:24-51) and of the
// shared MLPs: BatchNorm / ReLU / max-pool / concat, separate full passes over (B*G*32, 512) tensors in the
// reference (537 MB each at B=128), ride on the product as producers and epilogues.  Each entry builds an NtArgs and
// hands it to the exact-split bf16 kernel of the same contracts (rows3_kernel.h conv3_kernel, through
// rows3::conv3_takes / launch_conv3) -- the default arithmetic -- or to gemm_nt_kernel below: under
// PDAE_GEMM=f32mfma, and in either arithmetic when K % 32 != 0.  The fp32 MFMA of CDNA4 is exact fp32 (a k-ordered
// fmaf chain) at the fp32 vector peak (157 TFLOP/s): the reference's arithmetic class, no TF32/bf16.  No float
// atomics in any product; the BatchNorm column statistics alone use them outside deterministic mode.
//
// Kernel "NT":  C[M,N] = epi( pro(A)[M,K] . B[N,K]^T )          (both K-contiguous)
//   - block tile BM x BN (256x256 with 16 waves, 128x384 with 12, or 128x128 with 4),
//     BK = 32; every wave owns 64x64 = 2x2 MFMA tiles of 32x32 (64 accumulators/lane).
//     Measured on MI355X (B=128 shapes): 256x256 tiles 112-126
//     TFLOP/s (0.70 MFMA-busy), hipBLASLt 129-139 on the same shapes.
//   - The k index inside an 8-deep slab is permuted so that one ds_read_b128 per
//     operand row feeds four MFMAs: lane (r = l&31, h = l>>5) supplies
//     k = 8s + 4h + t to MFMA t (same permutation on A and B).  LDS rows are
//     padded to 36 floats: the four 16-lane groups of a ds_read_b128 then hit 64
//     distinct banks.
//   - global -> registers -> LDS staging, two LDS buffers, ONE barrier per
//     k-tile.  The issue order inside a k-tile is pinned with sched_group_barrier:
//     the loads of tile t+1 behind the first MFMAs of tile t, one fragment read of
//     the next 8-deep group behind every four MFMAs, the LDS stores of tile t+1
//     behind the last ones.
//   - persistent blocks: one residency of the chip; a block walks the tiles
//     slot, slot + nslots, ... of its XCD's contiguous chunk (blocks b, b+8, ...
//     share an L2; n fastest), and the slabs of consecutive tiles form one stream
//     through the LDS double buffer, so a tile boundary costs only the epilogue.
//   producers (applied to A while it is staged):
//     PRO_BNRELU   a := max(0, a * scale[k] + shift[k])   -- BatchNorm + ReLU of
//                  the previous layer never materialised; optional gather of whole
//                  32-row groups (a_groups)
//   epilogues:
//     EPI_GROUPBIAS_STATS    C = acc + gbias[m/32][n]; per-column sum / sum of
//                            squares of C accumulated into stats (BatchNorm
//                            batch statistics without another pass over C)
//     EPI_STATS              C = acc (+ bias[n]) with the same statistics
//     EPI_GROUPMAX           out[m/32][n] = max over the 32 rows of a group of
//                            (acc + bias[n]), arg[m/32][n] = first row attaining
//                            it; C itself is never written (max-pool fused)
//     EPI_STORE_GROUPMAX     both C = acc + bias and the group max / argmax
//     EPI_GROUP_SCATTER      C[c_groups[m/32]*32 + m%32] = acc + gbias[m/32][n]
// Pass "K = 4" (conv_k4_stats_kernel): the first layer of a set-abstraction level on coordinates alone -- its (M, N)
//     store is all there is; see the kernel.
#include <type_traits>
#include <cstdlib>

#include "common.h"
#include "nt_args.h"

namespace pdae {
int gemm_arith_rows();                                   // rows_gemm.hip: PDAE_GEMM_BF16X3 unless the fp32-input kernels were asked for
namespace rows3 {
bool conv3_takes(const NtArgs& a, int pro, int epi);    // rows3_gemm.hip: the same contracts on exact-split bf16
void launch_conv3(NtArgs& a, int pro, int epi, hipStream_t s);
}  // namespace rows3
// embed.hip: the stand-alone sweeps the folded epilogues replace, for the products conv3_kernel does not take
int group_sum_all(hipStream_t s, int G, int C, const float* X, float* out);
int group_scatter_add_listed(hipStream_t s, int n_listed, int C, int ld, const float* grad, const unsigned char* arg,
                             const int* groups, float* dst);
}  // namespace pdae

namespace pdae {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int GBK = 32, GLD = GBK + 4;

__device__ __forceinline__ float act_relu(float v) { return v > 0.f ? v : 0.f; }

template <int BM, int BN, int PRO, int EPI>
__global__ __launch_bounds__((BM / 64) * (BN / 64) * 64) void gemm_nt_kernel(const NtArgs p) {
  constexpr int WN = BN / 64;
  constexpr int NT = (BM / 64) * (BN / 64) * 64;
  constexpr int LA = (BM * 8 + NT - 1) / NT, LB = (BN * 8 + NT - 1) / NT;  // float4 per thread
  extern __shared__ float lds[];    // [2][(BM + BN) * GLD]
  // Persistent blocks: block (xcd, slot) walks tiles slot, slot + nslots, ... of its XCD's
  // chunk.  The slabs of consecutive tiles form ONE stream through the double-buffered LDS:
  // while a tile's last slab is multiplied the next tile's first slab is loaded and stored,
  // so a tile boundary costs the epilogue only -- no block relaunch, no exposed first load
  // (measured before: ~12-17 us of fixed cost per 256x256 tile, 20 % of conv3's time).
  const int chunk = (p.tiles + 7) >> 3;
  const int xcd = blockIdx.x & 7, nslots = gridDim.x >> 3;
  int slot = blockIdx.x >> 3;
  auto tile_of = [&](int sl) {
    const int t = xcd * chunk + sl;
    return (sl < chunk && t < p.tiles) ? t : -1;
  };
  int tile = tile_of(slot);
  if (tile < 0) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const int r = lane & 31, h = lane >> 5;
  const int r_ = r, h_ = h, wm_ = wm, wn_ = wn;
  const int scol = (tid & 7) * 4;
  const int M = p.M, N = p.N, K = p.K;

  // staging slot i of this thread is tile row (tid + i*NT) / 8; rows past the
  // matrix edge are clamped (their results are never stored), slots past the
  // tile (only when NT does not divide the tile) are skipped
  int m0 = 0, n0 = 0;
  // 32-bit element offsets from the (scalar) operand bases: one VGPR per staged row and the
  // base + offset addressing form of global_load (the launcher checks the operands fit)
  unsigned arow[LA], brow[LB];
  auto set_tile = [&](int t) {
    m0 = (t / p.tiles_n) * BM, n0 = (t % p.tiles_n) * BN;
#pragma unroll
    for (int i = 0; i < LA; ++i) {
      int m = min(m0 + ((tid + i * NT) >> 3), M - 1);
      if (p.a_groups) m = p.a_groups[m >> 5] * 32 + (m & 31);   // gather whole 32-row groups
      arow[i] = (unsigned)m * (unsigned)p.lda + scol;
    }
#pragma unroll
    for (int i = 0; i < LB; ++i)
      brow[i] = (unsigned)min(n0 + ((tid + i * NT) >> 3), N - 1) * (unsigned)p.ldb + scol;
  };
  set_tile(tile);
  auto a_ok = [&](int i) { return (BM * 8) % NT == 0 || ((tid + i * NT) >> 3) < BM; };
  auto b_ok = [&](int i) { return (BN * 8) % NT == 0 || ((tid + i * NT) >> 3) < BN; };

  float4 ra[LA], rb[LB];
  auto gload = [&](int kt) {
    const int k = kt * GBK;
    if (k + GBK <= K) {
#pragma unroll
      for (int i = 0; i < LA; ++i) ra[i] = *reinterpret_cast<const float4*>(p.A + (arow[i] + (unsigned)k));
#pragma unroll
      for (int i = 0; i < LB; ++i) rb[i] = *reinterpret_cast<const float4*>(p.B + (brow[i] + (unsigned)k));
    } else {  // partial last k-tile (K % 4 == 0): zero-fill
      const bool in = k + scol < K;
#pragma unroll
      for (int i = 0; i < LA; ++i)
        ra[i] = in ? *reinterpret_cast<const float4*>(p.A + (arow[i] + (unsigned)k)) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
      for (int i = 0; i < LB; ++i)
        rb[i] = in ? *reinterpret_cast<const float4*>(p.B + (brow[i] + (unsigned)k)) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    if (PRO == PRO_BNRELU) {
      const int kk = k + scol;
      if (kk < K) {
        const float4 sc = *reinterpret_cast<const float4*>(p.pro_scale + kk);
        const float4 sh = *reinterpret_cast<const float4*>(p.pro_shift + kk);
#pragma unroll
        for (int i = 0; i < LA; ++i) {
          ra[i].x = act_relu(ra[i].x * sc.x + sh.x);
          ra[i].y = act_relu(ra[i].y * sc.y + sh.y);
          ra[i].z = act_relu(ra[i].z * sc.z + sh.z);
          ra[i].w = act_relu(ra[i].w * sc.w + sh.w);
        }
      }
    }
  };
  auto lstore = [&](int buf) {
    float* As = lds + buf * (BM + BN) * GLD;
    float* Bs = As + BM * GLD;
#pragma unroll
    for (int i = 0; i < LA; ++i)
      if (a_ok(i)) *reinterpret_cast<float4*>(As + ((tid + i * NT) >> 3) * GLD + scol) = ra[i];
#pragma unroll
    for (int i = 0; i < LB; ++i)
      if (b_ok(i)) *reinterpret_cast<float4*>(Bs + ((tid + i * NT) >> 3) * GLD + scol) = rb[i];
  };

  f32x16 acc[2][2];
  const int KT = (K + GBK - 1) / GBK;
  gload(0);
  lstore(0);
  __syncthreads();
  int buf = 0;
  while (true) {
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      // EPI_GROUPBIAS_STATS: the accumulators START at the group's bias (a 32-row MFMA tile is one group,
      // a lane holds one column of it: one value for its 16 registers) -- the epilogue then has no add and
      // four live registers fewer at the kernel's 128-VGPR limit
      float init = 0.f;
      if (EPI == EPI_GROUPBIAS_STATS || EPI == EPI_GROUP_SCATTER) {
        const int gr = m0 + wm * 64 + i * 32, gc = n0 + wn * 64 + j * 32 + r;
        if (gr < M && gc < N && (EPI == EPI_GROUPBIAS_STATS || p.gbias)) init = p.gbias[(size_t)(gr >> 5) * N + gc];
      }
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = init;
    }
  int em0 = m0, en0 = n0, next = -1;   // the tile being multiplied (m0/n0 move on to the next one early)
  for (int kt = 0; kt < KT; ++kt) {
    bool more = kt + 1 < KT;
    if (more) {
      gload(kt + 1);
    } else {
      next = tile_of(slot + nslots);
      // (opaque: otherwise the next tile's address arithmetic is hoisted above the k loop and
      //  spilled across it)
      asm volatile("" : "+s"(next));
      if (next >= 0) {
        set_tile(next);
        gload(0);
        more = true;
      }
    }
    const float* As = lds + buf * (BM + BN) * GLD + (wm * 64 + r) * GLD + 4 * h;
    const float* Bs = lds + buf * (BM + BN) * GLD + BM * GLD + (wn * 64 + r) * GLD + 4 * h;
    // fragment reads run one 8-deep slab ahead of the MFMAs that consume them
    float4 a[2][2], b[2][2];
    a[0][0] = *reinterpret_cast<const float4*>(As);
    a[0][1] = *reinterpret_cast<const float4*>(As + 32 * GLD);
    b[0][0] = *reinterpret_cast<const float4*>(Bs);
    b[0][1] = *reinterpret_cast<const float4*>(Bs + 32 * GLD);
#pragma unroll
    for (int s = 0; s < GBK / 8; ++s) {
      const int cur = s & 1, nxt = cur ^ 1;
      if (s + 1 < GBK / 8) {
        a[nxt][0] = *reinterpret_cast<const float4*>(As + (s + 1) * 8);
        a[nxt][1] = *reinterpret_cast<const float4*>(As + 32 * GLD + (s + 1) * 8);
        b[nxt][0] = *reinterpret_cast<const float4*>(Bs + (s + 1) * 8);
        b[nxt][1] = *reinterpret_cast<const float4*>(Bs + 32 * GLD + (s + 1) * 8);
      }
#ifdef PDAE_NT_NO_SGB
      // keep the compiler from sinking those reads back to their first use
      __builtin_amdgcn_sched_barrier(0);
#endif
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[cur][i].x, b[cur][j].x, acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[cur][i].y, b[cur][j].y, acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[cur][i].z, b[cur][j].z, acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[cur][i].w, b[cur][j].w, acc[i][j], 0, 0, 0);
        }
#ifndef PDAE_NT_NO_SGB
      // issue order: one fragment read of the next k-group behind every four MFMAs (the reads
      // then never queue up in front of an MFMA that needs them; measured 99 -> 104 TFLOP/s in
      // tools/lab/NOTES.md), the next slab's global loads behind the first MFMAs
      if (s == 0) __builtin_amdgcn_sched_group_barrier(0x020, LA + LB, 0);
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
        if (s + 1 < GBK / 8) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
        else __builtin_amdgcn_sched_group_barrier(0x200, (LA + LB + 3) / 4, 0);   // the LDS stores of the next slab
      }
#endif
      // the next slab goes to the other LDS buffer (free since the last barrier) while this
      // slab's last MFMAs run, not after them
      if (s == GBK / 8 - 2 && more) lstore(buf ^ 1);
    }
    __syncthreads();
    buf ^= 1;
  }

  // ---- epilogue.  C/D layout of the 32x32 MFMA: column = lane & 31,
  // row = (e & 3) + 8 (e >> 2) + 4 (lane >> 5): a lane holds 16 rows of ONE column.
  float csum[2] = {0.f, 0.f}, csq[2] = {0.f, 0.f};
  // FULL = the whole tile lies inside the matrix (the only case on the step's shapes): no
  // per-element guards, one 64-bit base pointer per MFMA tile and 32-bit row offsets (the
  // guarded form spent ~6 us of VALU address arithmetic and 64 branches per tile)
  auto epilogue = [&](auto full_c) {
    constexpr bool FULL = decltype(full_c)::value;
    const unsigned ldc = (unsigned)p.ldc;
    // the lane coordinates pass through an opaque asm so that nothing of the epilogue's
    // address arithmetic is hoisted out of the persistent loop (it would be live, i.e.
    // spilled, across the whole MFMA loop: the 256x256 tile runs at the 128-VGPR limit)
    int r = r_, h = h_, wm = wm_, wn = wn_;
    asm volatile("" : "+v"(r), "+v"(h), "+v"(wm), "+v"(wn));
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int col = en0 + wn * 64 + j * 32 + r;
      const bool colok = FULL || col < N;
      const float bv = (p.bias && colok) ? p.bias[col] : 0.f;
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int rbase = em0 + wm * 64 + i * 32;  // one 32-row group per MFMA tile
        const float add = (EPI == EPI_GROUPBIAS_STATS || EPI == EPI_GROUP_SCATTER) ? 0.f : bv;
        float vmax = -__builtin_huge_valf();
        int amax = 0;
        float* cbase = (EPI != EPI_GROUPMAX) ? p.C + (size_t)(rbase + 4 * h) * ldc + col : nullptr;
        if (EPI == EPI_GROUP_SCATTER && (FULL || rbase < M))      // the 32-row MFMA tile is one group: one id
          cbase = p.C + (size_t)(p.c_groups[rbase >> 5] * 32 + 4 * h) * ldc + col;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int lr = (e & 3) + 8 * (e >> 2) + 4 * h;
          const int row = rbase + lr;
          float v = acc[i][j][e] + add;
          if ((EPI == EPI_GROUPBIAS_STATS || EPI == EPI_STATS) && (FULL || row < M)) {
            csum[j] += v;
            csq[j] += v * v;
          }
          if (EPI == EPI_GROUPMAX || EPI == EPI_STORE_GROUPMAX) {
            if (v > vmax) {  // e ascending => lr ascending within this half
              vmax = v;
              amax = lr;
            }
          }
          if (EPI != EPI_GROUPMAX && (FULL || (colok && row < M)))
            cbase[(unsigned)((e & 3) + 8 * (e >> 2)) * ldc] = v;
        }
        if (EPI == EPI_GROUPMAX || EPI == EPI_STORE_GROUPMAX) {
          // the other 16 rows of the group live in lane ^ 32
          const float ov = __shfl_xor(vmax, 32, kWave);
          const int oa = __shfl_xor(amax, 32, kWave);
          const bool take = (ov > vmax) || (ov == vmax && oa < amax);
          if (take) {
            vmax = ov;
            amax = oa;
          }
          if (h == 0 && colok && (FULL || rbase < M)) {
            p.gmax[(size_t)(rbase >> 5) * N + col] = vmax;
            p.garg[(size_t)(rbase >> 5) * N + col] = (unsigned char)amax;
          }
        }
      }
    }
  };
  if (em0 + BM <= M && en0 + BN <= N)
    epilogue(std::true_type{});
  else
    epilogue(std::false_type{});
  if (EPI == EPI_GROUPBIAS_STATS || EPI == EPI_STATS) {
    // per-tile column sums: one LDS slot per row of waves (plain stores), added in wave order,
    // then one atomic per column into the partial buffer of this block's XCD slot -- or, in
    // deterministic mode, a plain store into row (tile row) of p.stats_det
    constexpr int WM = BM / 64;
    float* red = lds + 2 * (BM + BN) * GLD;  // [WM][2][BN], behind the slab buffers (which already
                                             // hold the next tile's first slab)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      float s = csum[j] + __shfl_xor(csum[j], 32, kWave);
      float q = csq[j] + __shfl_xor(csq[j], 32, kWave);
      if (h == 0) {
        red[(wm * 2 + 0) * BN + wn * 64 + j * 32 + r] = s;
        red[(wm * 2 + 1) * BN + wn * 64 + j * 32 + r] = q;
      }
    }
    __syncthreads();
    float* dst = p.stats_det ? p.stats_det + (size_t)(em0 / BM) * 2 * N : p.stats + (size_t)(blockIdx.x & 7) * 2 * N;
    for (int c = tid; c < 2 * BN; c += NT) {
      const int half = c / BN, cc = c - half * BN;
      if (en0 + cc < N) {
        float t = red[half * BN + cc];
#pragma unroll
        for (int k = 1; k < WM; ++k) t += red[(k * 2 + half) * BN + cc];
        if (p.stats_det) dst[half * N + en0 + cc] = t;
        else atomicAdd(dst + half * N + en0 + cc, t);
      }
    }
    __syncthreads();   // red is written again by the next tile's epilogue
  }
  if (next < 0) break;
  slot += nslots;
  tile = next;
  }   // persistent tile loop
}

template <int BM, int BN, int PRO, int EPI>
static void launch_nt_cfg(NtArgs& a, hipStream_t s) {
  const int tiles_m = (a.M + BM - 1) / BM;
  a.tile_rows = tiles_m;
  a.tiles_n = (a.N + BN - 1) / BN;
  a.tiles = tiles_m * a.tiles_n;
  constexpr int NTH = (BM / 64) * (BN / 64) * 64;
  const size_t lds = (2 * (size_t)(BM + BN) * GLD + 2 * BN * (BM / 64)) * sizeof(float);
  // persistent blocks: one residency of the chip (32 CUs per XCD x blocks that fit a CU's LDS)
  const int chunk = (a.tiles + 7) / 8;
  const int per_cu = lds * 2 <= 160 * 1024 ? 2 : 1;
  const int nslots = chunk < 32 * per_cu ? chunk : 32 * per_cu;
  const int grid = 8 * nslots;
  static bool once = false;
  if (!once) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(gemm_nt_kernel<BM, BN, PRO, EPI>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    once = true;
  }
  hipLaunchKernelGGL((gemm_nt_kernel<BM, BN, PRO, EPI>), dim3(grid), dim3(NTH), lds, s, a);
}

// 256x256 tiles when they fill the chip (>= 3/4 of the 256 CUs busy in the last
// wave of blocks is not worth modelling: big problems only), else 128x128.
template <int PRO, int EPI>
static bool launch_conv3_if(NtArgs& a, hipStream_t s) {
  if (gemm_arith_rows() != PDAE_GEMM_BF16X3 || !rows3::conv3_takes(a, PRO, EPI)) return false;
  rows3::launch_conv3(a, PRO, EPI, s);
  return true;
}

template <int PRO, int EPI>
static int launch_nt(NtArgs& a, hipStream_t s) {
  if (launch_conv3_if<PRO, EPI>(a, s)) return check_launch("conv3");
  const long long big_tiles = (long long)((a.M + 255) / 256) * ((a.N + 255) / 256);
  if (big_tiles >= 512 && a.N % 256 != 0 && a.N % 384 == 0) launch_nt_cfg<128, 384, PRO, EPI>(a, s);
  else if (big_tiles >= 512) launch_nt_cfg<256, 256, PRO, EPI>(a, s);
  else launch_nt_cfg<128, 128, PRO, EPI>(a, s);
  return check_launch("gemm_nt");
}

static int check_nt(const char* who, int M, int N, int K) {
  if (M < 0 || N <= 0 || K <= 0) return bad_arg(who);
  if (K % 4 != 0) return unsupported("gemm: the reduction length must be a multiple of 4");
  // rows are addressed with 32-bit element offsets (lda, ldb <= max(K, N) here)
  if ((long long)M * (K > N ? K : N) >= (1LL << 32) || (long long)N * K >= (1LL << 32))
    return unsupported("gemm: operands of 2^32 elements or more");
  return PDAE_OK;
}

}  // namespace pdae

using namespace pdae;

// ---- fused patch-embedder layers (models/PointCAE_transformer.py:37-51) ------
extern "C" int pdae_embed_conv_groupbias_stats(int M, int N, int K, const float* X, const float* W,
                                               const float* gbias, float* Y, float* stats,
                                               pdae_stream_t stream) {
  int rc = check_nt("embed_conv_groupbias_stats: bad size", M, N, K);
  if (rc) return rc;
  if (M % 32 != 0) return bad_arg("embed_conv_groupbias_stats: M must be a multiple of 32");
  if (!stats) return bad_arg("embed_conv_groupbias_stats: null pointer");
  hipStream_t s = as_stream(stream);
  (void)hipMemsetAsync(stats, 0, sizeof(float) * 16 * (size_t)N, s);
  if (M == 0) return check_launch("embed_conv_groupbias_stats");
  if (!X || !W || !Y || !gbias) return bad_arg("embed_conv_groupbias_stats: null pointer");
  NtArgs a = {};
  a.M = M, a.N = N, a.K = K, a.A = X, a.lda = K, a.B = W, a.ldb = K, a.C = Y, a.ldc = N;
  a.gbias = gbias, a.stats = stats;
  // deterministic mode: one partial row per tile row (128-row tiles at the least), added in
  // row order into slot 0 of `stats`
  const int max_tile_rows = (M + 127) / 128;
  a.stats_det = static_cast<float*>(det_workspace(sizeof(float) * (size_t)max_tile_rows * 2 * N, &rc));
  if (rc) return rc;
  rc = launch_nt<PRO_NONE, EPI_GROUPBIAS_STATS>(a, s);
  if (rc || !a.stats_det) return rc;
  return det_reduce(s, a.tile_rows, 2 * N, a.stats_det, stats, 2 * N);
}

// The first layer of a set-abstraction level on coordinates alone (K = 4: xyz - centre and the zero pad column; sa1 of
// Point_CAE_PointNetv2: 2.1 M rows x 64 channels): 8 FLOPs per stored float, nothing for a matrix pipe to do -- the pass is
// its (M, N) store.  Thread = 4 adjacent channels of one row phase, weights in registers, y = fma(x3, w3, fma(x2, w2, fma(x1, w1, x0 w0)))
// (the k-ascending FMA chain of a CPU sgemm micro-kernel: what the reference's conv computes on the host);
// statistics as in the GEMM epilogue (float atomics into the 8 slots, or one partial row per block in deterministic mode).
constexpr int K4_ROWS = 2048;   // rows per block
__global__ __launch_bounds__(256) void conv_k4_stats_kernel(int M, int N, const float4* __restrict__ x, const float4* __restrict__ W,
                                                            float* __restrict__ y, float* __restrict__ stats,
                                                            float* __restrict__ det) {
  extern __shared__ float k4_red[];          // [phases][2][N]
  const int q = N >> 2, phases = 256 / q;
  const int cq = threadIdx.x % q, ph = threadIdx.x / q;
  const int c = cq * 4;
  float4 w[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) w[j] = W[c + j];
  float s1[4] = {0.f, 0.f, 0.f, 0.f}, s2[4] = {0.f, 0.f, 0.f, 0.f};
  const int mbeg = blockIdx.x * K4_ROWS, mend = min(M, mbeg + K4_ROWS);
  if (ph < phases) {
#pragma unroll 4
    for (int m = mbeg + ph; m < mend; m += phases) {
      const float4 xv = x[m];
      float v[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        v[j] = __builtin_fmaf(xv.w, w[j].w, __builtin_fmaf(xv.z, w[j].z, __builtin_fmaf(xv.y, w[j].y, xv.x * w[j].x)));
        s1[j] += v[j];
        s2[j] += v[j] * v[j];
      }
      *reinterpret_cast<float4*>(y + (size_t)m * N + c) = make_float4(v[0], v[1], v[2], v[3]);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      k4_red[(ph * 2 + 0) * N + c + j] = s1[j];
      k4_red[(ph * 2 + 1) * N + c + j] = s2[j];
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 2 * N; i += 256) {
    float t = 0.f;
    for (int p = 0; p < phases; ++p) t += k4_red[p * 2 * N + i];
    if (det) det[(size_t)blockIdx.x * 2 * N + i] = t;
    else atomicAdd(stats + (size_t)(blockIdx.x & 7) * 2 * N + i, t);
  }
}

// ---- one layer of a shared MLP (Conv 1x1, no bias -> BatchNorm -> ReLU; pointnet2_modules'
// SharedMLP): Y = act(X) . W^T with act = the PREVIOUS layer's BatchNorm + ReLU applied while X
// is staged (scale == null: X as is), and this layer's BatchNorm statistics from the epilogue.
extern "C" int pdae_conv_stats(int M, int N, int K, const float* X, const float* scale, const float* shift,
                               const float* W, float* Y, float* stats, pdae_stream_t stream) {
  int rc = check_nt("conv_stats: bad size", M, N, K);
  if (rc) return rc;
  if (!stats) return bad_arg("conv_stats: null pointer");
  if ((scale == nullptr) != (shift == nullptr)) return bad_arg("conv_stats: scale and shift go together");
  hipStream_t s = as_stream(stream);
  (void)hipMemsetAsync(stats, 0, sizeof(float) * 16 * (size_t)N, s);
  if (M == 0) return check_launch("conv_stats");
  if (!X || !W || !Y) return bad_arg("conv_stats: null pointer");
  if (K == 4 && !scale && N % 4 == 0 && N <= 1024 && 256 % (N / 4) == 0 && !(((uintptr_t)X | (uintptr_t)W | (uintptr_t)Y) & 15)) {
    const int blocks = (M + K4_ROWS - 1) / K4_ROWS, phases = 256 / (N / 4);
    float* det = static_cast<float*>(det_workspace(sizeof(float) * (size_t)blocks * 2 * N, &rc));
    if (rc) return rc;
    hipLaunchKernelGGL(conv_k4_stats_kernel, dim3(blocks), dim3(256), sizeof(float) * phases * 2 * N, s, M, N,
                       reinterpret_cast<const float4*>(X), reinterpret_cast<const float4*>(W), Y, stats, det);
    rc = check_launch("conv_stats");
    if (rc || !det) return rc;
    return det_reduce(s, blocks, 2 * N, det, stats, 2 * N);
  }
  NtArgs a = {};
  a.M = M, a.N = N, a.K = K, a.A = X, a.lda = K, a.B = W, a.ldb = K, a.C = Y, a.ldc = N;
  a.pro_scale = scale, a.pro_shift = shift, a.stats = stats;
  const int max_tile_rows = (M + 127) / 128;
  a.stats_det = static_cast<float*>(det_workspace(sizeof(float) * (size_t)max_tile_rows * 2 * N, &rc));
  if (rc) return rc;
  // narrow outputs (the first set-abstraction level: 64 / 128 channels): the 128-wide tile
  const bool narrow = N <= 128;
  if (scale ? launch_conv3_if<PRO_BNRELU, EPI_STATS>(a, s) : launch_conv3_if<PRO_NONE, EPI_STATS>(a, s)) {
  } else if (scale) {
    if (narrow) launch_nt_cfg<128, 128, PRO_BNRELU, EPI_STATS>(a, s);
    else launch_nt_cfg<256, 256, PRO_BNRELU, EPI_STATS>(a, s);
  } else {
    if (narrow) launch_nt_cfg<128, 128, PRO_NONE, EPI_STATS>(a, s);
    else launch_nt_cfg<256, 256, PRO_NONE, EPI_STATS>(a, s);
  }
  rc = check_launch("conv_stats");
  if (rc || !a.stats_det) return rc;
  return det_reduce(s, a.tile_rows, 2 * N, a.stats_det, stats, 2 * N);
}

extern "C" int pdae_embed_bnrelu_conv_groupmax(int M, int N, int K, const float* X,
                                               const float* scale, const float* shift,
                                               const float* W, const float* bias, float* gmax,
                                               unsigned char* garg, const int32_t* groups,
                                               pdae_stream_t stream) {
  int rc = check_nt("embed_bnrelu_conv_groupmax: bad size", M, N, K);
  if (rc) return rc;
  if (M % 32 != 0) return bad_arg("embed_bnrelu_conv_groupmax: M must be a multiple of 32");
  if (M == 0) return PDAE_OK;
  if (!X || !scale || !shift || !W || !gmax || !garg)
    return bad_arg("embed_bnrelu_conv_groupmax: null pointer");
  NtArgs a = {};
  a.M = M, a.N = N, a.K = K, a.A = X, a.lda = K, a.B = W, a.ldb = K, a.bias = bias;
  a.pro_scale = scale, a.pro_shift = shift, a.gmax = gmax, a.garg = garg, a.a_groups = groups;
  return launch_nt<PRO_BNRELU, EPI_GROUPMAX>(a, as_stream(stream));
}

// Y[c_groups[m/32]*32 + m%32, :] = X[a_groups[m/32]*32 + m%32, :] . W[N,K]^T + gbias[m/32, :] for the M rows
// (whole 32-row groups) of a compact product: gather on the way in (a_groups nullable: X is compact), one bias
// row per group (nullable), scatter on the way out.  The other rows of Y are not touched.
extern "C" int pdae_group_gemm_scatter(int M, int N, int K, const float* X, const int32_t* a_groups,
                                       const float* W, const float* gbias, float* Y, int ldy,
                                       const int32_t* c_groups, pdae_stream_t stream) {
  int rc = check_nt("group_gemm_scatter: bad size", M, N, K);
  if (rc) return rc;
  if (M % 32 != 0) return bad_arg("group_gemm_scatter: M must be a multiple of 32 (whole groups)");
  if (M == 0) return PDAE_OK;
  if (!X || !W || !Y || !c_groups || ldy < N) return bad_arg("group_gemm_scatter: null pointer / bad ldy");
  NtArgs a = {};
  a.M = M, a.N = N, a.K = K, a.A = X, a.lda = K, a.B = W, a.ldb = K, a.C = Y, a.ldc = ldy;
  a.gbias = gbias, a.a_groups = a_groups, a.c_groups = c_groups;
  if (launch_conv3_if<PRO_NONE, EPI_GROUP_SCATTER>(a, as_stream(stream))) return check_launch("group_gemm_scatter");
  // (the 256-row tile from 32 k rows on: measured on the embedder's two calls)
  if (M >= 32768 && N % 256 == 0) {
    launch_nt_cfg<256, 256, PRO_NONE, EPI_GROUP_SCATTER>(a, as_stream(stream));
    return check_launch("group_gemm_scatter");
  }
  return launch_nt<PRO_NONE, EPI_GROUP_SCATTER>(a, as_stream(stream));
}

extern "C" int pdae_embed_bnrelu_conv_store_groupmax(int M, int N, int K, const float* X,
                                                     const float* scale, const float* shift,
                                                     const float* W, const float* bias, float* Y,
                                                     float* gmax, unsigned char* garg,
                                                     pdae_stream_t stream) {
  int rc = check_nt("embed_bnrelu_conv_store_groupmax: bad size", M, N, K);
  if (rc) return rc;
  if (M % 32 != 0) return bad_arg("embed_bnrelu_conv_store_groupmax: M must be a multiple of 32");
  if (M == 0) return PDAE_OK;
  if (!X || !scale || !shift || !W || !Y || !gmax || !garg)
    return bad_arg("embed_bnrelu_conv_store_groupmax: null pointer");
  NtArgs a = {};
  a.M = M, a.N = N, a.K = K, a.A = X, a.lda = K, a.B = W, a.ldb = K, a.C = Y, a.ldc = N, a.bias = bias;
  a.pro_scale = scale, a.pro_shift = shift, a.gmax = gmax, a.garg = garg;
  return launch_nt<PRO_BNRELU, EPI_STORE_GROUPMAX>(a, as_stream(stream));
}

// embed_bnrelu_conv_store_groupmax with the groups' row sums of Y out of the same epilogue (gsum[M/32,N]); Y, gmax and garg
// are the plain entry's.  A product conv3_kernel does not take (the fp32-input arithmetic, K % 32 != 0) runs the plain entry
// and the group-sum sweep.
extern "C" int pdae_embed_bnrelu_conv_store_groupmax_sum(int M, int N, int K, const float* X, const float* scale,
                                                         const float* shift, const float* W, const float* bias, float* Y,
                                                         float* gmax, unsigned char* garg, float* gsum,
                                                         pdae_stream_t stream) {
  int rc = check_nt("embed_bnrelu_conv_store_groupmax_sum: bad size", M, N, K);
  if (rc) return rc;
  if (M % 32 != 0) return bad_arg("embed_bnrelu_conv_store_groupmax_sum: M must be a multiple of 32");
  if (M == 0) return PDAE_OK;
  if (!X || !scale || !shift || !W || !Y || !gmax || !garg || !gsum)
    return bad_arg("embed_bnrelu_conv_store_groupmax_sum: null pointer");
  NtArgs a = {};
  a.M = M, a.N = N, a.K = K, a.A = X, a.lda = K, a.B = W, a.ldb = K, a.C = Y, a.ldc = N, a.bias = bias;
  a.pro_scale = scale, a.pro_shift = shift, a.gmax = gmax, a.garg = garg, a.gsum = gsum;
  if (launch_conv3_if<PRO_BNRELU, EPI_STORE_GROUPMAX_SUM>(a, as_stream(stream)))
    return check_launch("embed_bnrelu_conv_store_groupmax_sum");
  if (N % 4 != 0) return unsupported("embed_bnrelu_conv_store_groupmax_sum: N must be a multiple of 4 on this arithmetic");
  rc = launch_nt<PRO_BNRELU, EPI_STORE_GROUPMAX>(a, as_stream(stream));
  if (rc) return rc;
  return group_sum_all(as_stream(stream), M / 32, N, Y, gsum);
}

// group_gemm_scatter with the max-pool gradient added where the rows are stored: row sarg[g][n] of destination group
// g = c_groups[m/32] receives + sgrad[g][n] (sgrad, sarg: [groups of Y][N], both or neither) -- what group_scatter_add over
// the listed groups would leave in Y (ldy == N with sgrad).  A product conv3_kernel does not take runs the two launches.
extern "C" int pdae_group_gemm_scatter_add(int M, int N, int K, const float* X, const int32_t* a_groups, const float* W,
                                           const float* gbias, float* Y, int ldy, const int32_t* c_groups,
                                           const float* sgrad, const unsigned char* sarg, pdae_stream_t stream) {
  int rc = check_nt("group_gemm_scatter_add: bad size", M, N, K);
  if (rc) return rc;
  if (M % 32 != 0) return bad_arg("group_gemm_scatter_add: M must be a multiple of 32 (whole groups)");
  if ((sgrad == nullptr) != (sarg == nullptr)) return bad_arg("group_gemm_scatter_add: sgrad and sarg go together");
  if (M == 0) return PDAE_OK;
  if (!X || !W || !Y || !c_groups || ldy < N) return bad_arg("group_gemm_scatter_add: null pointer / bad ldy");
  NtArgs a = {};
  a.M = M, a.N = N, a.K = K, a.A = X, a.lda = K, a.B = W, a.ldb = K, a.C = Y, a.ldc = ldy;
  a.gbias = gbias, a.a_groups = a_groups, a.c_groups = c_groups, a.sgrad = sgrad, a.sarg = sarg;
  if (launch_conv3_if<PRO_NONE, EPI_GROUP_SCATTER_ADD>(a, as_stream(stream))) return check_launch("group_gemm_scatter_add");
  rc = pdae_group_gemm_scatter(M, N, K, X, a_groups, W, gbias, Y, ldy, c_groups, stream);
  if (rc || !sgrad) return rc;
  return group_scatter_add_listed(as_stream(stream), M / 32, N, ldy, sgrad, sarg, c_groups, Y);
}
