// rows3_cfg.inc -- one tile shape of the exact-split row GEMM (rows3_kernel.h gemm3_kernel) with all its epilogues, both
// weight layouts, persistent and one-tile-per-block forms: included by rows3_cfg0.hip .. rows3_cfg3.hip with R3_TI,
// R3_TJ, R3_WM, R3_WN, R3_KS and R3_NAME defined (one translation unit per shape: they compile in parallel).
#include "rows3_kernel.h"

namespace pdae {
namespace rows3 {

// -> gridDim.x of the launch
template <int TI, int TJ, int WM, int WN, int KS, bool BKN, int EPI, bool PERS>
static int launch_cfg3_k(Args& a, int nslots, int splits, size_t lds, hipStream_t s) {
  auto k = gemm3_kernel<TI, TJ, WM, WN, KS, BKN, EPI, true, 0, PERS>;
  static size_t set_to = 0;                            // (EPI_BNRELU_STATS: the size depends on N)
  if (lds > set_to) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    set_to = lds;
  }
  hipLaunchKernelGGL(k, dim3(8 * nslots, splits, 1), dim3(WM * WN * 64), lds, s, a);
  return 8 * nslots;
}

// -> gridDim.x of the launch; a.tiles holds its tile count
template <int TI, int TJ, int WM, int WN, int KS, bool BKN, int EPI>
static int launch_cfg3(Args& a, int splits, int stream_blocks, hipStream_t s) {
  constexpr int BM = 32 * TI * WM, BN = 32 * TJ * WN;
  a.tiles_n = (a.N + BN - 1) / BN;
  a.tiles = ((a.M + BM - 1) / BM) * a.tiles_n;
  a.kchunk = ((a.K + splits - 1) / splits + BK3 - 1) / BK3 * BK3;
  const Cfg3 c = {TI, TJ, WM, WN, KS};
  // (EPI_BNRELU_STATS: [WM][2][BN] floats of column statistics behind the tile buffers)
  const size_t lds = lds_bytes3(c) + (EPI == rows::EPI_BNRELU_STATS ? (size_t)WM * 2 * BN * 4 + (size_t)2 * a.N * 4 : 0);
  const int chunk = (a.tiles + 7) / 8;
  (void)stream_blocks;
  a.stream_blocks = 0, a.slabs = splits;
  // persistent blocks (one residency: 32 CUs per XCD, shared by the splits) for launches of several rounds of tiles, when
  // the stream of LDS tiles keeps its parity across output tiles; else one tile per block (its own instantiation:
  // nothing of the tile loop in the k-loop)
  const int kt = a.kchunk / (16 * KS), per_xcd = 32 / splits > 0 ? 32 / splits : 1;
  if (kt % 2 == 0 && kt >= 4 && a.K % a.kchunk == 0 && chunk > per_xcd)
    return launch_cfg3_k<TI, TJ, WM, WN, KS, BKN, EPI, true>(a, per_xcd, splits, lds, s);
  return launch_cfg3_k<TI, TJ, WM, WN, KS, BKN, EPI, false>(a, chunk, splits, lds, s);
}

// -> gridDim.x of the launch, 0 when this tile shape does not carry the epilogue (nothing launched)
int R3_NAME(Args& a, bool w_kn, int epi, int splits, hipStream_t s) {
  constexpr int TI = R3_TI, TJ = R3_TJ, WM = R3_WM, WN = R3_WN, KS = R3_KS;
  if (!w_kn) {
    if (epi == rows::EPI_STORE) return launch_cfg3<TI, TJ, WM, WN, KS, false, rows::EPI_STORE>(a, splits, 0, s);
    if (epi == rows::EPI_BIAS_RELU) return launch_cfg3<TI, TJ, WM, WN, KS, false, rows::EPI_BIAS_RELU>(a, splits, 0, s);
    if (epi == rows::EPI_MUL_POS) return launch_cfg3<TI, TJ, WM, WN, KS, false, rows::EPI_MUL_POS>(a, splits, 0, s);
    return launch_cfg3<TI, TJ, WM, WN, KS, false, rows::EPI_BIAS_GELU2>(a, splits, 0, s);
  }
  if (epi == rows::EPI_STORE) return launch_cfg3<TI, TJ, WM, WN, KS, true, rows::EPI_STORE>(a, splits, 0, s);
  if (epi == rows::EPI_BNRELU_STATS) {
    if constexpr (TJ <= 2 && WM == 4 && WN == 2) return launch_cfg3<TI, TJ, WM, WN, KS, true, rows::EPI_BNRELU_STATS>(a, splits, 0, s);
    else return 0;
  }
  if (epi == rows::EPI_MUL_POS) return launch_cfg3<TI, TJ, WM, WN, KS, true, rows::EPI_MUL_POS>(a, splits, 0, s);
  return launch_cfg3<TI, TJ, WM, WN, KS, true, rows::EPI_MUL_GELUGRAD>(a, splits, 0, s);
}

}  // namespace rows3
}  // namespace pdae
