// rows3_wgrad.hip -- the grouped weight gradients on exact-split bf16 (rows3_kernel.h wgrad3b_kernel)
#include "rows3_kernel.h"

namespace pdae {
namespace rows3 {

// The row-staged kernel (wgrad3t_kernel: 16-byte row loads, transposed fragment reads) takes every group whose widths are
// multiples of 8 and whose operands are 16-byte aligned -- every weight gradient of the shipped models; the others take
// the column-patch kernel (wgrad3b_kernel).
static bool row_staged_ok(const rows::WgradArgs& g) {
  for (int i = 0; i < g.nprob; ++i) {
    const rows::WgradProb& p = g.p[i];
    if (p.N % 8 || p.K % 8 || ((uintptr_t)p.dY & 15) || ((uintptr_t)p.X & 15)) return false;
  }
  if (g.scale && (((uintptr_t)g.scale & 15) || ((uintptr_t)g.shift & 15))) return false;
  return true;
}

template <bool FORMS>
static void wgrad3_launch(const rows::WgradArgs& g, int pl, hipStream_t s) {
  using namespace rows;
  constexpr int TN = 128;
  constexpr int PARTS1 = WTM * TN / 4 / (256 * wru(1));
  constexpr int PARTSL = WTM * TN / 4 / 256;
  if (row_staged_ok(g)) {
    const size_t lds = (size_t)2 * 3 * 2 * 32 * 256;
    auto k = wgrad3t_kernel<FORMS>;
    static bool once = false;
    if (!once) {
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      once = true;
    }
    hipLaunchKernelGGL(k, dim3(g.blocks), dim3(512), lds, s, g);
  } else {
    const size_t lds = (size_t)2 * 3 * (WTM + TN) * 80;
    auto k = wgrad3b_kernel<FORMS>;
    static bool once = false;
    if (!once) {
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      once = true;
    }
    hipLaunchKernelGGL(k, dim3(g.blocks), dim3(512), lds, s, g);
  }
  if (g.direct) return;                              // whole tiles stored by their blocks: nothing to reduce
  if (pl == 1) hipLaunchKernelGGL((wgrad_reduce_kernel<1, TN>), dim3(g.tiles * PARTS1), dim3(256), 0, s, g);
  else if (pl == 4) hipLaunchKernelGGL((wgrad_reduce_kernel<4, TN>), dim3(g.tiles * PARTSL * 4), dim3(256), 0, s, g);
  else hipLaunchKernelGGL((wgrad_reduce_kernel<8, TN>), dim3(g.tiles * PARTSL * 8), dim3(256), 0, s, g);
}

void launch_wgrad3(const rows::WgradArgs& g, int tn, int pl, hipStream_t s) {
  (void)tn;                                             // (one tile width: 128)
  if (g.a_groups || g.b_groups || g.scale) wgrad3_launch<true>(g, pl, s);
  else wgrad3_launch<false>(g, pl, s);
}

}  // namespace rows3
}  // namespace pdae
