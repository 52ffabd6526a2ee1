// Four-wave GEMM (gemm_q4_kernel.h): the product's launcher.  In the product the kernel takes the tower's RESIDUAL layers
// (out-proj, c_proj; M % 256 == 0): x += A W^T + b (EPI_RESID) and the same with the LayerNorm that follows applied in the
// epilogue (EPI_RESID_LNX); the fp16-output layers run on the eight-wave kernel (gemm_w8.hip).  One instantiation per epilogue:
// DMA schedule 1, no switch; which shapes it takes and its grid: gemm_plan.h.  (The tools/ builds compile
// ablation/gemm_q4_select.hip instead.)
#include "gemm_q4_kernel.h"

namespace lla {

int launch_q4(int epi, const GemmParams &p_in, hipStream_t st) {
  const GemmShape s = gemm_shape(epi, A_PLAIN, p_in);
  if (!q4_takes(s)) return LLA_EINVAL;
  const int grid = q4_grid(s, num_cus());
  GemmParams p = p_in;
  // (conv_h is unused by A_PLAIN GEMMs: the tile-group height rides there; 0 = the kernel's default.  EPI_RESID_LNX: the three
  // column tiles of a row tile are consecutive logical tiles, so that they run in the same round of the persistent grid on
  // three neighbouring workgroups of one XCD and find each other's partial sums in time)
  p.conv_h = epi == EPI_RESID_LNX ? 1 : 0;
  switch (epi) {
    case EPI_RESID: gemm_q4_kernel<EPI_RESID, 1><<<grid, 256, 0, st>>>(p); return check_launch();
    case EPI_RESID_LNX:
      if (!p.lnx_g || !p.lnx_b || !p.lnx_h || !p.lnx_part || !p.lnx_flag || !p.lnx_done) return LLA_EINVAL;
      gemm_q4_kernel<EPI_RESID_LNX, 1><<<grid, 256, 0, st>>>(p);
      return check_launch();
    default: return LLA_EINVAL;   // (the fp16 epilogues: tools/ builds only)
  }
}

}  // namespace lla
