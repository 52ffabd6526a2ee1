// Eight-wave GEMM on v_mfma_f32_16x16x32_f16 (gemm_w8_kernel.h): the product's launcher.  Takes the tower's large fp16-output
// layers (QKV, c_fc + QuickGELU) at every M; one instantiation per epilogue, serial epilogue, no switch; which shapes it takes
// and its grid: gemm_plan.h.  (The tools/ builds compile ablation/gemm_w8_select.hip instead.)
#include "gemm_w8_kernel.h"

namespace lla {

int launch_w8(int epi, const GemmParams &p, hipStream_t st) {
  const GemmShape s = gemm_shape(epi, A_PLAIN, p);
  if (!w8_takes(s)) return LLA_EINVAL;
  const int grid = w8_grid(s, num_cus());
  if (epi == EPI_F16) gemm_w8_kernel<EPI_F16><<<grid, 512, 0, st>>>(p);
  else gemm_w8_kernel<EPI_QGELU><<<grid, 512, 0, st>>>(p);
  return check_launch();
}

}  // namespace lla
