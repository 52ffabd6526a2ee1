// launch_w8 of the tools/ builds (make ablation / make probes / make w8variant), compiled INSTEAD of ../gemm_w8.hip: the same
// gate and grid (../gemm_plan.h), plus the timing ablations (LLA_W8_DBG) and the pipelined epilogue (LLA_W8_PIPE=1) of
// tools/w8_probe.py.
#include "../gemm_w8_kernel.h"
#include "ablation.h"

namespace lla {
namespace {

template <int EPI>
int launch_w8_epi(const GemmParams &p, hipStream_t st, int grid) {
  static const int dbg = [] { const char *e = lla_getenv("LLA_W8_DBG"); return e ? std::atoi(e) : 0; }();
#define LLA_W8_DBG_CASE(D) if (dbg == D) { gemm_w8_kernel<EPI, D><<<grid, 512, 0, st>>>(p); return check_launch(); }
  LLA_W8_DBG_CASE(1) LLA_W8_DBG_CASE(2) LLA_W8_DBG_CASE(3) LLA_W8_DBG_CASE(4) LLA_W8_DBG_CASE(5) LLA_W8_DBG_CASE(13) LLA_W8_DBG_CASE(15)
#undef LLA_W8_DBG_CASE
  static const int pipe = [] { const char *e = lla_getenv("LLA_W8_PIPE"); return e ? std::atoi(e) : 0; }();
  if (pipe) gemm_w8_kernel<EPI, 0, 1><<<grid, 512, 0, st>>>(p);
  else gemm_w8_kernel<EPI><<<grid, 512, 0, st>>>(p);
  return check_launch();
}

}  // namespace

int launch_w8(int epi, const GemmParams &p, hipStream_t st) {
  const GemmShape s = gemm_shape(epi, A_PLAIN, p);
  if (!w8_takes(s)) return LLA_EINVAL;
  const int grid = w8_grid(s, num_cus());
  return epi == EPI_F16 ? launch_w8_epi<EPI_F16>(p, st, grid) : launch_w8_epi<EPI_QGELU>(p, st, grid);
}

}  // namespace lla
