// launch_q4 of the tools/ builds (make ablation / make probes), compiled INSTEAD of ../gemm_q4.hip: the same gate and grid
// (../gemm_plan.h), plus the choice among the kernel's alternative instantiations (LLA_Q4_SCHED, LLA_Q4_PIPE, LLA_Q4_GROUP_M, the
// fp16-output instantiations behind LLA_GEMM_W8=0) and, under -DLLA_PROBES, the timing ablations (LLA_Q4_DBG, LLA_Q4_TRACE).
#include "../gemm_q4_kernel.h"
#include "ablation.h"

namespace lla {
namespace {

template <int EPI>
int launch_q4_epi(const GemmParams &p_in, hipStream_t st, int grid) {
  GemmParams p = p_in;
  static const int gm = [] { const char *e = lla_getenv("LLA_Q4_GROUP_M"); return e ? std::atoi(e) : 0; }();
  // (conv_h is unused by A_PLAIN GEMMs: the tile-group height rides there.  EPI_RESID_LNX: the three column tiles of a row tile
  // are consecutive logical tiles, so that they run in the same round of the persistent grid on three neighbouring workgroups
  // of one XCD and find each other's partial sums in time)
  p.conv_h = EPI == EPI_RESID_LNX ? 1 : gm;
  // LLA_Q4_SCHED: DMA schedule (q_sched): 1 = four instructions per phase (default; 905-909 TFLOP/s per layer at M = 217 600
  // against 903-906 for 0 and 2, same box)
  static const int var = [] { const char *e = lla_getenv("LLA_Q4_SCHED"); return e ? std::atoi(e) : 1; }();
#if defined(LLA_PROBES) || defined(LLA_Q4_PROBE)
  static const int dbg = [] { const char *e = lla_getenv("LLA_Q4_DBG"); return e ? std::atoi(e) : 0; }();
  if (dbg == 20) {
    static unsigned long long *const tr = [] { const char *e = lla_getenv("LLA_Q4_TRACE"); return e ? reinterpret_cast<unsigned long long *>(std::strtoull(e, nullptr, 0)) : nullptr; }();
    p.trace = tr;
  }
#define LLA_Q4_DBG_CASE(D) if (dbg == D) { gemm_q4_kernel<EPI, 1, D><<<grid, 256, 0, st>>>(p); return check_launch(); }
  LLA_Q4_DBG_CASE(1) LLA_Q4_DBG_CASE(2) LLA_Q4_DBG_CASE(3) LLA_Q4_DBG_CASE(13) LLA_Q4_DBG_CASE(4) LLA_Q4_DBG_CASE(5) LLA_Q4_DBG_CASE(9)
  LLA_Q4_DBG_CASE(30) LLA_Q4_DBG_CASE(20) LLA_Q4_DBG_CASE(8) LLA_Q4_DBG_CASE(40) LLA_Q4_DBG_CASE(41) LLA_Q4_DBG_CASE(42)
  LLA_Q4_DBG_CASE(43) LLA_Q4_DBG_CASE(44) LLA_Q4_DBG_CASE(45) LLA_Q4_DBG_CASE(46) LLA_Q4_DBG_CASE(47) LLA_Q4_DBG_CASE(48)
  LLA_Q4_DBG_CASE(49) LLA_Q4_DBG_CASE(50)
  if constexpr (EPI == EPI_RESID) { LLA_Q4_DBG_CASE(31) }
#undef LLA_Q4_DBG_CASE
#endif
  // The product library holds ONE instantiation per epilogue: DMA schedule 1.  LLA_Q4_SCHED=0|2 and the fp16 epilogues -- pipelined
  // into the K loop, LLA_Q4_PIPE=0: serial -- (A/B; same bits: tests/test_gpu_variants.py) exist in the tools/ builds only.
  static const int pipe = [] { const char *e = lla_getenv("LLA_Q4_PIPE"); return e ? std::atoi(e) : 1; }();
  if constexpr (EPI == EPI_F16 || EPI == EPI_QGELU) {
    if (pipe && var == 1) { gemm_q4_kernel<EPI, 1, 0, 1><<<grid, 256, 0, st>>>(p); return check_launch(); }
  }
  if (var == 0) gemm_q4_kernel<EPI, 0><<<grid, 256, 0, st>>>(p);
  else if (var == 2) gemm_q4_kernel<EPI, 2><<<grid, 256, 0, st>>>(p);
  else gemm_q4_kernel<EPI, 1><<<grid, 256, 0, st>>>(p);
  return check_launch();
}

}  // namespace

int launch_q4(int epi, const GemmParams &p, hipStream_t st) {
  const GemmShape s = gemm_shape(epi, A_PLAIN, p);
  if (!q4_takes(s)) return LLA_EINVAL;
  const int grid = q4_grid(s, num_cus());
  switch (epi) {
    // (round 6: in the product the large fp16-output GEMMs run on gemm_w8.hip, so the four-wave kernel's fp16 instantiations
    // exist in the tools/ builds only: LLA_GEMM_W8=0, tests/test_gpu_variants.py)
    case EPI_F16: return launch_q4_epi<EPI_F16>(p, st, grid);
    case EPI_QGELU: return launch_q4_epi<EPI_QGELU>(p, st, grid);
    case EPI_RESID: return launch_q4_epi<EPI_RESID>(p, st, grid);
    case EPI_RESID_LNX:
      if (!p.lnx_g || !p.lnx_b || !p.lnx_h || !p.lnx_part || !p.lnx_flag || !p.lnx_done) return LLA_EINVAL;
      return launch_q4_epi<EPI_RESID_LNX>(p, st, grid);
    default: return LLA_EINVAL;
  }
}

}  // namespace lla
