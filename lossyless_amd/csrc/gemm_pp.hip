// The tower's GEMM launcher, product build: launches what the selection (gemm_plan.h: the table of kernels and shapes) answers
// for GemmKnobs{}.  No switches here -- the tools/ builds (`make ablation` / `make probes`) compile ablation/gemm_select.hip
// instead, which asks the same plan with the A/B switches of rounds 1-5 filled in and holds the alternative instantiations;
// that both give the same answers with no switch set is tests/test_host.py::test_tools_build_selects_what_the_product_selects.
#include "gemm_kernels.h"
#include "gemm_launch.h"

namespace lla {
namespace {

template <int EPI, int AMODE>
int launch_gemm(const GemmParams &p_in, hipStream_t st, Profiler *prof) {
  constexpr bool relu = EPI == EPI_RELU || EPI == EPI_ADDRELU;
  GemmParams p = p_in;
  const GemmPlan plan = plan_gemm(gemm_shape(EPI, AMODE, p), num_cus(), GemmKnobs{});
  if (plan.kernel == GK_NONE) return plan.status;
  if (!p.A || !p.W || !p.C) return LLA_EINVAL;
  p.n_store = stored_columns(p.n_store, p.N);
  ProfScope scope(prof, st, LLA_PROF_GEMM, 2.0 * p.M * p.N * p.K);
  const bool tall = plan.tile_rows == 320;
  switch (plan.kernel) {   // (a kernel this (epilogue, operand mode) pair has no instantiation of: LLA_EINVAL below)
    case GK_W8:
      if constexpr (AMODE == A_PLAIN && (EPI == EPI_F16 || EPI == EPI_QGELU)) return launch_w8(EPI, p, st);
      break;
    case GK_Q4:
      if constexpr (AMODE == A_PLAIN && EPI == EPI_RESID) return launch_q4(EPI, p, st);
      break;
    case GK_PP:
      if constexpr (!relu) {
        if (tall) gemm_pp_kernel<EPI, AMODE, 5><<<plan.grid, 512, 0, st>>>(p);
        else gemm_pp_kernel<EPI, AMODE, 4><<<plan.grid, 512, 0, st>>>(p);
        return check_launch();
      }
      break;
    case GK_PERSIST2:
      if constexpr (AMODE != A_CONV3) {
        if (tall) gemm_persistent_kernel<EPI, AMODE, 2, 64, 2, 0, 5><<<plan.grid, 512, 0, st>>>(p);
        else gemm_persistent_kernel<EPI, AMODE, 2, 64, 2, 0, 4><<<plan.grid, 512, 0, st>>>(p);
        return check_launch();
      }
      break;
    case GK_PERSIST1:
      if constexpr (!relu) {
        gemm_persistent_kernel<EPI, AMODE, 1, 64, 3, 0, 4><<<plan.grid, 512, 0, st>>>(p);
        return check_launch();
      }
      break;
    case GK_TILE256:
      gemm256_f16_kernel<EPI, AMODE><<<plan.grid, 512, 0, st>>>(p);
      return check_launch();
    case GK_TILE128:
      if constexpr (AMODE != A_CONV3) {
        gemm_f16_kernel<EPI, AMODE, true><<<plan.grid, kGemmThreads, 0, st>>>(p);
        return check_launch();
      }
      break;
    case GK_NONE: break;
  }
  return LLA_EINVAL;
}

}  // namespace

LLA_DEFINE_LAUNCH_GEMM(GemmKnobs{})

}  // namespace lla
