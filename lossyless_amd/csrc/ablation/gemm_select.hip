// The tower's GEMM launcher of the tools/ builds (make ablation / make probes), compiled INSTEAD of ../gemm_pp.hip (same
// lla::launch_gemm_rt symbol); never part of liblossyless_amd.so.  It asks the product's selection (../gemm_plan.h) with the A/B
// switches of rounds 1-5 that influence the CHOICE read from the environment (LLA_GEMM_TILE, _PP, _Q4, _W8, _TALL, _BALANCED,
// _PERSIST, _KB, _WIDE_MIN_N, LLA_RN_PERSIST): with none set the knobs are GemmKnobs{}, i.e. the product
// (tests/test_host.py::test_tools_build_selects_what_the_product_selects).  What lives here is the choice among alternative
// INSTANTIATIONS of the chosen kernel (LLA_GEMM_EPILOGUE, LLA_GEMM_GLDS) and, under -DLLA_PROBES, the timing ablations and the
// retired kernels.
#include "../gemm_kernels.h"
#include "../gemm_launch.h"
#include "ablation.h"
#ifdef LLA_PROBES
#include "gemm_retired.h"
#endif

namespace lla {
namespace {

int env_int(const char *name, int dflt) { const char *e = lla_getenv(name); return e ? std::atoi(e) : dflt; }

const GemmKnobs &knobs() {   // read once per process
  static const GemmKnobs v = [] {
    GemmKnobs k;
    k.tile = env_int("LLA_GEMM_TILE", k.tile);
    k.pp = env_int("LLA_GEMM_PP", k.pp);
    k.q4 = env_int("LLA_GEMM_Q4", k.q4);
    k.w8 = env_int("LLA_GEMM_W8", LLA_W8_DEFAULT);
    k.tall = env_int("LLA_GEMM_TALL", k.tall);
    const char *b = lla_getenv("LLA_GEMM_BALANCED");
    k.balanced = !(b && b[0] == '0');
    k.persist = env_int("LLA_GEMM_PERSIST", k.persist);
    k.kb = env_int("LLA_GEMM_KB", k.kb);
    k.wide_min_n = env_int("LLA_GEMM_WIDE_MIN_N", k.wide_min_n);
    k.rn_persist = env_int("LLA_RN_PERSIST", k.rn_persist);
    return k;
  }();
  return v;
}

template <int EPI, int AMODE, int NJ, int KB, int STAGES, int NI>
int launch_persistent_cfg(const GemmParams &p, hipStream_t st, int grid) {
  // LLA_GEMM_EPILOGUE=direct: MFMA-layout stores instead of the LDS-staged line-assembling epilogue
  static const int dbg = [] {
    const char *epi = lla_getenv("LLA_GEMM_EPILOGUE");
#ifdef LLA_PROBES
    if (const char *e = lla_getenv("LLA_GEMM_DEBUG")) return std::atoi(e);
#endif
    return (epi && epi[0] == 'd') ? 4 : 0;
  }();
#ifdef LLA_PROBES
  // Ablation / trace variants (wrong-element addresses, skipped pipes, s_memtime stamps): only in
  // the -DLLA_PROBES build that tools/ load explicitly; the shipped library ignores LLA_GEMM_DEBUG.
  if (dbg == 1) { gemm_persistent_kernel<EPI, AMODE, NJ, KB, STAGES, 1, NI><<<grid, 512, 0, st>>>(p); return check_launch(); }
  if (dbg == 2) { gemm_persistent_kernel<EPI, AMODE, NJ, KB, STAGES, 2, NI><<<grid, 512, 0, st>>>(p); return check_launch(); }
#endif
  if (dbg == 4) gemm_persistent_kernel<EPI, AMODE, NJ, KB, STAGES, 4, NI><<<grid, 512, 0, st>>>(p);
  else gemm_persistent_kernel<EPI, AMODE, NJ, KB, STAGES, 0, NI><<<grid, 512, 0, st>>>(p);
  return check_launch();
}

// lock-step persistent kernel.  KB = 32 (twice the ring depth, 256-row tiles only) measured WORSE end to end (61k vs 72k
// img/s): 64-byte row segments waste half of every 128-byte line fetched when the operands are not L2-warm.
template <int EPI, int AMODE, int NJ>
int launch_persistent(const GemmParams &p, hipStream_t st, bool tall, int grid) {
  if constexpr (NJ == 2) {
    if (knobs().kb != 64) return launch_persistent_cfg<EPI, AMODE, 2, 32, 4, 4>(p, st, grid);
    if (tall) return launch_persistent_cfg<EPI, AMODE, 2, 64, 2, 5>(p, st, grid);
    return launch_persistent_cfg<EPI, AMODE, 2, 64, 2, 4>(p, st, grid);
  } else {
    if (knobs().kb != 64) return launch_persistent_cfg<EPI, AMODE, 1, 32, 5, 4>(p, st, grid);
    return launch_persistent_cfg<EPI, AMODE, 1, 64, 3, 4>(p, st, grid);
  }
}

template <int EPI, int AMODE>
int launch_pp(const GemmParams &p, hipStream_t st, bool tall, int grid) {
#ifdef LLA_PROBES
  static const int dbg = env_int("LLA_GEMM_DEBUG", 0), cap = env_int("LLA_GEMM_GRID", 0);
  if (cap > 0 && grid > cap) grid = cap;   // experiment: fewer CUs (is the epilogue bandwidth-bound?)
#define LLA_PP_DBG(CODE, D, T)                                                 \
  if (dbg == CODE) {                                                           \
    if (tall) gemm_pp_kernel<EPI, AMODE, 5, D, T><<<grid, 512, 0, st>>>(p);    \
    else gemm_pp_kernel<EPI, AMODE, 4, D, T><<<grid, 512, 0, st>>>(p);         \
    return check_launch();                                                     \
  }
  LLA_PP_DBG(1, 1, false) LLA_PP_DBG(2, 2, false) LLA_PP_DBG(4, 4, false) LLA_PP_DBG(5, 5, false)
  LLA_PP_DBG(9, 0, true) LLA_PP_DBG(11, 1, true) LLA_PP_DBG(12, 2, true) LLA_PP_DBG(14, 4, true)
#undef LLA_PP_DBG
#endif
  if constexpr (epi_base(EPI) == EPI_F16 || epi_base(EPI) == EPI_QGELU) {
    static const bool staged = [] { const char *e = lla_getenv("LLA_GEMM_EPILOGUE"); return e && e[0] == 's'; }();
    if (staged) {   // A/B: LDS-staged fp16 epilogue (bit-identical)
      if (tall) gemm_pp_kernel<EPI, AMODE, 5, 0, false, false><<<grid, 512, 0, st>>>(p);
      else gemm_pp_kernel<EPI, AMODE, 4, 0, false, false><<<grid, 512, 0, st>>>(p);
      return check_launch();
    }
  }
  if (tall) gemm_pp_kernel<EPI, AMODE, 5><<<grid, 512, 0, st>>>(p);
  else gemm_pp_kernel<EPI, AMODE, 4><<<grid, 512, 0, st>>>(p);
  return check_launch();
}

template <int EPI, int AMODE>
int launch_gemm(const GemmParams &p_in, hipStream_t st, Profiler *prof = nullptr) {
  constexpr bool relu = EPI == EPI_RELU || EPI == EPI_ADDRELU, fp16_out = EPI == EPI_F16 || EPI == EPI_QGELU;
  GemmParams p = p_in;
  // tools/gemm_trace.py: LLA_GEMM_TRACE = device address of a u64 [8][128][4] buffer (with LLA_GEMM_DEBUG=9)
  static unsigned long long *const trace = [] {
    const char *e = lla_getenv("LLA_GEMM_TRACE");
    return e ? reinterpret_cast<unsigned long long *>(std::strtoull(e, nullptr, 0)) : nullptr;
  }();
  p.trace = trace;
  const GemmPlan plan = plan_gemm(gemm_shape(EPI, AMODE, p), num_cus(), knobs());
  if (plan.kernel == GK_NONE) return plan.status;
  if (!p.A || !p.W || !p.C) return LLA_EINVAL;
  p.n_store = stored_columns(p.n_store, p.N);
  ProfScope scope(prof, st, LLA_PROF_GEMM, 2.0 * p.M * p.N * p.K);
  const bool tall = plan.tile_rows == 320;
#ifdef LLA_PROBES
  // the retired kernels, as overrides in front of the plan: where the four- / eight-wave kernels did not take a large GEMM
  if constexpr (!relu) {
    if constexpr (AMODE == A_PLAIN) {
      static const int quad = env_int("LLA_GEMM_QUAD", 0);
      if (quad && plan.kernel != GK_W8 && plan.kernel != GK_Q4 && p.M >= kBigM && p.N % 256 == 0 && p.K >= 128) return launch_quad<EPI>(p, st);
    }
    static const int duo = env_int("LLA_GEMM_DUO", 0);
    const bool persistent = plan.kernel == GK_PP || plan.kernel == GK_PERSIST2 || plan.kernel == GK_PERSIST1;
    if (duo && persistent && p.N % 256 == 0 && p.N >= kWideMinN && p.K >= kPpMinK) return launch_duo<EPI, AMODE>(p, st);
  }
#endif
  switch (plan.kernel) {   // (a kernel this (epilogue, operand mode) pair has no instantiation of: LLA_EINVAL below)
    case GK_W8:
      if constexpr (AMODE == A_PLAIN && fp16_out) return launch_w8(EPI, p, st);
      break;
    case GK_Q4:   // (fp16 outputs: LLA_GEMM_W8=0, the round-5 selection)
      if constexpr (AMODE == A_PLAIN && (fp16_out || EPI == EPI_RESID)) return launch_q4(EPI, p, st);
      break;
    case GK_PP:   // (ReLU convolutions: LLA_RN_PERSIST=3)
      if constexpr (AMODE != A_CONV3) return launch_pp<EPI, AMODE>(p, st, tall, plan.grid);
      break;
    case GK_PERSIST2:
      if constexpr (AMODE != A_CONV3) return launch_persistent<EPI, AMODE, 2>(p, st, tall, plan.grid);
      break;
    case GK_PERSIST1:
      if constexpr (AMODE != A_CONV3) return launch_persistent<EPI, AMODE, 1>(p, st, tall, plan.grid);
      break;
    case GK_TILE256:
#ifdef LLA_PROBES
      if constexpr (!relu) {
        static const int dbg = env_int("LLA_GEMM_DEBUG", 0);
        if (knobs().tile == 256 && dbg == 1) { gemm256_f16_kernel<EPI, AMODE, 1><<<plan.grid, 512, 0, st>>>(p); return check_launch(); }
        if (knobs().tile == 256 && dbg == 2) { gemm256_f16_kernel<EPI, AMODE, 2><<<plan.grid, 512, 0, st>>>(p); return check_launch(); }
      }
#endif
      gemm256_f16_kernel<EPI, AMODE><<<plan.grid, 512, 0, st>>>(p);
      return check_launch();
    case GK_TILE128:
      if constexpr (AMODE != A_CONV3) {
        if constexpr (!relu) {   // LLA_GEMM_GLDS=0: operands staged through registers (round 1)
          static const bool glds = [] { const char *e = lla_getenv("LLA_GEMM_GLDS"); return !(e && e[0] == '0'); }();
          if (!glds) { gemm_f16_kernel<EPI, AMODE, false><<<plan.grid, kGemmThreads, 0, st>>>(p); return check_launch(); }
        }
        gemm_f16_kernel<EPI, AMODE, true><<<plan.grid, kGemmThreads, 0, st>>>(p);
        return check_launch();
      }
      break;
    case GK_NONE: break;
  }
  return LLA_EINVAL;
}

}  // namespace

LLA_DEFINE_LAUNCH_GEMM(knobs())

}  // namespace lla
