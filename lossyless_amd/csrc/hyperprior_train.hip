// Training passes of the scale-hyperprior rate estimator (HRateHyperprior with a frozen encoder) that are not GEMMs, on gfx950.
//
// Stands in for what autograd runs for lossyless/rates.py:631-678 in training mode around the two MLPs (which run on
// lla_gemm_f32 / _tn / _nn): the side information's EntropyBottleneck with an input gradient, compressai 1.1.5's
// GaussianConditional likelihood with its two LowerBounds, the lossy_Z distortion with p_norm 1 and the affine's gradient.
// include/lossyless_amd.h states the mathematics and the buffer layouts; HyperpriorFit (hyperprior_fit.py) drives the kernels
// and carries the float64 twin of every formula here.
//
//   lla_eb_side_pass          s_hat = x + u, sum rate_s, scale d rate_s / dx and scale d rate_s / d(the 58 S numbers):
//                             side_pass_kernel (forward + backward) then side_finish_kernel
//   (lla_eb_aux_grad_any, the side bottleneck's auxiliary loss, is in eb_train.hip next to eb_aux_kernel)
//   lla_gaussian_train_pass   y, sum dist, sum rate_z, scale d rate_z / d(scales | means | y), d dist / d scaling:
//                             gaussian_pass_kernel then gaussian_finish_kernel; with gp == NULL the prologue alone (y)
//   lla_affine_grad           the gradients of scaling and biasing from d loss / d y: affine_pass_kernel, affine_finish_kernel
//
// Arrangement of all three passes, as eb_pass_kernel: a LANE owns a channel, a wave owns 64 adjacent channels (a row's loads
// and stores are contiguous lines), one wave per workgroup; walker w of W walks the rows w, w + W, ...; nothing crosses lanes.
// Lanes beyond the width own the pad columns of the outputs and store zeros there.  A walker's sums are fp32 and go to the
// workspace; the finish kernels add the walkers of every (quantity, channel) in walker order in double and round once, and
// their last workgroup adds the channels' scalar sums in a fixed order in double.  W is a function of (B, width) alone
// (eb_walkers).  No atomics; LDS only in the finish kernels.
//
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): DESIGN.md 5.20.
#include "eb_net.h"

namespace lla {
namespace {

constexpr int kSidePart = 59;                // partial sums a side walker stores per channel: 58 gradients, the rate
constexpr int kGaussPart = 3;                // ... a Gaussian walker: d dist / d scaling, dist, rate
constexpr float kInvSqrt2 = 0.70710678118654752440f, kInvSqrt2Pi = 0.39894228040143267794f;

struct Pass {
  uint32_t k0, k1, step;
  int B, C, W;
  float scale;
};

// ------------------------------------------------------------------------------------------------------------- side pass
__global__ __launch_bounds__(64) void side_pass_kernel(const float *__restrict__ x, int ldx, const float *__restrict__ params,
                                                       float *__restrict__ s_hat, int lds, float *__restrict__ dx, int ldd,
                                                       float *__restrict__ part, Pass f) {
  const int c = blockIdx.x * kWave + threadIdx.x, w = blockIdx.y;
  if (c >= f.C) {                            // a pad column of either output, or nothing
    for (int i = w; i < f.B; i += f.W) {
      if (c < lds) s_hat[(size_t)i * lds + c] = 0.f;
      if (c < ldd) dx[(size_t)i * ldd + c] = 0.f;
    }
    return;
  }
  EbNet n;
  eb_load(n, params, f.C, c);
  EbAcc acc;
  eb_acc_zero(acc);
  float sum_rate = 0.f;
  float xn = w < f.B ? x[(size_t)w * ldx + c] : 0.f;
  for (int i = w; i < f.B; i += f.W) {
    const float xi = xn;
    if (i + f.W < f.B) xn = x[(size_t)(i + f.W) * ldx + c];
    const float u = noise_at((uint64_t)i * (uint64_t)f.C + (uint64_t)c, f.step, kSideTag, f.k0, f.k1);
    const float v = xi + u;
    s_hat[(size_t)i * lds + c] = v;
    dx[(size_t)i * ldd + c] = f.scale * eb_lik_step(n, v, acc, sum_rate);
  }
  float *out = part + (size_t)w * kSidePart * f.C + c;
  eb_store_grads(n, acc, params, f.C, c, out, 0);
  out[(size_t)kNet * f.C] = sum_rate;
}

// grads [58 S]: scale times the double sum of the element's W partials, rounded once.  The last workgroup: sum rate
// (channel_totals and walker_sum: eb_net.h).
__global__ __launch_bounds__(256) void side_finish_kernel(const float *__restrict__ part, float *__restrict__ grads,
                                                          double *__restrict__ out_sum, int C, int W, float scale) {
  __shared__ double red[1][256];
  const size_t slab = (size_t)kSidePart * C;
  if (blockIdx.x + 1 == gridDim.x) {
    channel_totals<1>(part, slab, kNet, C, W, out_sum, red);
    return;
  }
  const size_t at = (size_t)blockIdx.x * 256 + threadIdx.x;      // element of [58][S]: the partial rows have the same order
  if (at >= (size_t)kNet * C) return;
  grads[at] = (float)((double)scale * walker_sum(part, slab, at, W));
}

// --------------------------------------------------------------------------------------------------------- Gaussian pass
// Phi(a) = 0.5 erfc(-a / sqrt 2) (compressai's _standardized_cumulative) and phi(a) = exp(-a^2 / 2) / sqrt(2 pi)
__device__ __forceinline__ float std_cumulative(float a) { return 0.5f * erfcf(-kInvSqrt2 * a); }
__device__ __forceinline__ float std_density(float a) { return expf(-0.5f * (a * a)) * kInvSqrt2Pi; }

// FULL = false: the prologue, y and its pad columns alone.
template <typename T, bool FULL>
__global__ __launch_bounds__(64) void gaussian_pass_kernel(const void *__restrict__ z, size_t ldz,
                                                           const float *__restrict__ scaling, const float *__restrict__ biasing,
                                                           const float *__restrict__ gp, int ldg, float bound,
                                                           float *__restrict__ dgp, float *__restrict__ y, int ldy,
                                                           float *__restrict__ dy, float *__restrict__ part, Pass f) {
  const int c = blockIdx.x * kWave + threadIdx.x, w = blockIdx.y;
  if (c >= f.C) {                            // pad columns: c of y and dy, C + c (= 2C + (c - C)) of dgp
    for (int i = w; i < f.B; i += f.W) {
      if (c < ldy) {
        y[(size_t)i * ldy + c] = 0.f;
        if (FULL) dy[(size_t)i * ldy + c] = 0.f;
      }
      if (FULL && f.C + c < ldg) dgp[(size_t)i * ldg + f.C + c] = 0.f;
    }
    return;
  }
  const float s = scaling[c], bz = biasing[c];
  const float es = expf(s), ems = expf(-s);
  float g_dist_s = 0.f, sum_dist = 0.f, sum_rate = 0.f;
  float zn = w < f.B ? load_z<T>(z, (size_t)w * ldz + c) : 0.f;
  for (int i = w; i < f.B; i += f.W) {
    const float zi = zn;
    if (i + f.W < f.B) zn = load_z<T>(z, (size_t)(i + f.W) * ldz + c);
    const float yi = (zi + bz) * es;
    y[(size_t)i * ldy + c] = yi;
    if (!FULL) continue;
    const float sraw = gp[(size_t)i * ldg + c], mu = gp[(size_t)i * ldg + f.C + c];
    const float u = noise_at((uint64_t)i * (uint64_t)f.C + (uint64_t)c, f.step, kNoiseTag, f.k0, f.k1);
    const float v = yi + u;
    const float d = v - mu, t = fabsf(d);
    const float sc = fmaxf(sraw, bound);
    const float au = (0.5f - t) / sc, al = (-0.5f - t) / sc;
    const float lik = fmaxf(std_cumulative(au) - std_cumulative(al), kLikBound);
    sum_rate += -logf(lik);
    // d(-log lik) / d lik = -1 / lik passes the likelihood's bound (header); the scale's bound blocks a gradient that would
    // lower a scale already below it
    const float g = -1.f / lik;
    const float pu = std_density(au), pl = std_density(al);
    const float g_t = g * (-(pu - pl) / sc);
    const float g_sc = g * (-(au * pu - al * pl) / sc);
    const float sg = sign_f(d);
    dgp[(size_t)i * ldg + c] = (sraw >= bound || g_sc < 0.f) ? f.scale * g_sc : 0.f;
    dgp[(size_t)i * ldg + f.C + c] = f.scale * (g_t * -sg);
    dy[(size_t)i * ldy + c] = f.scale * (g_t * sg);
    const float r = u * ems, dd = r + 1e-6f;
    sum_dist += fabsf(dd);
    g_dist_s += -sign_f(dd) * r;
  }
  if (!FULL) return;
  float *out = part + (size_t)w * kGaussPart * f.C + c;
  out[0] = g_dist_s;
  out[(size_t)1 * f.C] = sum_dist;
  out[(size_t)2 * f.C] = sum_rate;
}

// g_dist [C]: the double sum of the channel's W partials, rounded once.  The last workgroup: sum dist, sum rate_z.
__global__ __launch_bounds__(256) void gaussian_finish_kernel(const float *__restrict__ part, float *__restrict__ g_dist,
                                                              double *__restrict__ out_sums, int C, int W) {
  __shared__ double red[2][256];
  const size_t slab = (size_t)kGaussPart * C;
  if (blockIdx.x + 1 == gridDim.x) {
    channel_totals<2>(part, slab, 1, C, W, out_sums, red);
    return;
  }
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  g_dist[c] = (float)walker_sum(part, slab, c, W);
}

// ----------------------------------------------------------------------------------------------------------- affine grad
__global__ __launch_bounds__(64) void affine_pass_kernel(const float *__restrict__ dy, int ld, const float *__restrict__ y, int ldy,
                                                         float *__restrict__ part, int B, int C, int W) {
  const int c = blockIdx.x * kWave + threadIdx.x, w = blockIdx.y;
  if (c >= C) return;
  float gs = 0.f, gb = 0.f;
  for (int i = w; i < B; i += W) {
    const float g = dy[(size_t)i * ld + c];
    gs += g * y[(size_t)i * ldy + c];
    gb += g;
  }
  part[(size_t)w * 2 * C + c] = gs;
  part[(size_t)w * 2 * C + C + c] = gb;
}

__global__ __launch_bounds__(256) void affine_finish_kernel(const float *__restrict__ part, const float *__restrict__ scaling,
                                                            const float *__restrict__ add, float add_scale,
                                                            float *__restrict__ g_scaling, float *__restrict__ g_biasing, int C,
                                                            int W) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  // walker_sum's loop, for two sums in ONE walk: a walk waits for each walker's load in turn, and two walks would wait twice
  double gs = 0.0, gb = 0.0;
  for (int w = 0; w < W; ++w) {
    gs += (double)part[(size_t)w * 2 * C + c];
    gb += (double)part[(size_t)w * 2 * C + C + c];
  }
  if (add) gs += (double)add_scale * (double)add[c];
  g_scaling[c] = (float)gs;
  g_biasing[c] = (float)((double)expf(scaling[c]) * gb);
}

bool width_ok(int B, int C) { return B >= 0 && C > 0 && C <= kMaxWidth; }
bool pitch_ok(int ld, int C) { return ld >= C && ld <= 2 * kMaxWidth; }

}  // namespace
}  // namespace lla

using namespace lla;

extern "C" size_t lla_eb_side_pass_workspace_bytes(int B, int S) {
  if (!width_ok(B, S) || B == 0) return 0;
  return (size_t)eb_walkers(B, S) * kSidePart * (size_t)S * sizeof(float);
}

extern "C" int lla_eb_side_pass(const float *x, int ldx, int B, int S, const float *params, uint64_t seed, uint32_t step,
                                float scale, float *s_hat, int lds, float *dx, int ldd, float *grads, double *out_sum,
                                void *workspace, void *stream) {
  if (!width_ok(B, S) || !pitch_ok(ldx, S) || !pitch_ok(lds, S) || !pitch_ok(ldd, S)) return LLA_EINVAL;
  if (B == 0) return LLA_OK;
  if (!x || !params || !s_hat || !dx || !grads || !out_sum || !workspace) return LLA_EINVAL;
  if (((uintptr_t)x & 3) || ((uintptr_t)s_hat & 3) || ((uintptr_t)dx & 3) || !aligned16(params) || !aligned16(grads) ||
      !aligned16(workspace) || ((uintptr_t)out_sum & 7))
    return LLA_EINVAL;
  const int W = eb_walkers(B, S);
  const Pass f = {(uint32_t)seed, (uint32_t)(seed >> 32), step, B, S, W, scale};
  const int lanes = lds > ldd ? lds : ldd;
  hipStream_t st = as_stream(stream);
  float *part = static_cast<float *>(workspace);
  side_pass_kernel<<<dim3((lanes + kWave - 1) / kWave, W), kWave, 0, st>>>(x, ldx, params, s_hat, lds, dx, ldd, part, f);
  int rc = check_launch();
  if (rc != LLA_OK) return rc;
  const int blocks = (int)(((size_t)kNet * S + 255) / 256) + 1;
  side_finish_kernel<<<blocks, 256, 0, st>>>(part, grads, out_sum, S, W, scale);
  return check_launch();
}

extern "C" size_t lla_gaussian_train_pass_workspace_bytes(int B, int C) {
  if (!width_ok(B, C) || B == 0) return 0;
  return (size_t)eb_walkers(B, C) * kGaussPart * (size_t)C * sizeof(float);
}

extern "C" int lla_gaussian_train_pass(const void *z, int z_dtype, size_t ldz, int B, int C, const float *scaling,
                                       const float *biasing, const float *gp, int ldg, float scale_bound, uint64_t seed,
                                       uint32_t step, float scale, float *dgp, float *y, int ldy, float *dy, float *g_dist,
                                       double *out_sums, void *workspace, void *stream) {
  if (!width_ok(B, C) || (z_dtype != LLA_Z_F16 && z_dtype != LLA_Z_F32) || ldz < (size_t)C || !pitch_ok(ldy, C)) return LLA_EINVAL;
  const bool full = gp != nullptr;
  if (full && (ldg < 2 * C || ldg > 4 * kMaxWidth || !(scale_bound > 0.f))) return LLA_EINVAL;
  if (B == 0) return LLA_OK;
  if (!z || !scaling || !biasing || !y) return LLA_EINVAL;
  if (full && (!dgp || !dy || !g_dist || !out_sums || !workspace)) return LLA_EINVAL;
  const size_t zb = z_dtype == LLA_Z_F16 ? 2 : 4;
  if (((uintptr_t)z & (zb - 1)) || !aligned16(scaling) || !aligned16(biasing) || ((uintptr_t)y & 3)) return LLA_EINVAL;
  if (full && (((uintptr_t)gp & 3) || ((uintptr_t)dgp & 3) || ((uintptr_t)dy & 3) || !aligned16(g_dist) || !aligned16(workspace) ||
               ((uintptr_t)out_sums & 7)))
    return LLA_EINVAL;
  const int W = eb_walkers(B, C);
  const Pass f = {(uint32_t)seed, (uint32_t)(seed >> 32), step, B, C, W, scale};
  int lanes = ldy;
  if (full && ldg - C > lanes) lanes = ldg - C;
  const dim3 grid((lanes + kWave - 1) / kWave, W);
  hipStream_t st = as_stream(stream);
  float *part = static_cast<float *>(workspace);
  const bool half = z_dtype == LLA_Z_F16;
  if (!full) {
    if (half)
      gaussian_pass_kernel<_Float16, false><<<grid, kWave, 0, st>>>(z, ldz, scaling, biasing, gp, ldg, scale_bound, dgp, y, ldy, dy, part, f);
    else
      gaussian_pass_kernel<float, false><<<grid, kWave, 0, st>>>(z, ldz, scaling, biasing, gp, ldg, scale_bound, dgp, y, ldy, dy, part, f);
    return check_launch();
  }
  if (half)
    gaussian_pass_kernel<_Float16, true><<<grid, kWave, 0, st>>>(z, ldz, scaling, biasing, gp, ldg, scale_bound, dgp, y, ldy, dy, part, f);
  else
    gaussian_pass_kernel<float, true><<<grid, kWave, 0, st>>>(z, ldz, scaling, biasing, gp, ldg, scale_bound, dgp, y, ldy, dy, part, f);
  int rc = check_launch();
  if (rc != LLA_OK) return rc;
  gaussian_finish_kernel<<<(C + 255) / 256 + 1, 256, 0, st>>>(part, g_dist, out_sums, C, W);
  return check_launch();
}

extern "C" size_t lla_affine_grad_workspace_bytes(int B, int C) {
  if (!width_ok(B, C) || B == 0) return 0;
  return (size_t)eb_walkers(B, C) * 2 * (size_t)C * sizeof(float);
}

extern "C" int lla_affine_grad(const float *dy_total, int ld, const float *y, int ldy, const float *scaling, int B, int C,
                               const float *add_scaling, float add_scale, float *g_scaling, float *g_biasing, void *workspace,
                               void *stream) {
  if (!width_ok(B, C) || !pitch_ok(ld, C) || !pitch_ok(ldy, C)) return LLA_EINVAL;
  if (B == 0) return LLA_OK;
  if (!dy_total || !y || !scaling || !g_scaling || !g_biasing || !workspace) return LLA_EINVAL;
  if (((uintptr_t)dy_total & 3) || ((uintptr_t)y & 3) || !aligned16(scaling) || !aligned16(g_scaling) || !aligned16(g_biasing) ||
      (add_scaling && !aligned16(add_scaling)) || !aligned16(workspace))
    return LLA_EINVAL;
  const int W = eb_walkers(B, C);
  hipStream_t st = as_stream(stream);
  float *part = static_cast<float *>(workspace);
  affine_pass_kernel<<<dim3((C + kWave - 1) / kWave, W), kWave, 0, st>>>(dy_total, ld, y, ldy, part, B, C, W);
  int rc = check_launch();
  if (rc != LLA_OK) return rc;
  affine_finish_kernel<<<(C + 255) / 256, 256, 0, st>>>(part, scaling, add_scaling, add_scale, g_scaling, g_biasing, C, W);
  return check_launch();
}
