// Training pass of the factorized rate estimator (HRateFactorizedPrior with a frozen encoder), forward and backward, on gfx950.
//
// Stands in for what autograd runs for lossyless/rates.py:534-554 in training mode (compressai 1.1.5 EntropyBottleneck with
// uniform noise in place of rounding, filters (3, 3, 3, 3)) plus the lossy_Z distortion with p_norm 1
// (lossyless/distortions.py:408-449) over a matrix of frozen features.  include/lossyless_amd.h states the mathematics and
// the buffer layouts; BottleneckFit (bottleneck_fit.py) drives the kernels and carries the float64 twin of every formula here.
//
//   lla_eb_train_pass   sum_i dist_i, sum_i rate_i and their gradients with respect to scaling, biasing and the 58 numbers of
//                       each channel's cumulative network: eb_pass_kernel (forward + backward) then eb_pass_finish_kernel
//   lla_eb_aux_grad     the auxiliary (quantile) loss and its gradient with respect to the quantiles: eb_aux_kernel
//   lla_eb_aux_grad_any the same for any channel count (the hyperprior's side bottleneck); one checked function, eb_aux_grad
//
// Arrangement of the pass: a LANE owns a channel, a wave owns 64 adjacent channels (a row's load is one contiguous line of 256
// or 128 bytes), one wave per workgroup.  Walker w of W walks the rows w, w + W, ...  The channel's parameters -- as the network
// uses them: softplus(matrix), bias, tanh(factor) -- and the 63 accumulators (58 network gradients, d rate / d scaling,
// d rate / d biasing, d dist / d scaling, the channel's dist and rate sums) stay in registers for the whole walk; nothing crosses
// lanes.  The chain rule through softplus and tanh of the parameters is applied once, after the walk.  Each walker stores its
// 63 partial sums; the finish kernel adds the walkers of every (quantity, channel) in walker order in double and rounds once, and
// its last workgroup adds the channels' dist and rate sums in a fixed order in double.  W is a function of (B, C) alone
// (eb_walkers), so the same inputs give the same bits.  No atomics, no LDS in the pass kernel.
//
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): DESIGN.md 5.19 records the register, scratch and occupancy
// figures of the three kernels.  The channel network's device functions, the noise stream (noise_at), the walk's shared parts
// (eb_acc_zero, eb_lik_step, eb_store_grads) and the finish kernels' sums (walker_sum, channel_totals) live in eb_net.h, which
// hyperprior_train.hip shares; eb_aux_kernel and both of its entry points are here.
#include "eb_net.h"

namespace lla {
namespace {

constexpr int kMain = 60;                    // ... of the main optimiser's buffer per channel: scaling, biasing, the network
constexpr int kPart = 63;                    // partial sums a walker stores per channel

struct EbPass {
  uint32_t k0, k1, step;
  int B, C, W;
};

template <typename T>
__global__ __launch_bounds__(64) void eb_pass_kernel(const void *__restrict__ z, size_t ldz, const float *__restrict__ params,
                                                     const float *__restrict__ scaling, const float *__restrict__ biasing,
                                                     float *__restrict__ part, EbPass f) {
  const int c = blockIdx.x * kWave + threadIdx.x, w = blockIdx.y;
  if (c >= f.C) return;                      // (nothing crosses lanes: a lane beyond C has no part in the walk)
  EbNet n;
  eb_load(n, params, f.C, c);
  const float s = scaling[c], bz = biasing[c];
  const float es = expf(s), ems = expf(-s);
  EbAcc acc;
  eb_acc_zero(acc);
  float g_rate_s = 0.f, g_rate_b = 0.f, g_dist_s = 0.f, sum_dist = 0.f, sum_rate = 0.f;
  float zn = w < f.B ? load_z<T>(z, (size_t)w * ldz + c) : 0.f;
  for (int i = w; i < f.B; i += f.W) {
    const float zi = zn;
    if (i + f.W < f.B) zn = load_z<T>(z, (size_t)(i + f.W) * ldz + c);   // the next row's load flies over this row's arithmetic
    const float u = noise_at((uint64_t)i * (uint64_t)f.C + (uint64_t)c, f.step, kNoiseTag, f.k0, f.k1);
    const float y = (zi + bz) * es;
    const float dv = eb_lik_step(n, y + u, acc, sum_rate);
    g_rate_s += dv * y;
    g_rate_b += dv * es;
    // dist: z_hat - z = u exp(-s) (closed form of the header), + the 1e-6 of nn.PairwiseDistance
    const float r = u * ems, d = r + 1e-6f;
    sum_dist += fabsf(d);
    g_dist_s += -sign_f(d) * r;
  }
  float *out = part + (size_t)w * kPart * f.C + c;
  out[0] = g_dist_s;
  out[(size_t)1 * f.C] = g_rate_s;
  out[(size_t)2 * f.C] = g_rate_b;
  eb_store_grads(n, acc, params, f.C, c, out, 3);
  out[(size_t)61 * f.C] = sum_dist;
  out[(size_t)62 * f.C] = sum_rate;
}

// grads[0][..] (dist) and grads[1][..] (rate), each 60 C: every element the sum of its W partials in walker order, in double,
// rounded once (the dist half is zero outside scaling).  The LAST workgroup adds the channels' dist and rate sums instead
// (channel_totals, eb_net.h).
__global__ __launch_bounds__(256) void eb_pass_finish_kernel(const float *__restrict__ part, float *__restrict__ grads,
                                                             double *__restrict__ out_sums, int C, int W) {
  __shared__ double red[2][256];
  const size_t slab = (size_t)kPart * C;
  if (blockIdx.x + 1 == gridDim.x) {
    channel_totals<2>(part, slab, 61, C, W, out_sums, red);
    return;
  }
  const size_t at = (size_t)blockIdx.x * 256 + threadIdx.x;      // element of the main layout: [60][C]
  if (at >= (size_t)kMain * C) return;
  const int k = (int)(at / C), c = (int)(at % C);
  // main layout row k: 0 scaling, 1 biasing, 2 + j network -> partial rows: rate (1, 2, 3 + j), dist (0 for scaling)
  const int rate_row = k == 0 ? 1 : k == 1 ? 2 : k + 1;
  grads[at] = k == 0 ? (float)walker_sum(part, slab, c, W) : 0.f;
  grads[(size_t)kMain * C + at] = (float)walker_sum(part, slab, (size_t)rate_row * C + c, W);
}

// aux = sum_c sum_k |L_c(q_c[k]) - target[k]| and d aux / d q_c[k] = sign(.) dL_c/dx (q_c[k]), the network held constant.
// ONE workgroup of 512 threads; a thread owns the channels t, t + 512, ...  The channels' losses are added in channel
// order in double: runs of 8 adjacent channels by the lanes of the first wave, then the 64 runs in order by lane 0, chunk
// of 512 channels after chunk.  Any C >= 1.
__global__ __launch_bounds__(512) void eb_aux_kernel(const float *__restrict__ params, const float *__restrict__ quantiles,
                                                      const float *__restrict__ target, float *__restrict__ grad_q,
                                                      double *__restrict__ out_loss, int C) {
  __shared__ double loss[512];
  __shared__ double runs[64];
  double total = 0.0;
  const float tg[3] = {target[0], target[1], target[2]};
  for (int c0 = 0; c0 < C; c0 += 512) {
    const int c = c0 + threadIdx.x;
    double mine = 0.0;
    if (c < C) {
      EbNet n;
      eb_load(n, params, C, c);
      EbAcc none;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        EbAct a;
        const float r = eb_forward(n, quantiles[(size_t)3 * c + k], a) - tg[k];
        const float sg = sign_f(r);
        grad_q[(size_t)3 * c + k] = sg == 0.f ? 0.f : sg * eb_backward<false>(n, a, 1.f, none);
        mine += (double)fabsf(r);
      }
    }
    loss[threadIdx.x] = mine;
    __syncthreads();
    if (threadIdx.x < 64) {
      double run = 0.0;
      for (int j = 0; j < 8; ++j) run += loss[8 * threadIdx.x + j];
      runs[threadIdx.x] = run;
    }
    __syncthreads();
    if (threadIdx.x == 0)
      for (int j = 0; j < 64; ++j) total += runs[j];
    __syncthreads();
  }
  if (threadIdx.x == 0) *out_loss = total;
}

bool eb_shape_ok(int B, int C) { return B >= 0 && C > 0 && !(C & 3) && C <= kMaxWidth; }

// what lla_eb_aux_grad and lla_eb_aux_grad_any share: every refusal but the first's C % 4, and the launch
int eb_aux_grad(const float *params, const float *quantiles, const float *target, int C, float *grad_q, double *out_loss,
                void *stream) {
  if (C <= 0 || C > kMaxWidth) return LLA_EINVAL;
  if (!params || !quantiles || !target || !grad_q || !out_loss) return LLA_EINVAL;
  if (!aligned16(params) || !aligned16(quantiles) || !aligned16(grad_q) || ((uintptr_t)target & 3) || ((uintptr_t)out_loss & 7))
    return LLA_EINVAL;
  eb_aux_kernel<<<1, 512, 0, as_stream(stream)>>>(params, quantiles, target, grad_q, out_loss, C);
  return check_launch();
}

}  // namespace
}  // namespace lla

using namespace lla;

extern "C" size_t lla_eb_train_pass_workspace_bytes(int B, int C) {
  if (!eb_shape_ok(B, C) || B == 0) return 0;
  return (size_t)eb_walkers(B, C) * kPart * (size_t)C * sizeof(float);
}

extern "C" int lla_eb_train_pass(const void *z, int z_dtype, size_t ldz, int B, int C, const float *params,
                                 const float *scaling, const float *biasing, uint64_t seed, uint32_t step, float *grads,
                                 double *out_sums, void *workspace, void *stream) {
  if (!eb_shape_ok(B, C) || (z_dtype != LLA_Z_F16 && z_dtype != LLA_Z_F32) || ldz < (size_t)C) return LLA_EINVAL;
  if (B == 0) return LLA_OK;
  if (!z || !params || !scaling || !biasing || !grads || !out_sums || !workspace) return LLA_EINVAL;
  const size_t zb = z_dtype == LLA_Z_F16 ? 2 : 4;
  if (((uintptr_t)z & (zb - 1)) || !aligned16(params) || !aligned16(scaling) || !aligned16(biasing) || !aligned16(grads) ||
      !aligned16(workspace) || ((uintptr_t)out_sums & 7))
    return LLA_EINVAL;
  const int W = eb_walkers(B, C);
  const EbPass f = {(uint32_t)seed, (uint32_t)(seed >> 32), step, B, C, W};
  const dim3 grid((C + kWave - 1) / kWave, W);
  hipStream_t st = as_stream(stream);
  float *part = static_cast<float *>(workspace);
  if (z_dtype == LLA_Z_F16)
    eb_pass_kernel<_Float16><<<grid, kWave, 0, st>>>(z, ldz, params, scaling, biasing, part, f);
  else
    eb_pass_kernel<float><<<grid, kWave, 0, st>>>(z, ldz, params, scaling, biasing, part, f);
  int rc = check_launch();
  if (rc != LLA_OK) return rc;
  const int blocks = (int)(((size_t)kMain * C + 255) / 256) + 1;
  eb_pass_finish_kernel<<<blocks, 256, 0, st>>>(part, grads, out_sums, C, W);
  return check_launch();
}

extern "C" int lla_eb_aux_grad(const float *params, const float *quantiles, const float *target, int C, float *grad_q,
                               double *out_loss, void *stream) {
  if (C & 3) return LLA_EINVAL;
  return eb_aux_grad(params, quantiles, target, C, grad_q, out_loss, stream);
}

extern "C" int lla_eb_aux_grad_any(const float *params, const float *quantiles, const float *target, int S, float *grad_q,
                                   double *out_loss, void *stream) {
  return eb_aux_grad(params, quantiles, target, S, grad_q, out_loss, stream);
}
