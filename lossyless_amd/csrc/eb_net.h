// Device functions of one channel's cumulative network (compressai 1.1.5 EntropyBottleneck, filters (3, 3, 3, 3)) and the
// Philox noise stream, shared by the training passes of the factorized model (eb_train.hip) and of the scale hyperprior
// (hyperprior_train.hip), with the per-element likelihood step of their two walks and the sums of their finish kernels.
// include/lossyless_amd.h states the mathematics; every formula here has ONE form, which the float64 twin of bottleneck_fit.py
// (twin_likelihood and what it calls) repeats line for line.
#pragma once
#include "common.h"

#include <cmath>

namespace lla {
namespace {

constexpr int kNet = 58;                     // numbers of one channel's cumulative network: 33 matrix, 13 bias, 12 factor
constexpr int kMat = 33, kBias = 13, kFac = 12;
static_assert(kMat + kBias + kFac == kNet, "layout of one channel");
constexpr int kRowsPerWalker = 8;            // rows that amortise a walker's parameter set-up
constexpr int kWaveSlots = 2048;             // 256 CUs x 4 SIMDs x 2 waves (the pass kernels' occupancy)
constexpr uint32_t kNoiseTag = 0x6e6f6973u;  // fourth counter word of the noise stream of z ("nois")
constexpr uint32_t kSideTag = 0x73696465u;   // ... of the side information's stream ("side")
constexpr float kLikBound = 1e-9f;
constexpr int kMaxWidth = 1 << 20;           // widest matrix (channels) a pass accepts

// Philox4x32-10 (Salmon et al., SC'11), as csrc/batchnorm.hip draws its dropout masks; word `pick` of the four.
__device__ __forceinline__ uint32_t philox_word(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                                int pick) {
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1, c3 = (uint32_t)p0, c0 = n0, c2 = n2;
    k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
  }
  return pick == 0 ? c0 : pick == 1 ? c1 : pick == 2 ? c2 : c3;
}

// The noise of element f = i cols + c of a [rows][cols] matrix, ANY cols: counter (f / 4 lo, f / 4 hi, step, tag), word f % 4,
// u = float(word >> 8) 2^-24 - 0.5 in [-0.5, 0.5).  Every pass draws from it; eb_pass_kernel's cols are multiples of 4, where
// the word is c % 4 (the definition of bottleneck_noise).
__device__ __forceinline__ float noise_at(uint64_t f, uint32_t step, uint32_t tag, uint32_t k0, uint32_t k1) {
  const uint64_t e = f >> 2;
  const uint32_t word = philox_word((uint32_t)e, (uint32_t)(e >> 32), step, tag, k0, k1, (int)(f & 3));
  return (float)(word >> 8) * 0x1p-24f - 0.5f;
}

// softplus(m) = max(m, 0) + log1p(exp(-|m|)) and its derivative sigmoid(m) = 1 / (1 + exp(-m)) from the same exponential
__device__ __forceinline__ float softplus_f(float m) { return fmaxf(m, 0.f) + log1pf(expf(-fabsf(m))); }
__device__ __forceinline__ float sigmoid_f(float t) {
  const float e = expf(-fabsf(t));
  return t <= 0.f ? e / (1.f + e) : 1.f / (1.f + e);
}

// One channel's cumulative network as its forward uses it.  Offsets into sp: layer 0 at 0 (3 x 1), layers 1..3 at 3 + 9 (k - 1)
// (3 x 3, row-major [out][in]), layer 4 at 30 (1 x 3); into b: 3 k; into tf: 3 k.
struct EbNet {
  float sp[kMat], b[kBias], tf[kFac];
};
// What the backward needs of one evaluation: h[k] the output of layer k (the input of layer k + 1), t[k] = tanh of its
// pre-activation, x the input.
struct EbAct {
  float x, h[4][3], t[4][3];
};
struct EbAcc {
  float sp[kMat], b[kBias], tf[kFac];
};

// params[k * C + c], k = 0 .. 57 in the order of the header: the lanes of a wave read adjacent words
__device__ __forceinline__ void eb_load(EbNet &n, const float *__restrict__ params, int C, int c) {
#pragma unroll
  for (int k = 0; k < kMat; ++k) n.sp[k] = softplus_f(params[(size_t)k * C + c]);
#pragma unroll
  for (int k = 0; k < kBias; ++k) n.b[k] = params[(size_t)(kMat + k) * C + c];
#pragma unroll
  for (int k = 0; k < kFac; ++k) n.tf[k] = tanhf(params[(size_t)(kMat + kBias + k) * C + c]);
}

// L(x): x <- softplus(M_k) x + B_k, then x <- x + tanh(F_k) tanh(x) for k < 4.  Every row sum is ((m0 h0 + m1 h1) + m2 h2) + b.
__device__ __forceinline__ float eb_forward(const EbNet &n, float x, EbAct &a) {
  a.x = x;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const float pre = n.sp[j] * x + n.b[j];
    a.t[0][j] = tanhf(pre);
    a.h[0][j] = pre + n.tf[j] * a.t[0][j];
  }
#pragma unroll
  for (int k = 1; k < 4; ++k) {
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const float *m = &n.sp[3 + 9 * (k - 1) + 3 * j];
      const float pre = ((m[0] * a.h[k - 1][0] + m[1] * a.h[k - 1][1]) + m[2] * a.h[k - 1][2]) + n.b[3 * k + j];
      a.t[k][j] = tanhf(pre);
      a.h[k][j] = pre + n.tf[3 * k + j] * a.t[k][j];
    }
  }
  return ((n.sp[30] * a.h[3][0] + n.sp[31] * a.h[3][1]) + n.sp[32] * a.h[3][2]) + n.b[12];
}

// Reverse pass of one evaluation seeded with g = d loss / d L(x): returns g dL/dx and, with ACC, adds g times the derivatives
// with respect to softplus(matrix), bias and tanh(factor) to `acc`.
template <bool ACC>
__device__ __forceinline__ float eb_backward(const EbNet &n, const EbAct &a, float g, EbAcc &acc) {
  float dh[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    dh[i] = g * n.sp[30 + i];
    if (ACC) acc.sp[30 + i] += g * a.h[3][i];
  }
  if (ACC) acc.b[12] += g;
#pragma unroll
  for (int k = 3; k >= 1; --k) {
    float da[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const float t = a.t[k][j];
      da[j] = dh[j] * (1.f + n.tf[3 * k + j] * (1.f - t * t));
      if (ACC) {
        acc.tf[3 * k + j] += dh[j] * t;
        acc.b[3 * k + j] += da[j];
#pragma unroll
        for (int i = 0; i < 3; ++i) acc.sp[3 + 9 * (k - 1) + 3 * j + i] += da[j] * a.h[k - 1][i];
      }
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const float *m = &n.sp[3 + 9 * (k - 1)];
      dh[i] = (m[i] * da[0] + m[3 + i] * da[1]) + m[6 + i] * da[2];
    }
  }
  float dx = 0.f;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const float t = a.t[0][j];
    const float da = dh[j] * (1.f + n.tf[j] * (1.f - t * t));
    if (ACC) {
      acc.tf[j] += dh[j] * t;
      acc.b[j] += da;
      acc.sp[j] += da * a.x;
    }
    dx += n.sp[j] * da;
  }
  return dx;
}

// lik = |sigmoid(a) - sigmoid(b)| for a = sgn upper, b = sgn lower (a + b <= 0: at most one is positive), signed as the
// difference.  Both in the lower tail: (exp(a) - exp(b)) / ((1 + exp(a)) (1 + exp(b))) with the numerator as
// -exp(max) expm1(-|a - b|) -- no cancellation between two nearly equal tail values; otherwise the plain difference.
__device__ __forceinline__ float sigmoid_diff(float a, float b) {
  const float ea = expf(-fabsf(a)), eb = expf(-fabsf(b));
  if (a <= 0.f && b <= 0.f) {
    const float d = a - b;
    const float num = d >= 0.f ? -(ea * expm1f(-d)) : eb * expm1f(d);   // expm1 of a non-positive number: no overflow
    return num / ((1.f + ea) * (1.f + eb));
  }
  const float sa = a <= 0.f ? ea / (1.f + ea) : 1.f / (1.f + ea), sb = b <= 0.f ? eb / (1.f + eb) : 1.f / (1.f + eb);
  return sa - sb;
}
// sigmoid'(t) = e / (1 + e)^2, e = exp(-|t|)
__device__ __forceinline__ float sigmoid_slope(float t) {
  const float e = expf(-fabsf(t));
  return e / ((1.f + e) * (1.f + e));
}
__device__ __forceinline__ float sign_f(float x) { return x > 0.f ? 1.f : x < 0.f ? -1.f : 0.f; }

// ---- what eb_pass_kernel and side_pass_kernel share of a walk: the accumulators' start, one element, the walker's 58 stores
__device__ __forceinline__ void eb_acc_zero(EbAcc &acc) {
#pragma unroll
  for (int k = 0; k < kMat; ++k) acc.sp[k] = 0.f;
#pragma unroll
  for (int k = 0; k < kBias; ++k) acc.b[k] = 0.f;
#pragma unroll
  for (int k = 0; k < kFac; ++k) acc.tf[k] = 0.f;
}

// One element of the bounded likelihood at v (noise already added): adds -log lik to sum_rate and the element's share of the
// network's gradients to acc, returns d(-log lik) / dv.
__device__ __forceinline__ float eb_lik_step(const EbNet &n, float v, EbAcc &acc, float &sum_rate) {
  EbAct lo, up;
  const float lower = eb_forward(n, v - 0.5f, lo), upper = eb_forward(n, v + 0.5f, up);
  const float sgn = -sign_f(lower + upper);
  const float a = sgn * upper, b = sgn * lower;
  const float diff = sigmoid_diff(a, b);
  const float lik = fmaxf(fabsf(diff), kLikBound);
  sum_rate += -logf(lik);
  // d(-log lik) / d lik = -1 / lik through the bound (header); |.| and the constant sign give the seeds of the two evaluations
  const float gl = -1.f / lik * sign_f(diff) * sgn;
  return eb_backward<true>(n, up, gl * sigmoid_slope(a), acc) + eb_backward<true>(n, lo, -gl * sigmoid_slope(b), acc);
}

// The lane's 58 network gradients to rows row0 .. row0 + 57 of `out` ([.][C], already at the lane's channel c), through the
// chain rule of the parameters' own images: d softplus(m) = sigmoid(m), d tanh(f) = 1 - tanh(f)^2.
__device__ __forceinline__ void eb_store_grads(const EbNet &n, const EbAcc &acc, const float *params, int C, int c, float *out,
                                               int row0) {
#pragma unroll
  for (int k = 0; k < kMat; ++k) out[(size_t)(row0 + k) * C] = acc.sp[k] * sigmoid_f(params[(size_t)k * C + c]);
#pragma unroll
  for (int k = 0; k < kBias; ++k) out[(size_t)(row0 + kMat + k) * C] = acc.b[k];
#pragma unroll
  for (int k = 0; k < kFac; ++k) out[(size_t)(row0 + kMat + kBias + k) * C] = acc.tf[k] * (1.f - n.tf[k] * n.tf[k]);
}

// ---- what the finish kernels share.  The sum of element `at` over the W walkers' slabs, in walker order, in double.
__device__ __forceinline__ double walker_sum(const float *__restrict__ part, size_t slab, size_t at, int W) {
  double sum = 0.0;
  for (int w = 0; w < W; ++w) sum += (double)part[w * slab + at];
  return sum;
}

// The scalar sums of a pass, by the LAST workgroup (256 threads) of its finish kernel: for q < Q, out[q] = the sum over the
// channels of the walker_sum of partial row first + q; thread t adds the channels t, t + 256, ... in ascending order and
// thread 0 .. Q-1 adds the 256 thread sums of its q in thread order.
template <int Q>
__device__ __forceinline__ void channel_totals(const float *__restrict__ part, size_t slab, int first, int C, int W,
                                               double *__restrict__ out, double (*red)[256]) {
  double tot[Q];
#pragma unroll
  for (int q = 0; q < Q; ++q) tot[q] = 0.0;
  for (int c = threadIdx.x; c < C; c += 256) {
#pragma unroll
    for (int q = 0; q < Q; ++q) tot[q] += walker_sum(part, slab, (size_t)(first + q) * C + c, W);
  }
#pragma unroll
  for (int q = 0; q < Q; ++q) red[q][threadIdx.x] = tot[q];
  __syncthreads();
  if (threadIdx.x < Q) {
    double sum = 0.0;
    for (int t = 0; t < 256; ++t) sum += red[threadIdx.x][t];
    out[threadIdx.x] = sum;
  }
}

template <typename T>
__device__ __forceinline__ float load_z(const void *z, size_t at) {
  return (float)reinterpret_cast<const T *>(z)[at];
}

inline bool aligned16(const void *q) { return ((uintptr_t)q & 15) == 0; }

// walkers of a pass: enough rows each to amortise the parameter set-up, no more waves than the chip holds at once
inline int eb_walkers(int B, int C) {
  const int groups = (C + kWave - 1) / kWave;
  const int most = kWaveSlots / groups > 1 ? kWaveSlots / groups : 1;
  const int want = (B + kRowsPerWalker - 1) / kRowsPerWalker;
  return want < 1 ? 1 : want < most ? want : most;
}

}  // namespace
}  // namespace lla
