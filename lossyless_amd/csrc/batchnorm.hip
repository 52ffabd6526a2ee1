// BatchNorm1d -> ReLU -> Dropout of an MLP predictor's hidden block, training mode, forward and backward, on gfx950.
//
// Stands in for the hidden blocks of the reference's predictor as its configuration builds them
// (config/architecture/mlp_probe.yaml: norm_layer batchnorm, activation ReLU, dropout_p 0.2): lossyless/architectures.py:137-153
// makes each block Linear(bias=False) -> BatchNorm1d -> ReLU -> Dropout(p).  The Linear layers are the GEMMs of gemm_f32.hip and
// mlp.hip, unchanged; BatchNormMLPProbe (probe.py) puts the two kernels below between them.
//
//   lla_bn_relu_dropout_fwd   out = dropout(relu(gamma (a - mean) rstd + beta)), the batch statistics mean / rstd for the
//                             backward, and torch.nn.BatchNorm1d's update of running_mean / running_var
//   lla_bn_bwd                dgamma, dbeta and da from g = dOut . [out > 0] (what lla_gemm_f32_nn's mask delivers)
//
// Arrangement, both kernels: ONE launch; a workgroup of 256 threads owns a strip of 32 columns over ALL B rows (as
// gemm_f32_tn_kernel owns its tile over all of M), so there is no workspace, no second kernel and no atomics.  Thread t holds
// the column quad 4 (t & 7) of the strip and walks the rows (t >> 3), (t >> 3) + 32, ...: 16 bytes per lane, eight lanes
// read one whole 128-byte line.  The rows are walked once per column sum and once more to apply (the re-reads hit L2: a
// strip is B x 128 bytes).
//
// Arithmetic: DOUBLE THROUGHOUT.  Every fp32 operand is widened, every sum, the statistics and every element are formed in
// double, and each stored fp32 value is rounded once.  The variance is the biased two-pass sum of (a - mean)^2 with the
// double mean (never E[a^2] - mean^2).  The backward recomputes xhat = (a - mean) rstd from the STORED fp32 mean and rstd.
// The kernels are bound by their memory traffic and by latency, not by the fp64 rate.
// Order of every column sum, a function of (B, N) alone: thread (r, q) adds its rows r, r + 32, ... in ascending order;
// the 32 partial sums of a column go through LDS and ONE thread adds them in the order r = 0 .. 31.  The same inputs give
// the same bits.
//
// Dropout is counter-based: Philox4x32-10 with key (seed_lo, seed_hi) and counter (e_lo, e_hi, step, layer),
// e = (i N + j) / 4 for the quad of columns j .. j + 3 of minibatch row i (N % 4 == 0: one row).  Word w of the output
// serves column j + w: u = (float)(word >> 8) 2^-24 (exact), kept iff u >= (float)p, and a kept value is h s in fp32 with
// s = (float)(1 / (1 - (double)p)).  The mask is a function of (seed, step, layer, i, j) alone -- not of the grid, the pitch
// or the decode group -- and p == 0 draws nothing.
#include "common.h"

#include <cmath>

namespace lla {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kBnCols = 32;                  // columns per workgroup: eight quads
constexpr int kBnRows = 32;                  // rows in flight per workgroup: 256 threads / 8 quads

struct Philox {
  uint32_t v[4];
};

// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11): ten rounds, the key bumped by the
// Weyl constants between them.
__device__ __forceinline__ Philox philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                                uint32_t k1) {
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1, c3 = (uint32_t)p0, c0 = n0, c2 = n2;
    k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
  }
  return {{c0, c1, c2, c3}};
}

// The sums over all rows of each of the strip's 32 columns, from the partial sums v[0..3] of thread (r, q) for the columns
// 4 q .. 4 q + 3: tot[c] = part[0][c] + part[1][c] + ... + part[31][c], added in that order by thread c.  Every thread of
// the workgroup calls it; on return tot is readable by all and part may be reused.
__device__ __forceinline__ void strip_column_sums(double (*part)[kBnCols], double *tot, const double v[4], int r, int q) {
#pragma unroll
  for (int e = 0; e < 4; ++e) part[r][4 * q + e] = v[e];
  __syncthreads();
  if (threadIdx.x < kBnCols) {
    double s = 0.0;
    for (int i = 0; i < kBnRows; ++i) s += part[i][threadIdx.x];
    tot[threadIdx.x] = s;
  }
  __syncthreads();
}

struct BnFwd {
  double eps, momentum;
  float p, s;                                // the drop probability and 1 / (1 - p), both as the fp32 values compared / multiplied
  uint32_t k0, k1, step, layer;
};

template <bool DROP>
__global__ __launch_bounds__(256) void bn_relu_dropout_fwd_kernel(const float *__restrict__ a, int lda,
                                                                  const float *__restrict__ gamma,
                                                                  const float *__restrict__ beta, float *__restrict__ out,
                                                                  int ldo, float *__restrict__ mean, float *__restrict__ rstd,
                                                                  float *__restrict__ running_mean,
                                                                  float *__restrict__ running_var, int B, int N, BnFwd f) {
  __shared__ double part[kBnRows][kBnCols];
  __shared__ double tot_a[kBnCols], tot_d[kBnCols];
  const int q = threadIdx.x & 7, r = threadIdx.x >> 3;
  const int j = blockIdx.x * kBnCols + 4 * q;
  const bool live = j < N;                   // N % 4 == 0: a quad is inside or outside
  const float *ap = a + j;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  if (live) {
#pragma unroll 4
    for (int i = r; i < B; i += kBnRows) {
      const f32x4 v = *reinterpret_cast<const f32x4 *>(ap + (size_t)i * lda);
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[e] += (double)v[e];
    }
  }
  strip_column_sums(part, tot_a, acc, r, q);
  double mu[4], var[4], rs[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) mu[e] = tot_a[4 * q + e] / (double)B, acc[e] = 0.0;
  if (live) {
#pragma unroll 4
    for (int i = r; i < B; i += kBnRows) {
      const f32x4 v = *reinterpret_cast<const f32x4 *>(ap + (size_t)i * lda);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const double d = (double)v[e] - mu[e];
        acc[e] += d * d;
      }
    }
  }
  strip_column_sums(part, tot_d, acc, r, q);
#pragma unroll
  for (int e = 0; e < 4; ++e) var[e] = tot_d[4 * q + e] / (double)B, rs[e] = 1.0 / sqrt(var[e] + f.eps);
  if (!live) return;                         // (after the last barrier)
  if (r == 0) {
    f32x4 m4, r4;
#pragma unroll
    for (int e = 0; e < 4; ++e) m4[e] = (float)mu[e], r4[e] = (float)rs[e];
    *reinterpret_cast<f32x4 *>(mean + j) = m4;
    *reinterpret_cast<f32x4 *>(rstd + j) = r4;
    if (running_mean != nullptr) {
      f32x4 rm = *reinterpret_cast<const f32x4 *>(running_mean + j), rv = *reinterpret_cast<const f32x4 *>(running_var + j);
      const double unbias = (double)B / (double)(B - 1);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        rm[e] = (float)((1.0 - f.momentum) * (double)rm[e] + f.momentum * mu[e]);
        rv[e] = (float)((1.0 - f.momentum) * (double)rv[e] + f.momentum * (var[e] * unbias));
      }
      *reinterpret_cast<f32x4 *>(running_mean + j) = rm;
      *reinterpret_cast<f32x4 *>(running_var + j) = rv;
    }
  }
  const f32x4 g4 = *reinterpret_cast<const f32x4 *>(gamma + j), b4 = *reinterpret_cast<const f32x4 *>(beta + j);
  double sc[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) sc[e] = (double)g4[e] * rs[e];
#pragma unroll 4
  for (int i = r; i < B; i += kBnRows) {
    const f32x4 v = *reinterpret_cast<const f32x4 *>(ap + (size_t)i * lda);
    f32x4 h;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const double y = sc[e] * ((double)v[e] - mu[e]) + (double)b4[e];
      h[e] = y > 0.0 ? (float)y : 0.f;
    }
    if (DROP) {
      const uint64_t quad = ((uint64_t)i * (uint64_t)N + (uint64_t)j) >> 2;
      const Philox w = philox4x32_10((uint32_t)quad, (uint32_t)(quad >> 32), f.step, f.layer, f.k0, f.k1);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float u = (float)(w.v[e] >> 8) * 0x1p-24f;
        h[e] = u >= f.p ? h[e] * f.s : 0.f;
      }
    }
    *reinterpret_cast<f32x4 *>(out + (size_t)i * ldo + j) = h;
  }
}

// g and da may be the same buffer: a thread reads its own element in both walks and writes it in the second, and the
// workgroups' strips are disjoint.
__global__ __launch_bounds__(256) void bn_bwd_kernel(const float *g, int ldg, const float *__restrict__ a, int lda,
                                                     const float *__restrict__ gamma, const float *__restrict__ mean,
                                                     const float *__restrict__ rstd, float s, float *__restrict__ dgamma,
                                                     float *__restrict__ dbeta, float *da, int ldda, int B, int N) {
  __shared__ double part[kBnRows][kBnCols];
  __shared__ double tot_b[kBnCols], tot_g[kBnCols];
  const int q = threadIdx.x & 7, r = threadIdx.x >> 3;
  const int j = blockIdx.x * kBnCols + 4 * q;
  const bool live = j < N;
  const double sd = (double)s;
  double mu[4] = {0.0, 0.0, 0.0, 0.0}, rs[4] = {0.0, 0.0, 0.0, 0.0};
  double sb[4] = {0.0, 0.0, 0.0, 0.0}, sg[4] = {0.0, 0.0, 0.0, 0.0};
  if (live) {
    const f32x4 m4 = *reinterpret_cast<const f32x4 *>(mean + j), r4 = *reinterpret_cast<const f32x4 *>(rstd + j);
#pragma unroll
    for (int e = 0; e < 4; ++e) mu[e] = (double)m4[e], rs[e] = (double)r4[e];
#pragma unroll 4
    for (int i = r; i < B; i += kBnRows) {
      const f32x4 gv = *reinterpret_cast<const f32x4 *>(g + (size_t)i * ldg + j);
      const f32x4 av = *reinterpret_cast<const f32x4 *>(a + (size_t)i * lda + j);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const double gh = sd * (double)gv[e];
        sb[e] += gh;
        sg[e] += gh * (((double)av[e] - mu[e]) * rs[e]);
      }
    }
  }
  strip_column_sums(part, tot_b, sb, r, q);
  strip_column_sums(part, tot_g, sg, r, q);
  if (!live) return;                         // (after the last barrier)
  double db[4], dg[4], sc[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) db[e] = tot_b[4 * q + e], dg[e] = tot_g[4 * q + e];
  if (r == 0) {
    f32x4 b4, g4;
#pragma unroll
    for (int e = 0; e < 4; ++e) b4[e] = (float)db[e], g4[e] = (float)dg[e];
    *reinterpret_cast<f32x4 *>(dbeta + j) = b4;
    *reinterpret_cast<f32x4 *>(dgamma + j) = g4;
  }
  const f32x4 w4 = *reinterpret_cast<const f32x4 *>(gamma + j);
#pragma unroll
  for (int e = 0; e < 4; ++e) sc[e] = (double)w4[e] * rs[e], db[e] /= (double)B, dg[e] /= (double)B;
#pragma unroll 4
  for (int i = r; i < B; i += kBnRows) {
    const f32x4 gv = *reinterpret_cast<const f32x4 *>(g + (size_t)i * ldg + j);
    const f32x4 av = *reinterpret_cast<const f32x4 *>(a + (size_t)i * lda + j);
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const double xh = ((double)av[e] - mu[e]) * rs[e];
      o[e] = (float)(sc[e] * ((sd * (double)gv[e] - db[e]) - xh * dg[e]));
    }
    *reinterpret_cast<f32x4 *>(da + (size_t)i * ldda + j) = o;
  }
}

bool aligned16(const void *q) { return ((uintptr_t)q & 15) == 0; }

bool shape_ok(int B, int N, int ld0, int ld1) {
  return B >= 0 && B != 1 && N > 0 && !(N & 3) && ld0 >= N && ld1 >= N && !(ld0 & 3) && !(ld1 & 3);
}

}  // namespace
}  // namespace lla

using namespace lla;

extern "C" int lla_bn_relu_dropout_fwd(const float *a, int lda, const float *gamma, const float *beta, float *out, int ldo,
                                       float *mean, float *rstd, float *running_mean, float *running_var, int B, int N,
                                       double eps, double momentum, double p, uint64_t seed, uint32_t step, uint32_t layer,
                                       void *stream) {
  if (!shape_ok(B, N, lda, ldo) || !(eps >= 0.0) || !(momentum >= 0.0 && momentum <= 1.0) || !(p >= 0.0 && p < 1.0) ||
      !((float)p < 1.f))
    return LLA_EINVAL;
  if (B == 0) return LLA_OK;
  if (!a || !gamma || !beta || !out || !mean || !rstd || (running_mean == nullptr) != (running_var == nullptr) || a == out)
    return LLA_EINVAL;
  if (!aligned16(a) || !aligned16(gamma) || !aligned16(beta) || !aligned16(out) || !aligned16(mean) || !aligned16(rstd) ||
      !aligned16(running_mean) || !aligned16(running_var))
    return LLA_EINVAL;
  const BnFwd f = {eps, momentum, (float)p, (float)(1.0 / (1.0 - p)), (uint32_t)seed, (uint32_t)(seed >> 32), step, layer};
  const int grid = (N + kBnCols - 1) / kBnCols;
  hipStream_t st = as_stream(stream);
  if (p > 0.0)
    bn_relu_dropout_fwd_kernel<true><<<grid, 256, 0, st>>>(a, lda, gamma, beta, out, ldo, mean, rstd, running_mean,
                                                         running_var, B, N, f);
  else
    bn_relu_dropout_fwd_kernel<false><<<grid, 256, 0, st>>>(a, lda, gamma, beta, out, ldo, mean, rstd, running_mean,
                                                          running_var, B, N, f);
  return check_launch();
}

extern "C" int lla_bn_bwd(const float *g, int ldg, const float *a, int lda, const float *gamma, const float *mean,
                          const float *rstd, double p, float *dgamma, float *dbeta, float *da, int ldda, int B, int N,
                          void *stream) {
  if (!shape_ok(B, N, ldg, lda) || ldda < N || (ldda & 3) || !(p >= 0.0 && p < 1.0) || !((float)p < 1.f)) return LLA_EINVAL;
  if (B == 0) return LLA_OK;
  if (!g || !a || !gamma || !mean || !rstd || !dgamma || !dbeta || !da || a == da) return LLA_EINVAL;
  if (!aligned16(g) || !aligned16(a) || !aligned16(gamma) || !aligned16(mean) || !aligned16(rstd) || !aligned16(dgamma) ||
      !aligned16(dbeta) || !aligned16(da))
    return LLA_EINVAL;
  bn_bwd_kernel<<<(N + kBnCols - 1) / kBnCols, 256, 0, as_stream(stream)>>>(g, ldg, a, lda, gamma, mean, rstd,
                                                                           (float)(1.0 / (1.0 - p)), dgamma, dbeta, da, ldda,
                                                                           B, N);
  return check_launch();
}
