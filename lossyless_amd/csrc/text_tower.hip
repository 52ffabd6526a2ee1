// CLIP text tower (gfx950): the kernels of `encode_text` (clip/model.py) that are not Linear layers.
//
// The reference featurises captions with `encode_text` (utils/data/images.py:1299-1323); zero-shot classification compares
// an image embedding with the text embeddings of class prompts.  The Linear layers of the tower (QKV, out-proj, c_fc,
// c_proj, text_projection) run on lla_gemm_f32 (gemm_f32.hip); what is here is the token embedding, the row LayerNorm, the
// causal attention and the two pointwise steps between the GEMMs, plus the unit-row step of ZeroShotProbe.
//
// Everything is fp32, there is no floating-point atomic, and the order of every sum is fixed by the row's own length alone:
// a row's bits do not depend on the batch size or on where the prompt sits in the batch.  include/lossyless_amd.h states the
// mathematics.  The Makefile compiles with -ffp-contract=off: a product and a sum round separately unless written as fmaf.
#include "common.h"

#include <math.h>

namespace lla {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kHeadDim = 64;
constexpr int kMaxContext = 77;

// x[r][:] = tok_emb[tokens[r]][:] + pos[r % T][:], a thread per 16 bytes.  The index is clamped: nothing is read outside
// tok_emb whatever the tokens hold (Python refuses ids outside [0, V) before the call).
__global__ __launch_bounds__(256) void text_embed_kernel(const int32_t *__restrict__ tokens,
                                                         const float *__restrict__ tok_emb,
                                                         const float *__restrict__ pos, float *__restrict__ x,
                                                         long long n4, int T, int V, int D4) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= n4) return;
  const long long r = e / D4;
  const int c = (int)(e - r * D4);
  int tok = tokens[r];
  tok = tok < 0 ? 0 : (tok >= V ? V - 1 : tok);
  const int t = (int)(r % T);
  const f32x4 a = reinterpret_cast<const f32x4 *>(tok_emb)[(size_t)tok * D4 + c];
  const f32x4 p = reinterpret_cast<const f32x4 *>(pos)[(size_t)t * D4 + c];
  reinterpret_cast<f32x4 *>(x)[e] = a + p;
}

// Row LayerNorm, one wave per row: lane l holds elements l, l + 64, ... (D / 64 <= 16 of them, in registers).  Two passes
// over the registers: the mean, then the variance of the centred values.  Each lane adds its elements in index order and
// the 64 lane sums go through wave_sum_f32's fixed tree.
__global__ __launch_bounds__(256) void layernorm_rows_kernel(const float *__restrict__ x, size_t row_stride,
                                                             const float *__restrict__ w, const float *__restrict__ b,
                                                             float *__restrict__ y, size_t y_stride, int rows, int D,
                                                             float eps) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;       // wave-uniform: the waves that stay are whole
  const int n = D >> 6;
  const float *xr = x + (size_t)row * row_stride;
  float v[16];
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    v[j] = j < n ? xr[j * 64 + lane] : 0.f;
    if (j < n) s += v[j];
  }
  const float mean = wave_sum_f32(s) / (float)D;
  float q = 0.f;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    v[j] -= mean;
    if (j < n) q += v[j] * v[j];
  }
  const float rstd = 1.f / sqrtf(wave_sum_f32(q) / (float)D + eps);
  float *yr = y + (size_t)row * y_stride;
#pragma unroll
  for (int j = 0; j < 16; ++j)
    if (j < n) yr[j * 64 + lane] = v[j] * rstd * w[j * 64 + lane] + b[j * 64 + lane];
}

// Causal attention, one workgroup per (prompt, head).  The head's K and V panels (T x 64 fp32 each) sit in LDS; thread i < T
// owns query row i: q_i and o_i in registers, every K / V read is the same address in all lanes (a broadcast).  Three walks
// over j <= i: the row maximum, the sum of expf(s - max), then o_i = sum_j (e_ij / sum) v_j in increasing j.  The score is
// recomputed in each walk (the same fmaf chain over the 64 dimensions, so the same bits) instead of being kept: T scores
// per lane would not stay in registers.  The walk runs to the wave's last row (jmax: the loop bound is wave-uniform), so a
// lane also reads keys j > i from LDS and computes their score and expf; the `j <= i` guards discard them, whatever they
// are.  The causal half therefore saves no work in a wave whose last row is long.
__global__ __launch_bounds__(128) void attention_causal_kernel(const float *__restrict__ qkv, float *__restrict__ o, int T,
                                                               int heads) {
  __shared__ f32x4 Ks[kMaxContext * kHeadDim / 4];
  __shared__ f32x4 Vs[kMaxContext * kHeadDim / 4];
  const int p = blockIdx.x / heads, h = blockIdx.x - p * heads;
  const int D = heads * kHeadDim;
  const size_t ld = 3 * (size_t)D;
  const float *base = qkv + (size_t)p * T * ld + (size_t)h * kHeadDim;
  for (int e = threadIdx.x; e < T * (kHeadDim / 4); e += blockDim.x) {
    const int j = e >> 4, c = e & 15;
    const float *row = base + (size_t)j * ld;
    Ks[e] = reinterpret_cast<const f32x4 *>(row + D)[c];
    Vs[e] = reinterpret_cast<const f32x4 *>(row + 2 * D)[c];
  }
  __syncthreads();
  const int i = threadIdx.x;
  if (i >= T) return;            // (after the only barrier)
  f32x4 q[16];
  {
    const f32x4 *qr = reinterpret_cast<const f32x4 *>(base + (size_t)i * ld);
#pragma unroll
    for (int c = 0; c < 16; ++c) q[c] = qr[c];
  }
  // the last row of this wave: the loop bound is the same in every lane, a lane's own rows end at j == i
  const int jmax = min(T - 1, (i | 63));
  auto score = [&](int j) {
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < 16; ++c) {
      const f32x4 k = Ks[j * 16 + c];
#pragma unroll
      for (int u = 0; u < 4; ++u) s = __builtin_fmaf(q[c][u], k[u], s);
    }
    return s * 0.125f;
  };
  float mx = score(0);
  for (int j = 1; j <= jmax; ++j) {
    const float s = score(j);
    if (j <= i) mx = fmaxf(mx, s);
  }
  float den = 0.f;
  for (int j = 0; j <= jmax; ++j) {
    const float e = expf(score(j) - mx);
    if (j <= i) den += e;
  }
  f32x4 acc[16];
  {
    const float pj = expf(score(0) - mx) / den;
#pragma unroll
    for (int c = 0; c < 16; ++c) acc[c] = Vs[c] * pj;
  }
  for (int j = 1; j <= jmax; ++j) {
    const float pj = expf(score(j) - mx) / den;
    if (j <= i) {
#pragma unroll
      for (int c = 0; c < 16; ++c) {
        const f32x4 v = Vs[j * 16 + c];
#pragma unroll
        for (int u = 0; u < 4; ++u) acc[c][u] = __builtin_fmaf(pj, v[u], acc[c][u]);
      }
    }
  }
  f32x4 *orow = reinterpret_cast<f32x4 *>(o + ((size_t)p * T + i) * D + (size_t)h * kHeadDim);
#pragma unroll
  for (int c = 0; c < 16; ++c) orow[c] = acc[c];
}

__device__ __forceinline__ float quick_gelu(float y) { return y * (1.f / (1.f + expf(-(1.702f * y)))); }

// mode 0: x += y;  mode 1: y = y sigmoid(1.702 y).  16 bytes per thread, the n % 4 tail one by one.
template <int MODE>
__global__ __launch_bounds__(256) void text_pointwise_kernel(float *__restrict__ x, float *__restrict__ y, long long n) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long n4 = n >> 2;
  if (e < n4) {
    f32x4 b = reinterpret_cast<f32x4 *>(y)[e];
    if (MODE == 0) {
      reinterpret_cast<f32x4 *>(x)[e] += b;
    } else {
#pragma unroll
      for (int u = 0; u < 4; ++u) b[u] = quick_gelu(b[u]);
      reinterpret_cast<f32x4 *>(y)[e] = b;
    }
  } else if (e - n4 < (n & 3)) {
    const long long t = 4 * n4 + (e - n4);
    if (MODE == 0) x[t] += y[t];
    else y[t] = quick_gelu(y[t]);
  }
}

// out[r] = z[r] / |z[r]|_2 (a row of zeros stays zeros), one wave per row: lane l adds the squares of elements l, l + 64, ...
// in index order, the lane sums go through wave_sum_f32's tree -- a function of C alone.
__global__ __launch_bounds__(256) void unit_rows_kernel(const float *__restrict__ z, size_t ld_z, float *__restrict__ out,
                                                        size_t ld_out, int rows, int C) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const float *zr = z + (size_t)row * ld_z;
  float q = 0.f;
  for (int c = lane; c < C; c += 64) q += zr[c] * zr[c];
  const float norm = sqrtf(wave_sum_f32(q));
  float *orow = out + (size_t)row * ld_out;
  for (int c = lane; c < C; c += 64) orow[c] = norm > 0.f ? zr[c] / norm : 0.f;
}

inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline bool blocks_ok(long long threads, int per_block) { return (threads + per_block - 1) / per_block <= 0x7fffffffLL; }

}  // namespace
}  // namespace lla

using namespace lla;

extern "C" int lla_text_embed(const int32_t *tokens, int P, int T, const float *tok_emb, int V, const float *pos, int D,
                              float *x, void *stream) {
  if (P < 0 || T <= 0 || V <= 0 || D <= 0 || (D & 3)) return LLA_EINVAL;
  if (P == 0) return LLA_OK;
  if (!tokens || !tok_emb || !pos || !x || !aligned16(tok_emb) || !aligned16(pos) || !aligned16(x)) return LLA_EINVAL;
  const long long n4 = (long long)P * T * (D / 4);
  if (!blocks_ok(n4, 256)) return LLA_EINVAL;
  text_embed_kernel<<<(unsigned)((n4 + 255) / 256), 256, 0, as_stream(stream)>>>(tokens, tok_emb, pos, x, n4, T, V, D / 4);
  return check_launch();
}

extern "C" int lla_layernorm_rows(const float *x, size_t row_stride, const float *w, const float *b, float *y,
                                  size_t y_stride, int rows, int D, float eps, void *stream) {
  if (rows < 0 || D < 64 || D > 1024 || (D & 63) || row_stride < (size_t)D || y_stride < (size_t)D || !(eps >= 0.f))
    return LLA_EINVAL;
  if (rows == 0) return LLA_OK;
  if (!x || !w || !b || !y) return LLA_EINVAL;
  layernorm_rows_kernel<<<(unsigned)((rows + 3) / 4), 256, 0, as_stream(stream)>>>(x, row_stride, w, b, y, y_stride, rows, D,
                                                                                  eps);
  return check_launch();
}

extern "C" int lla_attention_causal(const float *qkv, float *o, int P, int T, int heads, void *stream) {
  if (P < 0 || T < 1 || T > kMaxContext || heads < 1 || heads > 1024) return LLA_EINVAL;
  if (P == 0) return LLA_OK;
  if (!qkv || !o || !aligned16(qkv) || !aligned16(o)) return LLA_EINVAL;
  const long long grid = (long long)P * heads;
  if (grid > 0x7fffffffLL) return LLA_EINVAL;
  attention_causal_kernel<<<(unsigned)grid, T <= 64 ? 64 : 128, 0, as_stream(stream)>>>(qkv, o, T, heads);
  return check_launch();
}

extern "C" int lla_text_pointwise(float *x, float *y, long long n, int mode, void *stream) {
  if (n < 0 || (mode != 0 && mode != 1)) return LLA_EINVAL;
  if (n == 0) return LLA_OK;
  if (!y || !aligned16(y) || (mode == 0 && (!x || !aligned16(x)))) return LLA_EINVAL;
  const long long threads = (n >> 2) + (n & 3);
  if (!blocks_ok(threads, 256)) return LLA_EINVAL;
  const unsigned grid = (unsigned)((threads + 255) / 256);
  if (mode == 0) text_pointwise_kernel<0><<<grid, 256, 0, as_stream(stream)>>>(x, y, n);
  else text_pointwise_kernel<1><<<grid, 256, 0, as_stream(stream)>>>(x, y, n);
  return check_launch();
}

extern "C" int lla_unit_rows(const float *z, size_t ld_z, float *out, size_t ld_out, int rows, int C, void *stream) {
  if (rows < 0 || C < 1 || ld_z < (size_t)C || ld_out < (size_t)C) return LLA_EINVAL;
  if (rows == 0) return LLA_OK;
  if (!z || !out) return LLA_EINVAL;
  unit_rows_kernel<<<(unsigned)((rows + 3) / 4), 256, 0, as_stream(stream)>>>(z, ld_z, out, ld_out, rows, C);
  return check_launch();
}
