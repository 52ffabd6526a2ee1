// What a training step of an MLP predictor needs beside the forward GEMM (gemm_f32.hip), on gfx950: the two other GEMM
// orientations of the backward pass, the softmax cross-entropy residual and a fused AdamW update.
//
// Stands in for the reference's downstream predictor: lossyless/predictors.py:38-232 trains lossyless/architectures.py:94-168
// (MLP: Linear -> Norm -> ReLU -> Dropout per hidden layer, then Linear) with cross-entropy (predictors.py:172-186) and
// Adam / AdamW on shuffled minibatches of Z.  autograd's backward of a Linear layer is the two products below; MLPProbe
// (probe.py) runs them on minibatches that CompressedLatents.batches() decodes from the compressed copy in HBM.
//
//   lla_gemm_f32_nn    dX[M][K] = dY[M][N] W[N][K]  (. [H > 0], the ReLU backward)      reduction over N
//   lla_gemm_f32_tn    dW[N][K] = dY[M][N]^T X[M][K],  db[n] = sum_i dY[i][n]            reduction over the batch M
//   lla_softmax_xent   dlogits = scale (softmax(logits) - onehot(y)), the loss sum and the number of rows got right
//   lla_adamw_step     torch.optim.AdamW's update over flat buffers
//
// Arithmetic and determinism, as gemm_f32.hip and probe.hip: fp32 operands, `v_mfma_f32_32x32x2_f32` (bitwise an fp32 fma
// chain: one rounding per product, fp32 accumulation), no floating-point atomics, and the order of every sum is a
// function of the shape alone, so the same inputs give the same bits.
//
//   nn  One 32 x 32 output tile per wave, operands straight from global memory as gemm_f32.hip (no LDS): the tile's
//       accumulator runs over n = 0 .. N-1 in groups of 8 (within a group the two half-waves take n0 + 4 h + j, j = 0..3).
//   tn  One workgroup owns a 32 (n) x 128 (k) tile of dW over ALL of M, so there is no workspace and no second kernel:
//       it walks the batch in chunks of 32 rows, stages dY[32][32] and X[32][128] in LDS (rows beyond M and columns beyond
//       N / K are zero-filled: they add exactly nothing) and each wave adds its 32 x 32 tile's 16 MFMAs -- step 4 of
//       svm_pass_kernel.  Every element of dW is one fma chain in row order; db is added in row order by one thread per
//       column from the staged dY (the workgroups of the first k tile).
//   softmax_xent  One wave per row: max (and the lowest index that reaches it), sum exp(s - max), then
//       p = exp(s - max) / sum and the residual; the cross-lane steps are fixed butterflies.  Row losses go to the
//       workspace and one workgroup adds them in a fixed order (the loss in double).
#include "common.h"

namespace lla {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

// ---------------------------------------------------------------------------------------------------------------- nn
// D^T = W^T dY^T: "A" lane l = W[n][k0 + (l & 31)], "B" lane l = dY[m0 + (l & 31)][n], n = n0 + 4 (l >> 5) + j for MFMA j
// of the group.  Lane l then holds output row m = m0 + (l & 31) and the columns k0 + 8 g + 4 (l >> 5) + e of register
// 4 g + e: four 16-byte stores per lane, and the mask H is read the same way.
template <bool MASK>
__global__ __launch_bounds__(256) void gemm_f32_nn_kernel(const float *__restrict__ dY, int ldy,
                                                          const float *__restrict__ W, int ldw,
                                                          const float *__restrict__ H, int ldh, float *__restrict__ dX,
                                                          int ldx, int M, int N, int K) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int r32 = lane & 31, hk = lane >> 5;
  const int tiles_k = (K + 63) / 64;
  const int tm = blockIdx.x / tiles_k, tk = blockIdx.x - tm * tiles_k;
  const int m0 = tm * 64 + (wid >> 1) * 32, k0 = tk * 64 + (wid & 1) * 32;
  if (m0 >= M || k0 >= K) return;
  int m = m0 + r32, kc = k0 + r32;
  if (m >= M) m = M - 1;       // clamped rows and columns are computed and not stored
  if (kc >= K) kc = K - 1;
  const float *yp = dY + (size_t)m * ldy + 4 * hk;
  const float *wp = W + (size_t)(4 * hk) * ldw + kc;
  f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int n = 0; n < N; n += 8) {
    f32x4 a = {0.f, 0.f, 0.f, 0.f}, w = {0.f, 0.f, 0.f, 0.f};
    if (n + 4 * hk < N) {      // N % 4 == 0: a quad of n is inside or outside (outside: both operands are zeros)
      a = *reinterpret_cast<const f32x4 *>(yp + n);
#pragma unroll
      for (int j = 0; j < 4; ++j) w[j] = wp[(size_t)(n + j) * ldw];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w[j], a[j], acc, 0, 0, 0);
  }
  const int mo = m0 + r32;
  if (mo >= M) return;
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const int kq = k0 + 8 * g + 4 * hk;
    if (kq >= K) continue;     // K % 4 == 0
    f32x4 v = {acc[4 * g], acc[4 * g + 1], acc[4 * g + 2], acc[4 * g + 3]};
    if (MASK) {
      const f32x4 h = *reinterpret_cast<const f32x4 *>(H + (size_t)mo * ldh + kq);
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = h[e] > 0.f ? v[e] : 0.f;      // (-0.0 > 0 is false: it masks)
    }
    *reinterpret_cast<f32x4 *>(dX + (size_t)mo * ldx + kq) = v;
  }
}

// ---------------------------------------------------------------------------------------------------------------- tn
constexpr int kTnRows = 32;                  // batch rows per staged chunk
constexpr int kTnN = 32;                     // columns of dY (rows of dW) per workgroup
constexpr int kTnK = 128;                    // columns of X (columns of dW) per workgroup: 32 per wave
constexpr int kTnYPitch = kTnN + 4;          // floats: 16-byte stores, and the MFMA's 32-lane reads touch 32 banks
constexpr int kTnXPitch = kTnK + 4;

// "A" lane l = dY[row 2 s + (l >> 5)][n0 + (l & 31)], "B" lane l = X[row 2 s + (l >> 5)][k0 + 32 wave + (l & 31)], both
// from LDS.  Lane l then holds column k = k0 + 32 wave + (l & 31) of the rows n0 + 8 g + 4 (l >> 5) + e: every store
// instruction writes two 128-byte row segments.
__global__ __launch_bounds__(256) void gemm_f32_tn_kernel(const float *__restrict__ dY, int ldy,
                                                          const float *__restrict__ X, int ldx, float *__restrict__ dW,
                                                          int ldw, float *__restrict__ db, int M, int N, int K) {
  __shared__ __align__(16) float Ys[kTnRows * kTnYPitch];
  __shared__ __align__(16) float Xs[kTnRows * kTnXPitch];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int r32 = lane & 31, hk = lane >> 5;
  const int k0 = blockIdx.x * kTnK, n0 = blockIdx.y * kTnN;
  const bool bias = db != nullptr && blockIdx.x == 0 && tid < kTnN;
  // staging: thread -> (row, quad) of the dY chunk (one quad each) and of the X chunk (four quads each)
  const int yr = tid >> 3, yq = (tid & 7) * 4;
  f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  float bsum = 0.f;
  for (int row0 = 0; row0 < M; row0 += kTnRows) {
    {
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (row0 + yr < M && n0 + yq < N) v = *reinterpret_cast<const f32x4 *>(dY + (size_t)(row0 + yr) * ldy + n0 + yq);
      *reinterpret_cast<f32x4 *>(Ys + yr * kTnYPitch + yq) = v;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int idx = tid + 256 * i, xr = idx >> 5, xq = (idx & 31) * 4;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (row0 + xr < M && k0 + xq < K) v = *reinterpret_cast<const f32x4 *>(X + (size_t)(row0 + xr) * ldx + k0 + xq);
      *reinterpret_cast<f32x4 *>(Xs + xr * kTnXPitch + xq) = v;
    }
    __syncthreads();
    if (k0 + 32 * wid < K) {                 // (a wave whose 32 columns lie beyond K has nothing to store)
#pragma unroll 4
      for (int s2 = 0; s2 < kTnRows / 2; ++s2) {
        const float a = Ys[(2 * s2 + hk) * kTnYPitch + r32];
        const float b = Xs[(2 * s2 + hk) * kTnXPitch + 32 * wid + r32];
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
      }
    }
    if (bias) {
      for (int r = 0; r < kTnRows; ++r) bsum += Ys[r * kTnYPitch + tid];      // rows beyond M are zeros
    }
    __syncthreads();                         // the next chunk's staging overwrites Ys and Xs
  }
  const int kc = k0 + 32 * wid + r32;
  if (kc < K) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int n = n0 + 8 * (r >> 2) + 4 * hk + (r & 3);
      if (n < N) dW[(size_t)n * ldw + kc] = acc[r];
    }
  }
  if (bias && n0 + tid < N) db[n0 + tid] = bsum;
}

// ------------------------------------------------------------------------------------------------------ softmax_xent
constexpr int kXentRows = 4;                 // rows per workgroup: one per wave

// One wave per row.  Lane l reads the columns l, l + 64, ...; a lane without a column holds (-inf, 0).
__global__ __launch_bounds__(256) void softmax_xent_kernel(const float *__restrict__ logits, int ld,
                                                           const int32_t *__restrict__ y, int B, int K, int Kpad,
                                                           float scale, float *__restrict__ dlogits, int ldd,
                                                           float *__restrict__ row_loss, int32_t *__restrict__ row_hit) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int row = blockIdx.x * kXentRows + wid;
  if (row >= B) return;
  const float *s = logits + (size_t)row * ld;
  float *d = dlogits + (size_t)row * ldd;
  const int yy = y[row];
  const bool live = yy >= 0 && yy < K;
  // the row maximum and the lowest index that reaches it (torch.argmax)
  float mx = -INFINITY;
  int at = 0x7fffffff;
  for (int c = lane; c < K; c += 64) {
    const float v = s[c];
    if (v > mx) mx = v, at = c;              // ascending c: the first index of the lane's maximum
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const float om = __shfl_xor(mx, off);
    const int oa = __shfl_xor(at, off);
    if (om > mx || (om == mx && oa < at)) mx = om, at = oa;
  }
  float se = 0.f;
  for (int c = lane; c < K; c += 64) se += expf(s[c] - mx);
  se = wave_sum_f32(se);
  if (live) {
    for (int c = lane; c < K; c += 64) {
      const float p = expf(s[c] - mx) / se;
      d[c] = scale * (p - (c == yy ? 1.f : 0.f));
    }
  } else {
    for (int c = lane; c < K; c += 64) d[c] = 0.f;
  }
  for (int c = K + lane; c < Kpad; c += 64) d[c] = 0.f;
  if (lane == 0) {
    row_loss[row] = live ? (mx - s[yy]) + logf(se) : 0.f;       // lse_i - s_{i, y_i}
    row_hit[row] = (live && at == yy) ? 1 : 0;
  }
}

// out_loss = the row losses added in double: thread t takes the rows t, t + 256, ... in that order, then the 256 partial
// sums are added in thread order.  The count is an integer sum.
__global__ __launch_bounds__(256) void xent_reduce_kernel(const float *__restrict__ row_loss,
                                                          const int32_t *__restrict__ row_hit, int B,
                                                          double *__restrict__ out_loss, int32_t *__restrict__ out_correct) {
  __shared__ double ls[256];
  __shared__ int32_t hs[256];
  const int tid = threadIdx.x;
  double sum = 0.0;
  int32_t hit = 0;
  for (int i = tid; i < B; i += 256) sum += (double)row_loss[i], hit += row_hit[i];
  ls[tid] = sum, hs[tid] = hit;
  __syncthreads();
  if (tid == 0) {
    double total = 0.0;
    int32_t n = 0;
    for (int t = 0; t < 256; ++t) total += ls[t], n += hs[t];
    *out_loss = total;
    *out_correct = n;
  }
}

// -------------------------------------------------------------------------------------------------------------- adamw
struct AdamW {
  double beta1, one_minus_beta1, beta2, one_minus_beta2;
  float decay;             // 1 - lr wd
  float step;              // lr / bias_correction1
  float sqrt_bc2;          // sqrt(bias_correction2)
  float eps;
};

// The two moments are formed in double from the fp32 operands and rounded once: beta1 m and (1 - beta1) g often cancel,
// and an fp32 sum of two rounded products would lose the RELATIVE accuracy of a small result.  The kernel moves 28 bytes
// per element and is bound by them either way.
__device__ __forceinline__ void adamw_one(float &p, float g, float &m, float &v, const AdamW &a) {
  const double gd = (double)g;
  const float mn = (float)(a.beta1 * (double)m + a.one_minus_beta1 * gd);
  const float vn = (float)(a.beta2 * (double)v + a.one_minus_beta2 * (gd * gd));
  const float denom = sqrtf(vn) / a.sqrt_bc2 + a.eps;
  p = p * a.decay - a.step * mn / denom;
  m = mn, v = vn;
}

__global__ __launch_bounds__(256) void adamw_kernel(float *__restrict__ p, const float *__restrict__ g,
                                                    float *__restrict__ m, float *__restrict__ v, long long n, AdamW a) {
  const long long quads = n >> 2;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < quads) {
    f32x4 pp = reinterpret_cast<f32x4 *>(p)[i], mm = reinterpret_cast<f32x4 *>(m)[i], vv = reinterpret_cast<f32x4 *>(v)[i];
    const f32x4 gg = reinterpret_cast<const f32x4 *>(g)[i];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float pe = pp[e], me = mm[e], ve = vv[e];
      adamw_one(pe, gg[e], me, ve, a);
      pp[e] = pe, mm[e] = me, vv[e] = ve;
    }
    reinterpret_cast<f32x4 *>(p)[i] = pp, reinterpret_cast<f32x4 *>(m)[i] = mm, reinterpret_cast<f32x4 *>(v)[i] = vv;
  } else if (i - quads < (n & 3)) {          // the scalar tail
    const long long j = 4 * quads + (i - quads);
    adamw_one(p[j], g[j], m[j], v[j], a);
  }
}

bool aligned16(const void *q) { return ((uintptr_t)q & 15) == 0; }

}  // namespace
}  // namespace lla

using namespace lla;

extern "C" int lla_gemm_f32_nn(const float *dY, int ldy, const float *W, int ldw, const float *H, int ldh, float *dX,
                               int ldx, int M, int N, int K, void *stream) {
  if (M < 0 || N <= 0 || K <= 0 || (N & 3) || (K & 3) || ldy < N || ldw < K || ldx < K || (ldy & 3) || (ldx & 3) ||
      (H && (ldh < K || (ldh & 3))))
    return LLA_EINVAL;
  if (M == 0) return LLA_OK;
  if (!dY || !W || !dX || !aligned16(dY) || !aligned16(dX) || !aligned16(H)) return LLA_EINVAL;
  const long long tiles = (long long)((M + 63) / 64) * ((K + 63) / 64);
  if (tiles > 0x7fffffffLL) return LLA_EINVAL;
  hipStream_t st = as_stream(stream);
  if (H) gemm_f32_nn_kernel<true><<<(int)tiles, 256, 0, st>>>(dY, ldy, W, ldw, H, ldh, dX, ldx, M, N, K);
  else gemm_f32_nn_kernel<false><<<(int)tiles, 256, 0, st>>>(dY, ldy, W, ldw, nullptr, 0, dX, ldx, M, N, K);
  return check_launch();
}

extern "C" int lla_gemm_f32_tn(const float *dY, int ldy, const float *X, int ldx, float *dW, int ldw, float *db, int M,
                               int N, int K, void *stream) {
  if (M < 0 || N <= 0 || K <= 0 || (N & 3) || (K & 3) || ldy < N || ldx < K || ldw < K || (ldy & 3) || (ldx & 3))
    return LLA_EINVAL;
  const int tiles_n = (N + kTnN - 1) / kTnN;
  if (tiles_n > 65535) return LLA_EINVAL;
  if (M == 0) return LLA_OK;
  if (!dY || !X || !dW || !aligned16(dY) || !aligned16(X)) return LLA_EINVAL;
  gemm_f32_tn_kernel<<<dim3((K + kTnK - 1) / kTnK, tiles_n), 256, 0, as_stream(stream)>>>(dY, ldy, X, ldx, dW, ldw, db, M,
                                                                                        N, K);
  return check_launch();
}

extern "C" size_t lla_softmax_xent_workspace_bytes(int B) { return B < 0 ? 0 : (size_t)(B > 0 ? B : 1) * 8; }

extern "C" int lla_softmax_xent(const float *logits, int ld, const int32_t *y, int B, int K, int Kpad, float scale,
                                float *dlogits, int ldd, double *out_loss, int32_t *out_correct, void *workspace,
                                void *stream) {
  if (B < 0 || K < 1 || K > 1024 || Kpad < K || ld < K || ldd < Kpad) return LLA_EINVAL;
  if (B == 0) return LLA_OK;
  if (!logits || !y || !dlogits || !out_loss || !out_correct || !workspace || ((uintptr_t)workspace & 3))
    return LLA_EINVAL;
  float *row_loss = static_cast<float *>(workspace);
  int32_t *row_hit = reinterpret_cast<int32_t *>(row_loss + B);
  hipStream_t st = as_stream(stream);
  softmax_xent_kernel<<<(B + kXentRows - 1) / kXentRows, 256, 0, st>>>(logits, ld, y, B, K, Kpad, scale, dlogits, ldd,
                                                                       row_loss, row_hit);
  xent_reduce_kernel<<<1, 256, 0, st>>>(row_loss, row_hit, B, out_loss, out_correct);
  return check_launch();
}

extern "C" int lla_adamw_step(float *p, const float *g, float *m, float *v, long long n, double lr, double beta1,
                              double beta2, double eps, double weight_decay, double bias_correction1,
                              double bias_correction2, void *stream) {
  if (n < 0 || !(lr >= 0.0) || !(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0) || !(eps >= 0.0) ||
      !(weight_decay >= 0.0) || !(bias_correction1 > 0.0) || !(bias_correction2 > 0.0))
    return LLA_EINVAL;
  if (n == 0) return LLA_OK;
  if (!p || !g || !m || !v || !aligned16(p) || !aligned16(g) || !aligned16(m) || !aligned16(v)) return LLA_EINVAL;
  const long long threads = (n >> 2) + (n & 3);
  const long long blocks = (threads + 255) / 256;
  if (blocks > 0x7fffffffLL) return LLA_EINVAL;
  const AdamW a = {beta1, 1.0 - beta1, beta2, 1.0 - beta2, (float)(1.0 - lr * weight_decay),
                   (float)(lr / bias_correction1), (float)sqrt(bias_correction2), (float)eps};
  adamw_kernel<<<(int)blocks, 256, 0, as_stream(stream)>>>(p, g, m, v, n, a);
  return check_launch();
}
