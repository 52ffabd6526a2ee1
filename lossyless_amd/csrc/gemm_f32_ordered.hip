// fp32 Linear layers with a DEFINED arithmetic: C[M][N] = act(A[M][K] W[N][K]^T + bias), every output one fma chain.
//
// THE CONTRACT (lla_gemm_f32_ordered_host in host.cpp runs the same chain; include/lossyless_amd.h repeats it).  For every
// output element (m, n), whatever M, the grid, the tile or the row offset of the call:
//     acc = +0.0f
//     for k = 0, 1, ..., K-1 (ascending; the K that was passed in, padding columns included):
//         acc = fmaf(A[m][k], W[n][k], acc)        one IEEE-754 binary32 fused multiply-add, round to nearest even
//     y = acc + bias[n]                            one rounded binary32 add; skipped when bias == NULL
//     y = y > 0.f ? y : 0.f                        when relu (a NaN and -0.0f give +0.0f)
//     C[m][n] = y
// fp32 denormals are operands and results like any other value (the kernel runs in hipcc's default mode, which keeps
// them); no product, partial sum or chain is split over lanes or re-associated.
//
// Why it exists: the hyperprior's z_encoder picks the coding-table row of every element, so its values are part of the
// bitstream's contract (lossyless/rates.py:687-699).  lla_gemm_f32 (gemm_f32.hip) is an fma chain too, but in the K order
// of the matrix unit's operand layout, which nothing documents and a CPU cannot be asked to follow; this order a dozen
// lines of C++ reproduce bit for bit, so a container written here can be read on a machine with no GPU.
//
// Shape of the work: 512-wide layers, 1 .. 8 704 rows; 0.84 M multiply-adds per image through z_encoder, far below what the
// VALU offers, so this is a plain SGEMM: a 256-thread workgroup per 64 x 64 output tile, A and W staged through LDS in
// chunks of 32 k (transposed: [k][row], so that a thread reads its 4 rows and its 4 columns of one k as one 16-byte
// word each), a 4 x 4 register tile of independent chains per thread, k walked upwards across the chunks.  Rows and
// columns beyond M / N are computed on clamped addresses and not stored.
#include "common.h"

namespace lla {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kTile = 64;   // output rows and columns per workgroup
constexpr int kChunk = 32;  // k per LDS stage

template <bool RELU>
__global__ __launch_bounds__(256) void gemm_f32_ordered_kernel(const float *__restrict__ A, int lda,
                                                               const float *__restrict__ W, int ldw,
                                                               const float *__restrict__ bias, float *__restrict__ C,
                                                               int ldc, int M, int N, int K) {
  __shared__ __attribute__((aligned(16))) float As[kChunk][kTile];
  __shared__ __attribute__((aligned(16))) float Ws[kChunk][kTile];
  const int tid = threadIdx.x;
  const int tiles_n = (N + kTile - 1) / kTile;
  const int tm = blockIdx.x / tiles_n, tn = blockIdx.x - tm * tiles_n;
  const int m0 = tm * kTile, n0 = tn * kTile;

  // staging: thread -> (row of the tile, two 4-k quads of the chunk); a wave writes 64 consecutive LDS words per k
  const int srow = tid & 63, sq = tid >> 6;
  const float *ap = A + (size_t)min(m0 + srow, M - 1) * lda + 4 * sq;
  const float *wp = W + (size_t)min(n0 + srow, N - 1) * ldw + 4 * sq;
  f32x4 ra[2] = {}, rw[2] = {};
  auto fetch = [&](int k0) {
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const int k = k0 + 4 * sq + 16 * r;
      if (k < K) {     // (K % 8 == 0: a quad is inside or outside)
        ra[r] = *reinterpret_cast<const f32x4 *>(ap + k0 + 16 * r);
        rw[r] = *reinterpret_cast<const f32x4 *>(wp + k0 + 16 * r);
      }
    }
  };
  auto park = [&]() {   // (quads beyond K hold an earlier chunk's values: the walk below stops at K)
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        As[4 * sq + 16 * r + j][srow] = ra[r][j];
        Ws[4 * sq + 16 * r + j][srow] = rw[r][j];
      }
  };

  const int tx = tid & 15, ty = tid >> 4;   // columns n0 + 4 tx .. + 3, rows m0 + 4 ty .. + 3
  float acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;

  fetch(0);
  for (int k0 = 0; k0 < K; k0 += kChunk) {
    park();
    __syncthreads();
    if (k0 + kChunk < K) fetch(k0 + kChunk);   // in flight under this chunk's arithmetic
    const int kc = min(kChunk, K - k0);        // a multiple of 8
    for (int kb = 0; kb < kc; kb += 8) {
#pragma unroll
      for (int kk = 0; kk < 8; ++kk) {
        const f32x4 a = *reinterpret_cast<const f32x4 *>(&As[kb + kk][4 * ty]);
        const f32x4 w = *reinterpret_cast<const f32x4 *>(&Ws[kb + kk][4 * tx]);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_fmaf(a[i], w[j], acc[i][j]);
      }
    }
    __syncthreads();
  }

  const int nc = n0 + 4 * tx;
  if (nc >= N) return;     // N % 4 == 0: a quad is inside or outside
  f32x4 b = {0.f, 0.f, 0.f, 0.f};
  if (bias) b = *reinterpret_cast<const f32x4 *>(bias + nc);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int m = m0 + 4 * ty + i;
    if (m >= M) break;
    f32x4 v = {acc[i][0], acc[i][1], acc[i][2], acc[i][3]};
    if (bias) v += b;      // (-ffp-contract=off: one rounded add, fused with nothing)
    if (RELU) {
#pragma unroll
      // (selected on the bits: written on floats the compiler makes it a v_max_f32, and the contract should not rest on
      // which zero that instruction returns for max(+0, -0))
      for (int e = 0; e < 4; ++e) {
        const float y = v[e];   // (a scalar first: __builtin_bit_cast of a vector ELEMENT lvalue reads element 0)
        v[e] = __builtin_bit_cast(float, y > 0.f ? __builtin_bit_cast(int, y) : 0);
      }
    }
    *reinterpret_cast<f32x4 *>(C + (size_t)m * ldc + nc) = v;
  }
}

inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace
}  // namespace lla

using namespace lla;

extern "C" int lla_gemm_f32_ordered(const float *A, int lda, const float *W, int ldw, const float *bias, float *C,
                                    int ldc, int M, int N, int K, int relu, void *stream) {
  if (M < 0 || N <= 0 || K <= 0 || (K & 7) || (N & 3) || lda < K || ldw < K || ldc < N || (lda & 3) ||
      (ldw & 3) || (ldc & 3))
    return LLA_EINVAL;
  if (M == 0) return LLA_OK;
  if (!A || !W || !C || !aligned16(A) || !aligned16(W) || !aligned16(C) || !aligned16(bias)) return LLA_EINVAL;
  const long long tiles = (long long)((M + kTile - 1) / kTile) * ((N + kTile - 1) / kTile);
  if (tiles > 0x7fffffffLL) return LLA_EINVAL;
  hipStream_t st = as_stream(stream);
  if (relu) gemm_f32_ordered_kernel<true><<<(int)tiles, 256, 0, st>>>(A, lda, W, ldw, bias, C, ldc, M, N, K);
  else gemm_f32_ordered_kernel<false><<<(int)tiles, 256, 0, st>>>(A, lda, W, ldw, bias, C, ldc, M, N, K);
  return check_launch();
}
