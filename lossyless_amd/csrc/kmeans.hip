// One Lloyd iteration of k-means on the compressed representations (gfx950): the unsupervised protocol for judging frozen
// features (cluster, then score the clusters against the labels by NMI / ARI / purity: DeepCluster, Caron et al. 2018;
// SCAN, Van Gansbeke et al. 2020) and the way to build codebooks or pseudo-labels from a container that stays compressed.
// The reference has no clustering; the rows come from a decode group of CompressedLatents / HyperpriorLatents, as in probe.hip.
//
//   n2_i = sum_c z_ic^2
//   metric 0 (Euclidean):  s_ik = z_i . W_k + b_k              w_i = 1      dist_i = max(0, n2_i - 2 s_i,a_i)
//   metric 1 (spherical):  s_ik = (z_i . W_k) r_i + b_k        w_i = r_i    dist_i = 1 - s_i,a_i        r_i = 1 / sqrt(n2_i)
//   a_i = argmax_k s_ik (the lowest k on ties)      out_sum[k] = sum_{i: a_i = k} w_i z_i      out_count[k] = |{i: a_i = k}|
// With W = the centres and b_k = -1/2 |c_k|^2 the argmax is the nearest centre and dist its squared distance.
//
// The walk is probe.hip's (lla_svm_pass / lla_softmax_pass) with another step 3: steps 1, 2 and 4 are row_tile.h's.  A
// persistent workgroup (4 waves) owns one tile of 32 centroids and walks row tiles of 32 rows:
//   1. the row tile is staged in LDS once, as fp32 (fp16 rows are widened exactly), pitch C + 4 floats; eight threads per
//      row take the row's sum of squares over their columns, in an order fixed by C (as knn.hip: row_tile.h);
//   2. scores: S[32 centroids][32 rows] = W_tile Z_tile^T on v_mfma_f32_32x32x2_f32, the C dimension dealt to the four waves
//      in groups of 8 and their partial tiles added through LDS in a fixed order ((w0 + w2) + (w1 + w3));
//   3. assignment: one thread per row scans the K real centroids of the tile in ascending order with a strict >, writes
//      out_assign / out_dist and leaves (a_i, w_i) in LDS: the one-hot residual w_i [k == a_i] is never stored as a matrix;
//   4. sums: G[32 centroids][C] += R^T Z_tile, probe.hip's second MFMA with the residual formed from (a_i, w_i); each
//      wave keeps its C / 4 columns of the slice in accumulator registers over ALL its row tiles.
// Scores never leave the chip.  LDS: 32 (C + 4) + 2 * 1024 + 384 floats -- 74 KB at C = 512: two workgroups per CU.
//
// K <= 32: that one kernel; z is read once.  K > 32: kmeans_assign_kernel first -- the same staging and the same score MFMA
// over ALL centroid tiles of a row tile, a running (best, index) per thread over its centroids in ascending order, merged per
// row in a fixed order that keeps the lowest index on ties (the shape of softmax_rows_kernel) -- then the sums walk per
// centroid tile with a_i read from out_assign: steps 1, 3 and 4, no score MFMA.
//
// Cost model.  The assign kernel reads z once and W once per row-tile walker.  The sums walk for K > 32 reads z once per
// centroid tile, ceil(K / 32) times in all, and spends 32 x the flops a segmented sum would need on the one-hot MFMA: the
// cost of an lla_svm_pass at the same K.  At K = 1000 and C = 512 that is 32 reads of z (from L2 / MALL for a decode group
// that fits there) against the 1 a sort-based segmented sum would take; that variant is not built.
//
// Determinism: a score's bits depend on (z_i, W_k, b_k, C, metric) alone -- the MFMA chain of a wave runs over its column
// groups in ascending order, the four partial tiles and the eight partial sums of squares are added in a fixed order, the
// scaling and the add of b are one fp32 operation each (-ffp-contract=off), and both paths run the same code -- not on where
// the row falls in a tile, a call or a walker's range: the assignment is a pure function of the rows and the centroids.  No
// floating-point atomics (the counts are integers): every workgroup writes its partial sums to the workspace and
// kmeans_reduce_kernel adds them in workgroup order, counts and statistics in double; the number of workgroups is a function
// of (B, K) alone, so two calls on the same inputs give the same bits.
#include "row_tile.h"

namespace lla {
namespace {

// what a pass kernel does: everything (K <= 32), steps 1-3 only (K <= 32, predict), steps 1, 3, 4 from out_assign (K > 32)
enum { kFused = 0, kPredict = 1, kSumsOnly = 2 };

// Zs, two score slots, Np [32 rows][8], then b [32], a [32], w [32], count [32]
__host__ __device__ inline int lds_floats(int C) { return kRows * (C + kZPad) + 2 * kRows * kClasses + kRows * 8 + 4 * kClasses; }

// THE score of (row rr of the staged tile, centroid cl of the scored tile): both paths read it here, so that its bits are
// a function of (z_i, W_k, b_k, C, metric) alone
__device__ __forceinline__ float score_of(const float *Sp, int cl, int rr, float rinv, int cosine, float bk) {
  float sc = Sp[cl * kRows + rr] + Sp[kRows * kClasses + cl * kRows + rr];
  if (cosine) sc *= rinv;
  return sc + bk;
}

__device__ __forceinline__ float dist_of(float n2, float best, int cosine) {
  return cosine ? 1.f - best : fmaxf(0.f, n2 - 2.f * best);
}

// the 32 row threads' two running totals -> part_stats[2] of this workgroup, added in row order (Dp: 64 doubles of LDS)
__device__ __forceinline__ void store_stats(double *Dp, double dsum, double nsum, double *__restrict__ part_stats, int tid) {
  if (tid < kRows) Dp[tid] = dsum, Dp[kRows + tid] = nsum;
  __syncthreads();
  if (tid < 2) {
    double sum = 0.0;
    for (int r = 0; r < kRows; ++r) sum += Dp[tid * kRows + r];
    part_stats[tid] = sum;
  }
}

// NT: 32-column tiles of the sums slice per wave (C <= 128 NT).  MODE: kFused, kPredict or kSumsOnly (above).
// Workspace: part_W [centroid tile][walker][32][C], part_cnt [centroid tile][walker][32], part_stats [workgroup][2].
template <int NT, int MODE>
__global__ __launch_bounds__(256) void kmeans_pass_kernel(const void *__restrict__ z, int z_f16, int ld_z, int B, int C,
                                                          const float *__restrict__ W, const float *__restrict__ bias,
                                                          int K, int ld_w, int cosine, int32_t *__restrict__ assign,
                                                          float *__restrict__ dist, float *__restrict__ part_W,
                                                          int32_t *__restrict__ part_cnt, double *__restrict__ part_stats) {
  extern __shared__ __align__(16) float lds[];
  constexpr bool SCORE = MODE != kSumsOnly, SUMS = MODE != kPredict;
  const int pitch = C + kZPad;
  float *Zs = lds;                             // [32 rows][pitch]
  float *Sp = Zs + kRows * pitch;              // [slot][32 centroids][32 rows]
  float *Np = Sp + 2 * kRows * kClasses;       // [32 rows][8] partial sums of squares
  float *Bs = Np + kRows * 8;                  // b of the tile's centroids
  int *Ai = reinterpret_cast<int *>(Bs + kClasses);      // a_i of the staged rows (-1: no row)
  float *Wi = Bs + 2 * kClasses;               // w_i
  int *Cnt = reinterpret_cast<int *>(Bs + 3 * kClasses); // rows this workgroup gave to each centroid of its tile

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int r32 = lane & 31, hk = lane >> 5;
  const int ct = blockIdx.y, P = gridDim.x, p = blockIdx.x;
  const int k0 = ct * kClasses;
  const int nreal = K - k0 < kClasses ? K - k0 : kClasses;

  int n = k0 + r32;
  if (n >= K) n = K - 1;                       // clamped centroids are computed and never scanned
  const float *wp = W + (size_t)n * ld_w + 4 * hk;
  if (tid < kClasses) {                        // (visible after the barrier that follows the first staging)
    Bs[tid] = (SCORE && tid < nreal) ? bias[k0 + tid] : 0.f;
    Cnt[tid] = 0;
  }

  f32x16 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
  double dsum = 0.0, nsum = 0.0;               // row threads: sum of dist_i and of n2_i over this workgroup's rows

  const int ntiles = (B + kRows - 1) / kRows;
  for (int tile = p; tile < ntiles; tile += P) {
    const int row0 = tile * kRows;
    stage_rows(Zs, z, z_f16, ld_z, row0, B, C, tid);                 // 1.
    __syncthreads();
    if (SCORE || cosine) row_squares(Zs, Np, C, tid);
    if constexpr (SCORE) tile_scores<false>(Zs, Sp, wp, nullptr, C, lane, wid);      // 2.
    else __syncthreads();

    if (tid < kRows) {                                               // 3. one thread per row
      const bool row_ok = row0 + tid < B;
      const float n2 = (SCORE || cosine) ? row_n2(Np, tid) : 0.f;
      const float rinv = cosine ? inv_norm(n2) : 1.f;
      int a = -1;
      if constexpr (SCORE) {
        float best = score_of(Sp, 0, tid, rinv, cosine, Bs[0]);
        a = 0;
        for (int cl = 1; cl < nreal; ++cl) {
          const float sc = score_of(Sp, cl, tid, rinv, cosine, Bs[cl]);
          if (sc > best) best = sc, a = cl;
        }
        if (row_ok) {
          const float d = dist_of(n2, best, cosine);
          assign[row0 + tid] = a, dist[row0 + tid] = d;
          dsum += (double)d, nsum += (double)n2;
        } else {
          a = -1;
        }
      } else if (row_ok) {
        a = assign[row0 + tid] - k0;
      }
      const bool mine = a >= 0 && a < kClasses;
      Ai[tid] = mine ? a : -1;
      Wi[tid] = rinv;
      if (SUMS && mine) atomicAdd(&Cnt[a], 1);                      // (an integer: the order does not matter)
    }
    if constexpr (SUMS) {
      __syncthreads();
      // 4. sums slice: "A" lane l = w_i [a_i == l & 31] of row 2 s + (l >> 5)
      slice_mfma(acc, Zs, [&](int row) { return Ai[row] == r32 ? Wi[row] : 0.f; }, C, lane, wid);
      __syncthreads();                           // the next tile's staging overwrites Zs, and step 3 Ai and Wi
    }
    // (kPredict: the next tile's staging writes Zs only, which step 3 does not read; a barrier follows it before Np and Sp
    // are written again)
  }

  if constexpr (SUMS) {
    // this workgroup's partial sums -> workspace (centroids beyond K hold exact zeros and are never read)
    slice_store(acc, part_W + (size_t)(ct * P + p) * kClasses * C, C, lane, wid);
    if (tid < kClasses) part_cnt[(size_t)(ct * P + p) * kClasses + tid] = Cnt[tid];     // (behind the loop's last barrier)
  }
  if constexpr (MODE == kFused) store_stats(reinterpret_cast<double *>(Sp), dsum, nsum, part_stats + 2 * (size_t)p, tid);
}

// The assignment over more than one centroid tile.  A persistent workgroup stages a row tile as step 1 does and takes the
// scores of every centroid tile with the MFMA of step 2 and score_of (the bits the one-kernel path sees).  Thread (row, q)
// sees centroids q + 8 j of every tile, in ascending order, and keeps its best with a strict >: the lowest index among its
// own maxima.  The eight partial (best, index) of a row are merged once per row tile: the larger score, the lower index
// between equal scores -- the lowest index among all maxima, whatever the order of the merge.  The grid is a function of B
// alone.  part_stats == NULL (predict only): no statistics are kept.
__global__ __launch_bounds__(256) void kmeans_assign_kernel(const void *__restrict__ z, int z_f16, int ld_z, int B, int C,
                                                            const float *__restrict__ W, const float *__restrict__ bias,
                                                            int K, int ld_w, int cosine, int32_t *__restrict__ assign,
                                                            float *__restrict__ dist, double *__restrict__ part_stats) {
  extern __shared__ __align__(16) float lds[];
  float *Zs = lds;
  float *Sp = Zs + kRows * (C + kZPad);
  float *Np = Sp + 2 * kRows * kClasses;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int r32 = lane & 31, hk = lane >> 5;
  const int rr = tid & 31, cl0 = tid >> 5;
  const int nct = (K + kClasses - 1) / kClasses, ntiles = (B + kRows - 1) / kRows;
  double dsum = 0.0, nsum = 0.0;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int row0 = tile * kRows;
    stage_rows(Zs, z, z_f16, ld_z, row0, B, C, tid);
    __syncthreads();
    row_squares(Zs, Np, C, tid);                 // (read after the barriers of the first tile_scores)
    float best = 0.f, n2 = 0.f, rinv = 1.f;
    int at = 0;
    for (int ct = 0; ct < nct; ++ct) {
      const int k0 = ct * kClasses;
      int n = k0 + r32;
      if (n >= K) n = K - 1;
      float bk[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {              // (asked for before the MFMAs, used after them)
        const int c = k0 + cl0 + 8 * j;
        bk[j] = c < K ? bias[c] : 0.f;
      }
      tile_scores<false>(Zs, Sp, W + (size_t)n * ld_w + 4 * hk, nullptr, C, lane, wid);
      if (ct == 0) {
        n2 = row_n2(Np, rr);
        rinv = cosine ? inv_norm(n2) : 1.f;
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int cl = cl0 + 8 * j, k = k0 + cl;
        if (k < K) {
          const float sc = score_of(Sp, cl, rr, rinv, cosine, bk[j]);
          if (k == cl0 || sc > best) best = sc, at = k;        // (k == cl0: the thread's first centroid, always a real one)
        }
      }
      __syncthreads();                           // the next centroid tile's scores (or the merge) overwrite Sp
    }
    Sp[cl0 * kRows + rr] = best;
    reinterpret_cast<int *>(Sp)[(8 + cl0) * kRows + rr] = at;
    __syncthreads();
    if (tid < kRows && row0 + tid < B) {
      float top = Sp[tid];
      int a = reinterpret_cast<const int *>(Sp)[8 * kRows + tid];
      for (int q = 1; q < 8; ++q) {
        const float v = Sp[q * kRows + tid];
        const int i = reinterpret_cast<const int *>(Sp)[(8 + q) * kRows + tid];
        if (v > top || (v == top && i < a)) top = v, a = i;
      }
      const float d = dist_of(n2, top, cosine);  // (tid < 32: rr == tid)
      assign[row0 + tid] = a, dist[row0 + tid] = d;
      dsum += (double)d, nsum += (double)n2;
    }
    __syncthreads();                             // the next tile's row_squares and scores overwrite Np and Sp
  }
  if (part_stats) store_stats(reinterpret_cast<double *>(Sp), dsum, nsum, part_stats + 2 * (size_t)blockIdx.x, tid);
}

// out (+)= the partial sums of walkers 0 .. P-1, in that order.  One thread per (centroid, column); column C of a centroid
// is its count; the last two threads take the statistics of the nstat workgroups that kept them.
__global__ __launch_bounds__(64) void kmeans_reduce_kernel(const float *__restrict__ part_W,
                                                           const int32_t *__restrict__ part_cnt,
                                                           const double *__restrict__ part_stats, int P, int nstat, int C,
                                                           int K, int ld_w, float *__restrict__ out_sum,
                                                           double *__restrict__ out_count, double *__restrict__ out_stats,
                                                           int accumulate) {
  const long long idx = (long long)blockIdx.x * 64 + threadIdx.x, n_out = (long long)K * (C + 1);
  if (idx >= n_out + 2) return;
  if (idx >= n_out) {
    const int s = (int)(idx - n_out);
    const double sum = ordered_sum<double>(part_stats + s, 2, nstat);
    out_stats[s] = accumulate ? out_stats[s] + sum : sum;
    return;
  }
  const int k = (int)(idx / (C + 1)), c = (int)(idx - (long long)k * (C + 1));
  const int ct = k / kClasses, i = k - ct * kClasses;
  if (c < C) {
    const float sum = ordered_sum<float>(part_W + ((size_t)ct * P * kClasses + i) * C + c, (size_t)kClasses * C, P);
    float *o = out_sum + (size_t)k * ld_w + c;
    *o = accumulate ? *o + sum : sum;
  } else {
    const double sum = ordered_sum<double>(part_cnt + (size_t)ct * P * kClasses + i, kClasses, P);
    out_count[k] = accumulate ? out_count[k] + sum : sum;
  }
}

template <int MODE>
const void *pass_kernel(int C) {
  if (C <= 128) return reinterpret_cast<const void *>(&kmeans_pass_kernel<1, MODE>);
  if (C <= 256) return reinterpret_cast<const void *>(&kmeans_pass_kernel<2, MODE>);
  if (C <= 512) return reinterpret_cast<const void *>(&kmeans_pass_kernel<4, MODE>);
  return reinterpret_cast<const void *>(&kmeans_pass_kernel<8, MODE>);
}

bool shape_ok(int C, int K) { return cols_ok(C) && K >= 1 && class_tiles(K) <= 65535; }

// floats of partial sums and counts: [centroid tile][walker][32][C + 1]
size_t partial_floats(int C, int K) {
  const int nct = class_tiles(K);
  return (size_t)nct * tile_walkers(nct) * kClasses * (C + 1);
}

}  // namespace
}  // namespace lla

using namespace lla;

extern "C" size_t lla_kmeans_pass_workspace_bytes(int C, int K) {
  if (!shape_ok(C, K)) return 0;
  return partial_floats(C, K) * sizeof(float) + (size_t)kResident * 2 * sizeof(double);
}

extern "C" int lla_kmeans_pass(const void *z, int z_dtype, int ld_z, int B, int C, const float *W, const float *b, int K,
                               int ld_w, int metric, int32_t *out_assign, float *out_dist, float *out_sum,
                               double *out_count, double *out_stats, int accumulate, void *workspace, void *stream) {
  if (!shape_ok(C, K) || !rows_ok(z, z_dtype, ld_z, B, C) || ld_w < C || (ld_w & 3) || (metric != 0 && metric != 1))
    return LLA_EINVAL;
  if (!W || !b || !out_assign || !out_dist || !workspace || (out_sum && (!out_count || !out_stats))) return LLA_EINVAL;
  if (((uintptr_t)W & 15) || ((uintptr_t)out_sum & 15) || ((uintptr_t)workspace & 15) ||
      ((uintptr_t)out_assign & 3) || ((uintptr_t)out_dist & 3) || ((uintptr_t)out_count & 7) || ((uintptr_t)out_stats & 7))
    return LLA_EINVAL;
  if (B == 0 && (accumulate || !out_sum)) return LLA_OK;

  const int nct = class_tiles(K), ntiles = (B + kRows - 1) / kRows;
  const int pmax = tile_walkers(nct);
  const int P = ntiles < pmax ? ntiles : pmax;                         // walkers of the pass kernel
  const int A = ntiles < kResident ? ntiles : kResident;               // workgroups of the assign kernel
  float *part_W = static_cast<float *>(workspace);
  int32_t *part_cnt = reinterpret_cast<int32_t *>(part_W + (size_t)nct * pmax * kClasses * C);
  double *part_stats = reinterpret_cast<double *>(part_cnt + (size_t)nct * pmax * kClasses);
  hipStream_t st = as_stream(stream);
  const size_t lds_bytes = (size_t)lds_floats(C) * sizeof(float);
  const int z_f16 = z_dtype == LLA_Z_F16, sums = out_sum != nullptr;
  if (B > 0) {
    const void *kernel = nct > 1 ? pass_kernel<kSumsOnly>(C) : sums ? pass_kernel<kFused>(C) : pass_kernel<kPredict>(C);
    const void *assign_kernel = reinterpret_cast<const void *>(&kmeans_assign_kernel);
    if (lds_bytes > dynamic_lds_limit(kernel) || (nct > 1 && lds_bytes > dynamic_lds_limit(assign_kernel))) return LLA_ECAP;
    if (nct > 1) {
      double *stats = sums ? part_stats : nullptr;
      void *args[] = {(void *)&z, (void *)&z_f16, (void *)&ld_z, (void *)&B, (void *)&C, (void *)&W, (void *)&b, (void *)&K,
                      (void *)&ld_w, (void *)&metric, (void *)&out_assign, (void *)&out_dist, (void *)&stats};
      hipError_t e = hipLaunchKernel(assign_kernel, dim3(A), dim3(256), args, lds_bytes, st);
      if (e != hipSuccess) return hip_fail(e);
    }
    if (nct == 1 || sums) {
      void *args[] = {(void *)&z, (void *)&z_f16, (void *)&ld_z, (void *)&B, (void *)&C, (void *)&W, (void *)&b, (void *)&K,
                      (void *)&ld_w, (void *)&metric, (void *)&out_assign, (void *)&out_dist, (void *)&part_W,
                      (void *)&part_cnt, (void *)&part_stats};
      hipError_t e = hipLaunchKernel(kernel, dim3(P, nct), dim3(256), args, lds_bytes, st);
      if (e != hipSuccess) return hip_fail(e);
    }
  }
  if (!sums) return LLA_OK;
  const long long n_out = (long long)K * (C + 1) + 2;
  kmeans_reduce_kernel<<<(unsigned)((n_out + 63) / 64), 64, 0, st>>>(part_W, part_cnt, part_stats, P, nct > 1 ? A : P, C, K,
                                                                        ld_w, out_sum, out_count, out_stats, accumulate);
  return check_launch();
}
