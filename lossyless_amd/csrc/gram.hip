// The second moments of the compressed representations in one pass (gfx950): what a ridge probe on frozen features needs
// (scikit-learn's Ridge / RidgeClassifier; the reference fits only iterative predictors and has no closed-form one).  The
// statistics do not depend on the penalty and add over rows, so one walk of a container gives every (alpha, fold) of a search.
//
//   out_gram  [C][C] = sum_i z_i z_i^T          out_sum [C] = sum_i z_i
//   out_cross [T][C] = sum_i t_i z_i^T          out_tsum [T] = sum_i t_i          out_tsq [T] = sum_i t_i^2        (t != NULL)
//   lla_segment_sums:  out [S][C] = sum_{i in segment s} z_i    -- what a one-hot target matrix would give for class labels
//
// lla_gram_pass is one kernel and one reduction.  The grid is (tiles, walkers).  The first nt (nt + 1) / 2 tiles, nt =
// ceil(C / 128), are the upper-triangular 128 x 128 tiles (ti <= tj) of the Gram matrix; the others are the 32-target x
// 128-column tiles of the cross-moments.  Walker p of P takes the 32-row chunks p, p + P, ... : at any moment all the
// tiles of a walker, and all walkers, read one window of P chunks, so that z comes from HBM about once and the panels the
// other tiles of the same rows re-read come from L2 / MALL.
//   Gram tile (4 waves): the two column panels [32 rows][128] of a chunk are staged in LDS as fp32 (fp16 rows are widened
//     exactly), pitch 128 + kZPad floats; a diagonal tile stages one panel.  Wave (wr, wc) owns the 64 x 64 quarter as four
//     32 x 32 accumulators kept in registers over ALL its rows: per pair of rows two A reads, two B reads (ds_read_b32,
//     consecutive columns per half-wave: no bank conflict) and four v_mfma_f32_32x32x2_f32 -- 64 accumulator registers,
//     32 for the next chunk's rows, which are loaded before the MFMAs of this one and stored after them.  The 32 x 32 blocks
//     below the diagonal of a diagonal tile are not computed (6 of its 16): wave (1, 0) idles, waves (0, 0) and (1, 1) run
//     three blocks and wave (0, 1) all four, so a diagonal tile takes as long as any other.  A diagonal tile also adds its
//     panel's columns, in double: thread (column, half) takes rows 16 half .. 16 half + 15 of every chunk in row order.
//   Cross tile: one panel and the chunk's [32 rows][32 targets]; wave w owns columns 32 w .. 32 w + 31 as one accumulator.
//     The cross tiles of panel 0 also add t and t^2 per target, in double, two halves of 16 rows as above.
//   Every workgroup writes its fp32 partial tile and its double partial sums to the workspace; gram_reduce_kernel adds the
//   walkers' partials in walker order in double (halves in order within a walker), adds into or writes the output, and writes
//   the mirrored element out_gram[d][c] from the value it wrote to out_gram[c][d].
// LDS: 2 x 32 x 132 floats = 33 KB; 96 VGPRs + 64 AGPRs, no scratch: three waves per SIMD by registers; the grid is cut to
// kResident = 512 workgroups, two per CU.
//
// Cost model.  In time, nt (nt + 1) / 2 tiles of 128 x 128 x B fp32 multiply-adds (C = 512: 10 of 16, 0.63 of z^T z), since a
// diagonal tile's busiest wave runs all four blocks; in MFMA work executed, 0.53 of z^T z at C = 512 (136 of 256 blocks).  +
// a quarter tile per (panel, 32 targets); z from HBM once; the partials cost at most 512 x 64 KB written and read once.
// Walkers are kResident / tiles: beyond 512 tiles (C = 1024: more than 1900 targets) every tile has ONE walker -- a chain as
// long as the call's rows and no row parallelism inside a tile; T is capped at kMaxTargets = 4096 (grid and workspace size).
//
// Determinism: no floating-point atomics; a walker's chain runs over its chunks in ascending order, the number of walkers is
// a function of (B, C, T) alone and the reduction is ordered: the same inputs give the same bits, and out_gram is symmetric
// bit for bit.  An fp32 chain is never longer than the call's rows; what joins chains is double.
//
// lla_segment_sums: one workgroup per (segment, 128 columns), 8 row lanes x 32 threads of four columns.  Lane l adds rows
// l, l + 8, ... of the segment in row order in double; the eight lanes are then added in lane order.  No workspace.
#include "row_tile.h"      // kRows (a chunk), kZPad, kResident, the checks of the rows and the ordered sum

namespace lla {
namespace {

constexpr int kTile = 128;            // columns per panel: the edge of a Gram tile
constexpr int kTargets = 32;          // targets per cross tile
constexpr int kPitch = kTile + kZPad;
constexpr int kTPitch = kTargets + kZPad;
constexpr int kMaxTargets = 4096;
constexpr int kSegBatch = 256;        // segments per launch of segment_sums_kernel (their offsets travel as an argument)
constexpr int kSegLanes = 8;

struct Plan {
  int nt, ntri, ntt, tiles, pmax;
};

inline bool shape_ok(int C, int T) { return cols_ok(C) && T >= 0 && T <= kMaxTargets; }

inline Plan plan_of(int C, int T) {
  Plan pl;
  pl.nt = (C + kTile - 1) / kTile;
  pl.ntri = pl.nt * (pl.nt + 1) / 2;
  pl.ntt = (T + kTargets - 1) / kTargets;
  pl.tiles = pl.ntri + pl.nt * pl.ntt;
  pl.pmax = tile_walkers(pl.tiles);
  return pl;
}

// this thread's four float4 of the panel [32 rows][128 columns from col0] of the chunk at row0: rows beyond B and columns
// beyond C are zeros
__device__ __forceinline__ void load_panel(f32x4 (&v)[4], const void *__restrict__ z, int z_f16, int ld_z, int row0, int B,
                                           int col0, int C, int tid) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int i = tid + 256 * k, row = i >> 5, col = col0 + 4 * (i & 31);
    v[k] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (row0 + row < B && col < C) {
      const size_t at = (size_t)(row0 + row) * ld_z + col;
      if (z_f16) {
        const uint2 raw = *reinterpret_cast<const uint2 *>(static_cast<const __half *>(z) + at);
        const __half2 lo = __builtin_bit_cast(__half2, raw.x), hi = __builtin_bit_cast(__half2, raw.y);
        v[k] = f32x4{__low2float(lo), __high2float(lo), __low2float(hi), __high2float(hi)};
      } else {
        v[k] = *reinterpret_cast<const f32x4 *>(static_cast<const float *>(z) + at);
      }
    }
  }
}

__device__ __forceinline__ void store_panel(float *Ps, const f32x4 (&v)[4], int tid) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int i = tid + 256 * k;
    *reinterpret_cast<f32x4 *>(Ps + (i >> 5) * kPitch + 4 * (i & 31)) = v[k];
  }
}

// this thread's four values of the targets [32 rows][32 targets from t0] of the chunk at row0 (zeros beyond B and T)
__device__ __forceinline__ void load_targets(float (&v)[4], const float *__restrict__ t, int ld_t, int row0, int B, int t0,
                                             int T, int tid) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int i = tid + 256 * k, row = i >> 5, tc = t0 + (i & 31);
    v[k] = (row0 + row < B && tc < T) ? t[(size_t)(row0 + row) * ld_t + tc] : 0.f;
  }
}

__device__ __forceinline__ void store_targets(float *Ts, const float (&v)[4], int tid) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int i = tid + 256 * k;
    Ts[(i >> 5) * kTPitch + (i & 31)] = v[k];
  }
}

// upper-triangular tile q of nt x nt, rows first: (0, 0), (0, 1), ... (0, nt - 1), (1, 1), ...
__device__ __forceinline__ void tile_of(int q, int nt, int &ti, int &tj) {
  ti = 0;
  while (q >= nt - ti) q -= nt - ti, ++ti;
  tj = ti + q;
}

__device__ __forceinline__ void gram_tile(float *lds, const void *__restrict__ z, int z_f16, int ld_z, int B, int C, int q,
                                          int nt, float *__restrict__ partG, double *__restrict__ partS) {
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int r32 = lane & 31, hk = lane >> 5, wr = wid >> 1, wc = wid & 1;
  const int P = gridDim.y, p = blockIdx.y, nchunks = (B + kRows - 1) / kRows;
  int ti, tj;
  tile_of(q, nt, ti, tj);
  const bool diag = ti == tj;
  const int ca = ti * kTile, cb = tj * kTile;
  float *Pa = lds, *Pb = diag ? lds : lds + kRows * kPitch;

  // which of the wave's four 32 x 32 blocks hold an element (c, d), c <= d, of the matrix (wave-uniform)
  bool on[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
      on[i][j] = ca + 64 * wr + 32 * i < C && cb + 64 * wc + 32 * j < C && !(diag && 64 * wr + 32 * i > 64 * wc + 32 * j);

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  double dsum = 0.0;                            // diagonal tiles: the sum of column tid & 127 over rows 16 (tid >> 7) .. + 15

  f32x4 ra[4], rb[4];
  if (p < nchunks) {
    load_panel(ra, z, z_f16, ld_z, p * kRows, B, ca, C, tid);
    if (!diag) load_panel(rb, z, z_f16, ld_z, p * kRows, B, cb, C, tid);
  }
  for (int chunk = p; chunk < nchunks; chunk += P) {
    store_panel(Pa, ra, tid);
    if (!diag) store_panel(Pb, rb, tid);
    __syncthreads();
    if (chunk + P < nchunks) {                  // the next chunk's rows travel while this one's are multiplied
      load_panel(ra, z, z_f16, ld_z, (chunk + P) * kRows, B, ca, C, tid);
      if (!diag) load_panel(rb, z, z_f16, ld_z, (chunk + P) * kRows, B, cb, C, tid);
    }
    // "A" lane l = Z[row 2 s + (l >> 5)][ca + ...], "B" lane l = Z[the same row][cb + ...]
#pragma unroll 4
    for (int s = 0; s < kRows / 2; ++s) {
      const float *pa = Pa + (2 * s + hk) * kPitch + 64 * wr + r32;
      const float *pb = Pb + (2 * s + hk) * kPitch + 64 * wc + r32;
      const float a0 = pa[0], a1 = pa[32], b0 = pb[0], b1 = pb[32];
      if (on[0][0]) acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
      if (on[0][1]) acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
      if (on[1][0]) acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
      if (on[1][1]) acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
    }
    if (diag) {
      const float *col = Pa + (tid >> 7) * 16 * kPitch + (tid & 127);
#pragma unroll
      for (int r = 0; r < 16; ++r) dsum += (double)col[r * kPitch];
    }
    __syncthreads();                            // the next chunk's store overwrites the panels
  }

  // register r of lane l is row 8 (r >> 2) + 4 (l >> 5) + (r & 3) ("A"), column l & 31 ("B") of its block
  float *pg = partG + ((size_t)q * P + p) * (kTile * kTile);
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
      if (on[i][j]) {
#pragma unroll
        for (int r = 0; r < 16; ++r)
          pg[(64 * wr + 32 * i + 8 * (r >> 2) + 4 * hk + (r & 3)) * kTile + 64 * wc + 32 * j + r32] = acc[i][j][r];
      }
  if (diag) partS[((size_t)ti * P + p) * (2 * kTile) + tid] = dsum;
}

// cross tile x: panel ct = x % nt, targets 32 (x / nt) .. + 31
__device__ __forceinline__ void cross_tile(float *lds, const void *__restrict__ z, int z_f16, int ld_z, int B, int C,
                                           const float *__restrict__ t, int ld_t, int T, int x, int nt,
                                           float *__restrict__ partR, double *__restrict__ partT) {
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int r32 = lane & 31, hk = lane >> 5;
  const int P = gridDim.y, p = blockIdx.y, nchunks = (B + kRows - 1) / kRows;
  const int ct = x % nt, tt = x / nt;
  const int c0 = ct * kTile, t0 = tt * kTargets;
  float *Pa = lds, *Ts = lds + kRows * kPitch;
  const bool on = c0 + 32 * wid < C;            // (wave-uniform)
  const bool sums = ct == 0 && tid < 2 * kTargets;

  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  double ts = 0.0, tq = 0.0;                    // panel 0: target tid & 31 over rows 16 (tid >> 5) .. + 15

  f32x4 ra[4];
  float rt[4];
  if (p < nchunks) {
    load_panel(ra, z, z_f16, ld_z, p * kRows, B, c0, C, tid);
    load_targets(rt, t, ld_t, p * kRows, B, t0, T, tid);
  }
  for (int chunk = p; chunk < nchunks; chunk += P) {
    store_panel(Pa, ra, tid);
    store_targets(Ts, rt, tid);
    __syncthreads();
    if (chunk + P < nchunks) {
      load_panel(ra, z, z_f16, ld_z, (chunk + P) * kRows, B, c0, C, tid);
      load_targets(rt, t, ld_t, (chunk + P) * kRows, B, t0, T, tid);
    }
    if (on) {
#pragma unroll 4
      for (int s = 0; s < kRows / 2; ++s) {
        const float a = Ts[(2 * s + hk) * kTPitch + r32];
        const float b = Pa[(2 * s + hk) * kPitch + 32 * wid + r32];
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
      }
    }
    if (sums) {
      const float *col = Ts + (tid >> 5) * 16 * kTPitch + (tid & 31);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const double v = (double)col[r * kTPitch];
        ts += v;
        tq += v * v;
      }
    }
    __syncthreads();
  }

  float *pr = partR + ((size_t)x * P + p) * (kTargets * kTile);
  if (on) {
#pragma unroll
    for (int r = 0; r < 16; ++r) pr[(8 * (r >> 2) + 4 * hk + (r & 3)) * kTile + 32 * wid + r32] = acc[r];
  }
  if (sums) {                                   // [target tile][walker][half][sum, squares][32]
    double *pt = partT + (((size_t)tt * P + p) * 2 + (tid >> 5)) * (2 * kTargets) + (tid & 31);
    pt[0] = ts;
    pt[kTargets] = tq;
  }
}

// Workspace: partG [Gram tile][walker][128][128] fp32, partR [cross tile][walker][32][128] fp32,
// partS [panel][walker][2][128] double, partT [target tile][walker][2][2][32] double.
__global__ __launch_bounds__(256) void gram_pass_kernel(const void *__restrict__ z, int z_f16, int ld_z, int B, int C,
                                                        const float *__restrict__ t, int ld_t, int T, int nt, int ntri,
                                                        float *__restrict__ partG, float *__restrict__ partR,
                                                        double *__restrict__ partS, double *__restrict__ partT) {
  __shared__ __align__(16) float lds[2 * kRows * kPitch];
  const int q = blockIdx.x;
  if (q < ntri) gram_tile(lds, z, z_f16, ld_z, B, C, q, nt, partG, partS);
  else cross_tile(lds, z, z_f16, ld_z, B, C, t, ld_t, T, q - ntri, nt, partR, partT);
}

__device__ __forceinline__ void put(double *o, double sum, int accumulate) { *o = accumulate ? *o + sum : sum; }

// out (+)= the partials of walkers 0 .. P-1, in that order.  Blocks: 64 per Gram tile, then one per panel (column sums), then
// 16 per cross tile, then one per target tile (target sums).
__global__ __launch_bounds__(256) void gram_reduce_kernel(const float *__restrict__ partG, const float *__restrict__ partR,
                                                          const double *__restrict__ partS, const double *__restrict__ partT,
                                                          int P, int C, int T, int nt, int ntri, int ntt,
                                                          double *__restrict__ out_gram, double *__restrict__ out_sum,
                                                          double *__restrict__ out_cross, double *__restrict__ out_tsum,
                                                          double *__restrict__ out_tsq, int accumulate) {
  const int tid = threadIdx.x;
  int b = blockIdx.x;
  if (b < ntri * 64) {
    const int q = b >> 6, e = (b & 63) * 256 + tid;
    int ti, tj;
    tile_of(q, nt, ti, tj);
    const int c = ti * kTile + (e >> 7), d = tj * kTile + (e & 127);
    if (c >= C || d >= C || c > d) return;
    const double sum = ordered_sum<double>(partG + (size_t)q * P * (kTile * kTile) + e, (size_t)kTile * kTile, P);
    double *o = out_gram + (size_t)c * C + d;
    const double v = accumulate ? *o + sum : sum;
    *o = v;
    out_gram[(size_t)d * C + c] = v;            // the mirrored element: the same value
    return;
  }
  b -= ntri * 64;
  if (b < nt) {
    const int c = b * kTile + tid;
    if (tid < kTile && c < C) put(out_sum + c, ordered_sum<double>(partS + (size_t)b * P * (2 * kTile) + tid, kTile, 2 * P), accumulate);
    return;
  }
  b -= nt;
  if (b < nt * ntt * 16) {
    const int x = b >> 4, e = (b & 15) * 256 + tid;
    const int k = (x / nt) * kTargets + (e >> 7), c = (x % nt) * kTile + (e & 127);
    if (k < T && c < C)
      put(out_cross + (size_t)k * C + c,
          ordered_sum<double>(partR + (size_t)x * P * (kTargets * kTile) + e, (size_t)kTargets * kTile, P), accumulate);
    return;
  }
  b -= nt * ntt * 16;
  const int k = b * kTargets + (tid & 31);
  if (tid < 2 * kTargets && k < T) {
    const double sum = ordered_sum<double>(partT + (size_t)b * P * (4 * kTargets) + (tid >> 5) * kTargets + (tid & 31), 2 * kTargets, 2 * P);
    put((tid >> 5 ? out_tsq : out_tsum) + k, sum, accumulate);
  }
}

struct SegBatch {
  int32_t off[kSegBatch + 1];
};

// Workgroup (segment s of the batch, 128 columns from 128 blockIdx.y): thread (lane l = tid >> 5, four columns from
// 4 (tid & 31)) adds rows off[s] + l, + 8, ... in row order in double; then thread c < 128 adds the eight lanes in order.
__global__ __launch_bounds__(256) void segment_sums_kernel(const void *__restrict__ z, int z_f16, int ld_z, int C,
                                                           SegBatch seg, double *__restrict__ out, int accumulate) {
  __shared__ double Dp[kSegLanes][kTile];
  const int tid = threadIdx.x, l = tid >> 5, col = blockIdx.y * kTile + 4 * (tid & 31);
  const int r0 = seg.off[blockIdx.x], r1 = seg.off[blockIdx.x + 1];
  double sum[4] = {0.0, 0.0, 0.0, 0.0};
  if (col < C) {
#pragma unroll 4
    for (int row = r0 + l; row < r1; row += kSegLanes) {
      const size_t at = (size_t)row * ld_z + col;
      f32x4 v;
      if (z_f16) {
        const uint2 raw = *reinterpret_cast<const uint2 *>(static_cast<const __half *>(z) + at);
        const __half2 lo = __builtin_bit_cast(__half2, raw.x), hi = __builtin_bit_cast(__half2, raw.y);
        v = f32x4{__low2float(lo), __high2float(lo), __low2float(hi), __high2float(hi)};
      } else {
        v = *reinterpret_cast<const f32x4 *>(static_cast<const float *>(z) + at);
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) sum[k] += (double)v[k];
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) Dp[l][4 * (tid & 31) + k] = sum[k];
  __syncthreads();
  const int c = blockIdx.y * kTile + tid;
  if (tid < kTile && c < C) {
    double total = Dp[0][tid];
#pragma unroll
    for (int j = 1; j < kSegLanes; ++j) total += Dp[j][tid];
    put(out + (size_t)blockIdx.x * C + c, total, accumulate);
  }
}

}  // namespace
}  // namespace lla

using namespace lla;

extern "C" size_t lla_gram_pass_workspace_bytes(int C, int T) {
  if (!shape_ok(C, T)) return 0;
  const Plan pl = plan_of(C, T);
  const size_t P = (size_t)pl.pmax;
  return sizeof(float) * P * ((size_t)pl.ntri * kTile * kTile + (size_t)pl.nt * pl.ntt * kTargets * kTile) +
         sizeof(double) * P * ((size_t)pl.nt * 2 * kTile + (size_t)pl.ntt * 4 * kTargets);
}

extern "C" int lla_gram_pass(const void *z, int z_dtype, int ld_z, int B, int C, const float *t, int ld_t, int T,
                             double *out_gram, double *out_sum, double *out_cross, double *out_tsum, double *out_tsq,
                             int accumulate, void *workspace, void *stream) {
  if (!shape_ok(C, T) || !rows_ok(z, z_dtype, ld_z, B, C)) return LLA_EINVAL;
  if (t ? (T < 1 || ld_t < T || ((uintptr_t)t & 3) || !out_cross || !out_tsum || !out_tsq) : T != 0) return LLA_EINVAL;
  if (!out_gram || !out_sum || !workspace) return LLA_EINVAL;
  if (((uintptr_t)out_gram & 15) || ((uintptr_t)out_sum & 15) || ((uintptr_t)workspace & 15)) return LLA_EINVAL;
  if (t && (((uintptr_t)out_cross & 15) || ((uintptr_t)out_tsum & 15) || ((uintptr_t)out_tsq & 15))) return LLA_EINVAL;
  hipStream_t st = as_stream(stream);
  if (B == 0) {
    if (accumulate) return LLA_OK;
    hipError_t e = hipMemsetAsync(out_gram, 0, sizeof(double) * C * C, st);
    if (e == hipSuccess) e = hipMemsetAsync(out_sum, 0, sizeof(double) * C, st);
    if (e == hipSuccess && t) e = hipMemsetAsync(out_cross, 0, sizeof(double) * T * C, st);
    if (e == hipSuccess && t) e = hipMemsetAsync(out_tsum, 0, sizeof(double) * T, st);
    if (e == hipSuccess && t) e = hipMemsetAsync(out_tsq, 0, sizeof(double) * T, st);
    return e == hipSuccess ? LLA_OK : hip_fail(e);
  }

  const Plan pl = plan_of(C, T);
  const int nchunks = (B + kRows - 1) / kRows;
  const int P = nchunks < pl.pmax ? nchunks : pl.pmax;               // walkers: at least one chunk each
  float *partG = static_cast<float *>(workspace);
  float *partR = partG + (size_t)pl.pmax * pl.ntri * kTile * kTile;
  double *partS = reinterpret_cast<double *>(partR + (size_t)pl.pmax * pl.nt * pl.ntt * kTargets * kTile);
  double *partT = partS + (size_t)pl.pmax * pl.nt * 2 * kTile;
  const int z_f16 = z_dtype == LLA_Z_F16;
  gram_pass_kernel<<<dim3(pl.tiles, P), 256, 0, st>>>(z, z_f16, ld_z, B, C, t, ld_t, T, pl.nt, pl.ntri, partG, partR, partS,
                                                      partT);
  int rc = check_launch();
  if (rc != LLA_OK) return rc;
  const int blocks = pl.ntri * 64 + pl.nt + pl.nt * pl.ntt * 16 + pl.ntt;
  gram_reduce_kernel<<<blocks, 256, 0, st>>>(partG, partR, partS, partT, P, C, T, pl.nt, pl.ntri, pl.ntt, out_gram, out_sum,
                                             out_cross, out_tsum, out_tsq, accumulate);
  return check_launch();
}

extern "C" int lla_segment_sums(const void *z, int z_dtype, int ld_z, int B, int C, const int32_t *seg_offsets, int S,
                                double *out, int accumulate, void *stream) {
  if (!shape_ok(C, 0) || !rows_ok(z, z_dtype, ld_z, B, C) || S < 1 || !seg_offsets || !out || ((uintptr_t)out & 15))
    return LLA_EINVAL;
  if (seg_offsets[0] != 0 || seg_offsets[S] != B) return LLA_EINVAL;
  for (int s = 0; s < S; ++s)
    if (seg_offsets[s] > seg_offsets[s + 1]) return LLA_EINVAL;
  hipStream_t st = as_stream(stream);
  if (B == 0) {
    if (accumulate) return LLA_OK;
    hipError_t e = hipMemsetAsync(out, 0, sizeof(double) * S * C, st);
    return e == hipSuccess ? LLA_OK : hip_fail(e);
  }
  const int z_f16 = z_dtype == LLA_Z_F16;
  for (int s0 = 0; s0 < S; s0 += kSegBatch) {
    const int n = S - s0 < kSegBatch ? S - s0 : kSegBatch;
    SegBatch seg;
    for (int s = 0; s <= n; ++s) seg.off[s] = seg_offsets[s0 + s];
    for (int s = n + 1; s <= kSegBatch; ++s) seg.off[s] = seg.off[n];
    segment_sums_kernel<<<dim3(n, (C + kTile - 1) / kTile), 256, 0, st>>>(z, z_f16, ld_z, C, seg, out + (size_t)s0 * C,
                                                                         accumulate);
    const int rc = check_launch();
    if (rc != LLA_OK) return rc;
  }
  return LLA_OK;
}
