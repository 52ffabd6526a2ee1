// The walk over decoded rows in 32-row tiles that probe.hip, knn.hip, kmeans.hip and gram.hip share (gfx950): the ONE copy
// of the staging of a row tile (step 1 of their file heads), of the score MFMA and the ordered merge of its partial tiles
// (step 2), of a staged row's sum of squares, of the slice MFMA and its store (step 4), of the ordered sum over walkers, and
// of the argument checks of the rows.  The determinism contract of every probe rests on these: a row's bits do not depend
// on the batch, a k-means score equals a kNN score, and partials are added in walker order.  Step 3 is each file's own.
#pragma once
#include "common.h"

#include <hip/hip_fp16.h>

namespace lla {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kRows = 32;          // rows per staged tile
constexpr int kClasses = 32;       // classes, centroids or queries per workgroup: the other edge of a score tile
constexpr int kZPad = 4;           // floats: 16-byte reads of one column group from 32 rows touch 16 distinct slots
constexpr int kResident = 512;     // workgroups the chip holds at two per CU: the grid is cut to it

inline int class_tiles(int K) { return (K + kClasses - 1) / kClasses; }
inline int tile_walkers(int nct) { const int w = kResident / nct; return w < 1 ? 1 : w; }

// the row widths every pass takes: column groups of 8, at most the 1024 whose staged tile fits in LDS
inline bool cols_ok(int C) { return C >= 8 && C <= 1024 && (C & 7) == 0; }

// B rows of C columns at z.  The four files had the same rule (gram.hip's form): no file was stricter or looser in the
// alignment of z (16 bytes for fp32 rows, 8 for fp16: the widest load of a row), and each checks it for B == 0 too.
inline bool rows_ok(const void *z, int z_dtype, int ld_z, int B, int C) {
  if (B < 0 || ld_z < C || (ld_z & 3) || (z_dtype != LLA_Z_F32 && z_dtype != LLA_Z_F16)) return false;
  if (B > 0 && !z) return false;
  return ((uintptr_t)z & (z_dtype == LLA_Z_F32 ? 15 : 7)) == 0;
}

// 1. rows row0 .. row0 + 31 -> Zs [32][C + kZPad] as fp32 (rows beyond B are zeros: they contribute exactly nothing, become
// no candidate and are assigned nowhere)
__device__ __forceinline__ void stage_rows(float *Zs, const void *__restrict__ z, int z_f16, int ld_z, int row0, int B,
                                           int C, int tid) {
  const int pitch = C + kZPad, c4n = C >> 2;
  for (int i = tid; i < kRows * c4n; i += 256) {
    const int row = i / c4n, c4 = i - row * c4n;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (row0 + row < B) {
      const size_t at = (size_t)(row0 + row) * ld_z + 4 * c4;
      if (z_f16) {
        const uint2 raw = *reinterpret_cast<const uint2 *>(static_cast<const __half *>(z) + at);
        const __half2 lo = __builtin_bit_cast(__half2, raw.x), hi = __builtin_bit_cast(__half2, raw.y);
        v = f32x4{__low2float(lo), __high2float(lo), __low2float(hi), __high2float(hi)};
      } else {
        v = *reinterpret_cast<const f32x4 *>(static_cast<const float *>(z) + at);
      }
    }
    *reinterpret_cast<f32x4 *>(Zs + row * pitch + 4 * c4) = v;
  }
}

// the staged rows' sums of squares -> Np [32 rows][8]: thread (row, part) takes columns 4 (part + 8 i) .. + 3, i ascending
__device__ __forceinline__ void row_squares(const float *Zs, float *Np, int C, int tid) {
  const int row = tid >> 3, part = tid & 7;
  float ss = 0.f;
  for (int c4 = part; c4 < (C >> 2); c4 += 8) {
    const f32x4 v = *reinterpret_cast<const f32x4 *>(Zs + row * (C + kZPad) + 4 * c4);
    ss += v[0] * v[0];
    ss += v[1] * v[1];
    ss += v[2] * v[2];
    ss += v[3] * v[3];
  }
  Np[tid] = ss;
}

// n2 of a staged row from its eight partial sums, in the order of the parts
__device__ __forceinline__ float row_n2(const float *Np, int row) {
  const f32x4 a = *reinterpret_cast<const f32x4 *>(Np + 8 * row), b = *reinterpret_cast<const f32x4 *>(Np + 8 * row + 4);
  float ss = a[0];
  ss += a[1], ss += a[2], ss += a[3], ss += b[0], ss += b[1], ss += b[2], ss += b[3];
  return ss;
}

__device__ __forceinline__ float inv_norm(float n2) { return n2 > 0.f ? 1.f / sqrtf(n2) : 0.f; }

// The four waves' partial score tiles -> Sp [product][slot][32 classes][32 rows], added in wave order: register r of lane l
// is class 8 (r >> 2) + 4 (l >> 5) + (r & 3), row l & 31.  One product (TWO = false): waves 0, 1 write the two slots and
// waves 2, 3 add to them, (w0 + w2) and (w1 + w3), for the reader to add; two products hold one slot each in the same bytes,
// the waves adding one after the other.  Ends on a barrier.
template <bool TWO>
__device__ __forceinline__ void merge_score_slots(float *Sp, f32x16 s, f32x16 tv, int r32, int hk, int wid) {
  constexpr int NSLOT = TWO ? 1 : 2;
#pragma unroll
  for (int stage = 0; stage < 4 / NSLOT; ++stage) {
    if (wid / NSLOT == stage) {
      float *dst = Sp + (wid % NSLOT) * (kRows * kClasses);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int at = (8 * (r >> 2) + 4 * hk + (r & 3)) * kRows + r32;
        if (stage == 0) {
          dst[at] = s[r];
          if (TWO) dst[kRows * kClasses + at] = tv[r];
        } else {
          dst[at] += s[r];
          if (TWO) dst[kRows * kClasses + at] += tv[r];
        }
      }
    }
    __syncthreads();
  }
}

// 2. scores of the staged tile against 32 classes, the C dimension dealt to the four waves in groups of 8 and the partial
// tiles merged as above (HV: the second product, with V).  wp / vp: this lane's row of W / V, + 4 (lane >> 5); vp is not
// read unless HV.  "A" lane l = W[class l & 31][c + (l >> 5)], "B" lane l = Z[row l & 31][c + (l >> 5)]  (gemm_f32.hip)
template <bool HV>
__device__ __forceinline__ void tile_scores(const float *Zs, float *Sp, const float *__restrict__ wp,
                                            const float *__restrict__ vp, int C, int lane, int wid) {
  const int pitch = C + kZPad, ngroups = C >> 3;
  const int r32 = lane & 31, hk = lane >> 5;
  f32x16 s, tv;
#pragma unroll
  for (int r = 0; r < 16; ++r) s[r] = 0.f, tv[r] = 0.f;
  for (int g = wid; g < ngroups; g += 4) {
    const f32x4 a = *reinterpret_cast<const f32x4 *>(Zs + r32 * pitch + 8 * g + 4 * hk);
    const f32x4 w = *reinterpret_cast<const f32x4 *>(wp + 8 * g);
#pragma unroll
    for (int j = 0; j < 4; ++j) s = __builtin_amdgcn_mfma_f32_32x32x2f32(w[j], a[j], s, 0, 0, 0);
    if (HV) {
      const f32x4 v = *reinterpret_cast<const f32x4 *>(vp + 8 * g);
#pragma unroll
      for (int j = 0; j < 4; ++j) tv = __builtin_amdgcn_mfma_f32_32x32x2f32(v[j], a[j], tv, 0, 0, 0);
    }
  }
  merge_score_slots<HV>(Sp, s, tv, r32, hk, wid);
}

// 4. the slice [32 classes][C] += A^T Z_tile on v_mfma_f32_32x32x2_f32: "A" lane l = a_of(row 2 s + (l >> 5)), the value
// of class l & 31 for that row; "B" lane l = Z[row 2 s + (l >> 5)][column].  NT: 32-column tiles of the slice per wave
// (C <= 128 NT), kept in accumulator registers over ALL the row tiles of a walker.
template <int NT, typename A>
__device__ __forceinline__ void slice_mfma(f32x16 (&acc)[NT], const float *Zs, A a_of, int C, int lane, int wid) {
  const int pitch = C + kZPad, r32 = lane & 31, hk = lane >> 5;
#pragma unroll 4
  for (int s2 = 0; s2 < kRows / 2; ++s2) {
    const float a = a_of(2 * s2 + hk);
    const float *zrow = Zs + (2 * s2 + hk) * pitch;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int c0 = (wid + 4 * t) * 32;
      if (c0 < C) {
        int cc = c0 + r32;
        if (cc > C - 1) cc = C - 1;          // clamped columns are computed and not stored
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, zrow[cc], acc[t], 0, 0, 0);
      }
    }
  }
}

// a walker's slice -> pw [32][C], its part of part_W
template <int NT>
__device__ __forceinline__ void slice_store(const f32x16 (&acc)[NT], float *__restrict__ pw, int C, int lane, int wid) {
  const int r32 = lane & 31, hk = lane >> 5;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int cc = (wid + 4 * t) * 32 + r32;
    if (cc < C) {
#pragma unroll
      for (int r = 0; r < 16; ++r) pw[(size_t)(8 * (r >> 2) + 4 * hk + (r & 3)) * C + cc] = acc[t][r];
    }
  }
}

// sum over walkers 0 .. P-1 of src[p * stride], added in that order in T; the loads go out eight at a time (a thread that
// waited for each one before asking for the next spent 0.35 ms on 512 partial sums)
template <typename T, typename S>
__device__ __forceinline__ T ordered_sum(const S *__restrict__ src, size_t stride, int P) {
  T sum = 0;
  int p = 0;
  for (; p + 8 <= P; p += 8) {
    S v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = src[(size_t)(p + j) * stride];
#pragma unroll
    for (int j = 0; j < 8; ++j) sum += (T)v[j];
  }
  for (; p < P; ++p) sum += (T)src[(size_t)p * stride];
  return sum;
}

}  // namespace
}  // namespace lla
