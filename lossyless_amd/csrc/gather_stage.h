// Staging of the gathered decoders (rans_decode_gather_kernel in entropy.hip, gaussian_decode_gather_kernel in
// entropy_gaussian.hip): lane b of a 256-lane workgroup decodes the record index[b] names, and neither its values nor
// (conditional coder) its scales and means travel lane by lane through rows that lie 2 KB apart -- a lane that stored its
// own row would put 64 separate cache lines behind every store of a wave.  They pass through LDS in blocks of 256 rows x
// kGatherG channels instead:
//   staging: [256 lanes][kGatherG floats] in 16-byte chunks; lane L's chunk j sits at slot (j + (L >> 1)) & 3 of
//   its 64-byte line.  A ds_write_b128 is served in groups of 8 consecutive lanes over 32 banks; their lines are 64
//   bytes apart, so without the rotation lanes L, L+2, L+4, L+6 meet in the same four banks (4-way conflict); with it
//   the eight chunks cover the 32 banks once.  The block side reads and writes whole lines: four consecutive threads
//   cover the 64 contiguous bytes (fp32) one row has in the group, 64 rows per pass, every chunk once.
// No lane leaves before the last barrier: one without a record parks zeros, which is also what its row must hold.
#pragma once
#include "rans.h"

namespace lla {
namespace {

constexpr int kGatherG = 16;
constexpr int kChunks = kGatherG / 4;        // 16-byte chunks per staged line
constexpr int kPasses = kEncThreads / 64;    // 4 threads per row, 64 rows per pass
constexpr size_t kGatherStageBytes = (size_t)kEncThreads * kGatherG * sizeof(float);
constexpr size_t kVoteBytes = 16;            // the overrun vote: one word of the DYNAMIC block, so that a kernel has no static LDS

struct GatherLanes {
  int lane, row0, img;   // this lane decodes row img = row0 + lane of the launch
  int wr, wj;            // block side: chunk wj of rows p * 64 + wr, p < kPasses
  int rows_here;         // rows of the launch in this workgroup
};
__device__ __forceinline__ GatherLanes gather_lanes(int B) {
  GatherLanes g;
  g.lane = threadIdx.x;
  g.row0 = blockIdx.x * kEncThreads;
  g.img = g.row0 + g.lane;
  g.wr = g.lane >> 2, g.wj = g.lane & 3;
  g.rows_here = min(kEncThreads, B - g.row0);
  return g;
}

// The record of row img: status 0 and an open stream (returns true), or the status the row ends with -- status_in's when
// that is given and set, 2 for an index outside [0, N), 1 for a stream that cannot be opened; untouched past B.
// image index[img] is record off_first + index * off_step: in 64 bits, and only once the index is known to be in
// [0, N) (the product is then below 2^62)
__device__ __forceinline__ bool pick_record(DecState &s, int &st, int img, int B, const int64_t *__restrict__ index, int N,
                                            const uint8_t *__restrict__ payload, const uint64_t *__restrict__ off, int skip,
                                            int off_first, int off_step, const int32_t *__restrict__ status_in = nullptr) {
  st = 0;
  if (img >= B) return false;
  const int64_t rec = index[img];
  if (status_in && status_in[img] != 0) st = status_in[img];
  else if (rec < 0 || rec >= (int64_t)N) st = 2;
  else if (!open_stream(s, payload, off, skip, (size_t)((int64_t)off_first + rec * (int64_t)off_step))) st = 1;
  return st == 0;
}

// lane side: chunk j of the lane's own line
__device__ __forceinline__ int own_slot(int lane, int j) { return lane * kChunks + ((j + (lane >> 1)) & 3); }
__device__ __forceinline__ void park_own(float4 *stage, int lane, int j, const float4 &v) { stage[own_slot(lane, j)] = v; }

// four channels from column c of a row into q, which holds zeros: one 16-byte load where allowed, else those below C
__device__ __forceinline__ void load4(float4 &q, const float *src, bool vec, int c, int C) {
  if (vec && c + 3 < C) {
    q = *reinterpret_cast<const float4 *>(src);
  } else {
    q.x = src[0];
    if (c + 1 < C) q.y = src[1];
    if (c + 2 < C) q.z = src[2];
    if (c + 3 < C) q.w = src[3];
  }
}
// block side, global -> LDS: this thread's share of the 256 x kGatherG block at column c0 of the row-major matrix `base`
// (leading dimension ld; vec: base and ld allow 16-byte loads) -- zeros outside B x C and for the rows whose bit of `dead`
// is set, which are not read at all.  (The SCALES block of gaussian_decode_gather_kernel deliberately keeps this walk as a
// lambda of its own, for registers and time: see there.)
__device__ __forceinline__ void fetch_block(const float *__restrict__ base, size_t ld, bool vec, const GatherLanes &g, int c0,
                                            int C, unsigned dead, float4 (&q)[kPasses]) {
  const int c = c0 + 4 * g.wj;
#pragma unroll
  for (int p = 0; p < kPasses; ++p) {
    const int r = p * 64 + g.wr;
    q[p] = float4{0.f, 0.f, 0.f, 0.f};
    if (r < g.rows_here && c < C && !((dead >> p) & 1u)) load4(q[p], base + (size_t)(g.row0 + r) * ld + c, vec, c, C);
  }
}
__device__ __forceinline__ void park_block(float4 *buf, const GatherLanes &g, const float4 (&q)[kPasses]) {
#pragma unroll
  for (int p = 0; p < kPasses; ++p) {
    const int r = p * 64 + g.wr;
    buf[r * kChunks + ((g.wj + (r >> 1)) & 3)] = q[p];
  }
}

// block side, LDS -> global: the staged block to columns [c0, c0 + kGatherG) of `out` (call between two barriers)
template <typename OutT>
__device__ __forceinline__ void write_out(const float4 *stage, OutT *__restrict__ out, size_t ld_out, const GatherLanes &g,
                                          int c0, int C, bool vec_ok) {
  const int c = c0 + 4 * g.wj;
#pragma unroll
  for (int p = 0; p < kPasses; ++p) {
    const int r = p * 64 + g.wr;
    if (r < g.rows_here && c < C) {
      const float4 q = stage[r * kChunks + ((g.wj + (r >> 1)) & 3)];
      OutT *dst = out + (size_t)(g.row0 + r) * ld_out + c;
      if (vec_ok && c + 3 < C) {
        store_out4(dst, q);
      } else {
        store_out(dst, q.x);
        if (c + 1 < C) store_out(dst + 1, q.y);
        if (c + 2 < C) store_out(dst + 2, q.z);
        if (c + 3 < C) store_out(dst + 3, q.w);
      }
    }
  }
}
template <typename OutT>
__device__ __forceinline__ bool out_vec_ok(const OutT *out, size_t ld_out) {
  return (reinterpret_cast<uintptr_t>(out) % (4 * sizeof(OutT)) == 0) && (ld_out % 4 == 0);
}

// A stream that overran is known only after the last symbol, when other lanes have written its row: the workgroup votes
// through *vote (zeroed before an earlier barrier), and once those stores have completed (agent-scope fence in every
// thread, then the barrier) the row's own lane zeroes it.  Rare path.
template <typename OutT>
__device__ __forceinline__ void zero_overrun(int *vote, bool overran, OutT *__restrict__ out, size_t ld_out, int img, int C) {
  if (overran) *vote = 1;
  __syncthreads();
  if (*vote) {
    __threadfence();
    __syncthreads();
    if (overran) {
      OutT *dst = out + (size_t)img * ld_out;
      for (int c = 0; c < C; ++c) store_out(dst + c, 0.f);
    }
  }
}

}  // namespace
}  // namespace lla
