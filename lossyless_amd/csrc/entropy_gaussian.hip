// Entropy stage, scale hyperprior, conditional part (lossyless/rates.py:694-729; entropy.hip holds the factorized and
// indexed coders): the table row AND the mean of every element come from the predicted scale, so subtract / round /
// build_indexes / code (and decode / add / process_z_out) are one kernel each -- encode, decode, gathered decode, with
// and without the predicted means.  One image per lane as in entropy.hip; rows are read from global memory by the
// encoder (one look-up per symbol, off the state's dependency chain) and searched in LDS by the decoder.  The coder's
// primitives are rans.h's, the gathered decoder's staging gather_stage.h's.
#include "gather_stage.h"

namespace lla {
namespace {

struct __attribute__((aligned(8))) AffineParams {
  float bias, es;
};

// LDS both kernels start with: [C] (bias, exp_scale) | [T] scale table (padded to 8 bytes)
__host__ __device__ inline size_t gauss_head_bytes(int C, int T) {
  return (size_t)C * sizeof(AffineParams) + (((size_t)T * sizeof(float) + 7) & ~(size_t)7);
}

__device__ __forceinline__ void stage_gauss_head(uint8_t *smem, int C, int T, const float *__restrict__ bias,
                                                 const float *__restrict__ exp_scale,
                                                 const float *__restrict__ scale_table) {
  AffineParams *aff = reinterpret_cast<AffineParams *>(smem);
  float *stab = reinterpret_cast<float *>(smem + (size_t)C * sizeof(AffineParams));
  for (int c = threadIdx.x; c < C; c += blockDim.x) aff[c] = AffineParams{bias[c], exp_scale[c]};
  for (int t = threadIdx.x; t < T; t += blockDim.x) stab[t] = scale_table[t];
}

// GaussianConditional.build_indexes for G elements at once (every table entry is read once per group):
// T-1 minus the number of t < T-1 with max(scale, bound) <= table[t].  Counted as the reference counts it, not
// searched: nothing is assumed about the table's order, and a NaN scale compares false everywhere (row T-1) as
// torch.max / <= make it.  The result is in [0, T-1] whatever the scale.
template <int G>
__device__ __forceinline__ void scale_rows(const float *stab, int T, float bound, const float *scale, int *row) {
  float sb[G];
#pragma unroll
  for (int k = 0; k < G; ++k) {
    sb[k] = scale[k] < bound ? bound : scale[k];
    row[k] = T - 1;
  }
  for (int t = 0; t < T - 1; ++t) {
    const float v = stab[t];
#pragma unroll
    for (int k = 0; k < G; ++k) row[k] -= sb[k] <= v ? 1 : 0;
  }
}

// Opt-in operand of the three conditional kernels: the means the coder subtracts and adds back, element (b, c) at
// p[b*ld + c] (the second half of the z_encoder output, lossyless/rates.py:647-650).  It is a trailing parameter PACK
// (`Means...` is empty or one MeanRows): the instantiations without it are the kernels as they were -- same arguments,
// same kernarg layout, same instructions, the mean is the predicted scale (rates.py:694-696) -- and every use of the
// means sits behind `if constexpr (kMeans)`.
struct MeanRows {
  const float *p;
  size_t ld;
};
__device__ __forceinline__ const float *mean_row(size_t) { return nullptr; }
__device__ __forceinline__ const float *mean_row(size_t b, MeanRows m) { return m.p + b * m.ld; }
__device__ __forceinline__ size_t mean_ld() { return 0; }
__device__ __forceinline__ size_t mean_ld(MeanRows m) { return m.ld; }

template <int ZMODE, typename... Means>
__global__ __launch_bounds__(kEncThreads) void gaussian_encode_kernel(
    const void *__restrict__ in, int B, int C, const float *__restrict__ bias,
    const float *__restrict__ exp_scale, const float *__restrict__ scales, size_t ld_scales,
    const float *__restrict__ scale_table, float scale_bound, const int32_t *__restrict__ cdf, int T, int W,
    const int32_t *__restrict__ cdf_len, const int32_t *__restrict__ offset, uint8_t *__restrict__ scratch,
    size_t stride, uint32_t *__restrict__ lengths, int32_t *__restrict__ symbols_out,
    int32_t *__restrict__ indexes_out, Means... means) {
  constexpr bool kMeans = sizeof...(Means) != 0;
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const AffineParams *aff = reinterpret_cast<const AffineParams *>(smem);
  const float *stab = reinterpret_cast<const float *>(smem + (size_t)C * sizeof(AffineParams));
  int2 *par = reinterpret_cast<int2 *>(smem + gauss_head_bytes(C, T));   // [T] (row length, offset)
  stage_gauss_head(smem, C, T, bias, exp_scale, scale_table);
  for (int t = threadIdx.x; t < T; t += blockDim.x) par[t] = make_int2(row_len(cdf_len[t], W), offset[t]);
  __syncthreads();

  const int img = blockIdx.x * kEncThreads + threadIdx.x;
  if (img >= B) return;

  using F = Fetch<ZMODE>;
  constexpr int G = F::G;
  using elem = typename F::elem;
  const elem *src = reinterpret_cast<const elem *>(in) + (size_t)img * C;
  const float *sc = scales + (size_t)img * ld_scales;
  [[maybe_unused]] const float *mn = mean_row((size_t)img, means...);

  EncState s;
  uint8_t *end = open_encoder(s, scratch, stride, img);

  const bool vec_z = (reinterpret_cast<uintptr_t>(src) & 15u) == 0;
  const bool vec_s = (reinterpret_cast<uintptr_t>(sc) & 15u) == 0;
  // (means = scales + C is the caller's layout: for C % 4 != 0 the two rows are not aligned alike)
  [[maybe_unused]] const bool vec_m = (reinterpret_cast<uintptr_t>(mn) & 15u) == 0;
  // what a group needs: z, the scales and the table rows they select (every table entry read once per group), the means
  elem v[G];
  float sv[G];
  [[maybe_unused]] float mv[G];
  int t[G];
  auto load = [&](int c0, auto n_c) {
    if constexpr (decltype(n_c)::value == 1) {
      sv[0] = sc[c0];
      scale_rows<1>(stab, T, scale_bound, sv, t);
      if constexpr (kMeans) mv[0] = mn[c0];
      v[0] = src[c0];
    } else {
      load_group(v, src + c0, vec_z);
      load_group(sv, sc + c0, vec_s);
      scale_rows<G>(stab, T, scale_bound, sv, t);
      if constexpr (kMeans) load_group(mv, mn + c0, vec_m);
    }
  };
  auto prep = [&](int c, int k) {
    const AffineParams a = aff[c];
    const float zf = as_float(v[k]);
    // (z + bias) * exp_scale - mean, three separately rounded operations; without kMeans the mean IS the predicted
    // scale, unbounded
    float mean = sv[k];
    if constexpr (kMeans) mean = mv[k];
    const int32_t sym = quantise_one(zf, a.bias, a.es, mean);
    if (symbols_out) symbols_out[(size_t)img * C + c] = sym;
    if (indexes_out) indexes_out[(size_t)img * C + c] = t[k];
    const int2 q = par[t[k]];
    return prepare_channel(cdf + (size_t)t[k] * W, q.x, q.y, sym);
  };
  encode_walk<G>(s, C, load, prep);
  close_encoder(s, end, lengths, img);
}

// Inverse: image i's stream is record i * off_step of `off` (off_step = 2 walks the z records of an interleaved
// (z, side) body).  Every read is bounded by the record (refill) and by the row length (search_row); the row comes
// from scale_rows, i.e. is in range whatever the scales hold.
template <typename... Means>
__global__ __launch_bounds__(kEncThreads) void gaussian_decode_kernel(
    const uint8_t *__restrict__ payload, const uint64_t *__restrict__ off, int skip, int off_step, int B, int C,
    const float *__restrict__ bias, const float *__restrict__ exp_scale, const float *__restrict__ scales,
    size_t ld_scales, const float *__restrict__ scale_table, float scale_bound,
    const int32_t *__restrict__ cdf, int T, int W, const int32_t *__restrict__ cdf_len,
    const int32_t *__restrict__ offset, float *__restrict__ z_hat, int32_t *__restrict__ status,
    unsigned lds_bytes, Means... means) {
  constexpr bool kMeans = sizeof...(Means) != 0;
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const AffineParams *aff = reinterpret_cast<const AffineParams *>(smem);
  const float *stab = reinterpret_cast<const float *>(smem + (size_t)C * sizeof(AffineParams));
  const size_t head = gauss_head_bytes(C, T);     // (<= lds_bytes: checked by the launcher)
  stage_gauss_head(smem, C, T, bias, exp_scale, scale_table);
  __syncthreads();
  const PackedRows rows = stage_packed_rows(smem + head, lds_bytes - (unsigned)head, cdf, T, W, cdf_len, offset);

  const int i = blockIdx.x * kEncThreads + threadIdx.x;
  if (i >= B) return;
  DecState s;
  float *dst = z_hat + (size_t)i * C;
  if (!open_stream(s, payload, off, skip, i * off_step)) {
    for (int c = 0; c < C; ++c) dst[c] = 0.f;
    if (status) status[i] = 1;
    return;
  }
  const float *sc = scales + (size_t)i * ld_scales;
  // The rows do not depend on the coder state: they are derived a group ahead of the serial decode, so that every
  // scale-table entry is read once per group (as the encoder does), and the next group's scales are in flight.
  constexpr int G = 4;
  float sv_next[G];
#pragma unroll
  for (int k = 0; k < G; ++k) sv_next[k] = k < C ? sc[k] : 0.f;
  // (kMeans: the means travel with the scales, a group ahead, aligned or not as their own row is)
  [[maybe_unused]] const float *mn = mean_row((size_t)i, means...);
  [[maybe_unused]] float mv_next[G];
  if constexpr (kMeans) {
#pragma unroll
    for (int k = 0; k < G; ++k) mv_next[k] = k < C ? mn[k] : 0.f;
  }
  for (int c0 = 0; c0 < C; c0 += G) {
    float sv[G];
    [[maybe_unused]] float mv[G];
    int t[G];
#pragma unroll
    for (int k = 0; k < G; ++k) {
      sv[k] = sv_next[k];
      sv_next[k] = c0 + G + k < C ? sc[c0 + G + k] : 0.f;
    }
    if constexpr (kMeans) {
#pragma unroll
      for (int k = 0; k < G; ++k) {
        mv[k] = mv_next[k];
        mv_next[k] = c0 + G + k < C ? mn[c0 + G + k] : 0.f;
      }
    }
    scale_rows<G>(stab, T, scale_bound, sv, t);
#pragma unroll
    for (int k = 0; k < G; ++k) {
      const int c = c0 + k;
      if (c >= C) break;
      const int32_t sym = decode_row(s, rows, t[k], cdf, W, cdf_len, offset);
      const AffineParams a = aff[c];
      float mean = sv[k];
      if constexpr (kMeans) mean = mv[k];
      dst[c] = dequantise_one((float)sym, a.bias, a.es, mean);   // (sym + mean) / exp_scale - bias
    }
  }
  if (status) status[i] = s.pos > s.nwords ? 1 : 0;
}

// ---------------------------------------------------------------------------
// Gathered conditional decode (the second half of lossyless/rates.py:715-724 for the images a caller names): lane b
// decodes record off_first + index[b] * off_step with the rows and means of scales row b, exactly as
// gaussian_decode_kernel does (scale_rows, decode_symbol<true>, dequantise_one), but neither its scales nor its values
// go lane by lane through 2 KB-apart rows.  Both take gather_stage.h's staging, as rans_decode_gather_kernel's values do:
//   scales  global -> LDS: the workgroup reads the block of group g + 1 BEFORE it decodes group g and parks it after; two
//           buffers, since a fast wave parks group g + 1 while a slow one may still be reading group g.
// LDS in front of the packed rows: gauss_head_bytes + kVoteBytes + 3 x 256 x kGatherG x 4 = 4 352 + 16 + 49 152 bytes at C = 512,
// T = 64.  No static LDS (the vote is a word of the dynamic block, not __syncthreads_or's array): the launch may ask for
// the whole opt-in limit, as gaussian_decode_kernel does.
// ---------------------------------------------------------------------------
// With means (MeanRows, see gaussian_encode_kernel) they take the scales' road through two buffers of their own, in front
// of the scales' (+ 32 768 bytes), and a row whose status_in is set is left out of BOTH block reads.
__host__ __device__ inline size_t gauss_gather_front(int C, int T, int stages = 3) {
  return ((gauss_head_bytes(C, T) + 15u) & ~(size_t)15u) + kVoteBytes + stages * kGatherStageBytes;
}

template <typename OutT, typename... Means>
__global__ __launch_bounds__(kEncThreads) void gaussian_decode_gather_kernel(
    const uint8_t *__restrict__ payload, const uint64_t *__restrict__ off, int skip, int off_first, int off_step, int N,
    const int64_t *__restrict__ index, int B, int C, const float *__restrict__ bias,
    const float *__restrict__ exp_scale, const float *__restrict__ scales, size_t ld_scales,
    const float *__restrict__ scale_table, float scale_bound, const int32_t *__restrict__ cdf, int T, int W,
    const int32_t *__restrict__ cdf_len, const int32_t *__restrict__ offset, OutT *__restrict__ out, size_t ld_out,
    const int32_t *__restrict__ status_in, int32_t *__restrict__ status, unsigned lds_bytes, Means... means) {
  constexpr bool kMeans = sizeof...(Means) != 0;
  constexpr int kStages = kMeans ? 5 : 3;
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const AffineParams *aff = reinterpret_cast<const AffineParams *>(smem);
  const float *stab = reinterpret_cast<const float *>(smem + (size_t)C * sizeof(AffineParams));
  const size_t front = gauss_gather_front(C, T, kStages);     // (<= lds_bytes: checked by the launcher)
  [[maybe_unused]] float4 *mstage = reinterpret_cast<float4 *>(smem + front - 5 * kGatherStageBytes);   // [2][256][kGatherG] means
  float4 *sstage = reinterpret_cast<float4 *>(smem + front - 3 * kGatherStageBytes);   // [2][256][kGatherG] scales
  float4 *stage = reinterpret_cast<float4 *>(smem + front - kGatherStageBytes);        // [256][kGatherG] values
  int *vote = reinterpret_cast<int *>(smem + front - kStages * kGatherStageBytes - kVoteBytes);
  stage_gauss_head(smem, C, T, bias, exp_scale, scale_table);
  if (threadIdx.x == 0) *vote = 0;
  __syncthreads();
  const PackedRows rows = stage_packed_rows(smem + front, lds_bytes - (unsigned)front, cdf, T, W, cdf_len, offset);

  const GatherLanes g = gather_lanes(B);
  const int lane = g.lane, img = g.img;
  int st;
  DecState s;
  const bool live = pick_record(s, st, img, B, index, N, payload, off, skip, off_first, off_step, status_in);

  const bool vec_ok = out_vec_ok(out, ld_out);
  const bool vec_in = ((reinterpret_cast<uintptr_t>(scales) & 15u) == 0) && (ld_scales % 4 == 0);
  // kMeans: bit p = row p * 64 + wr has its status_in set, and neither block read touches it
  [[maybe_unused]] unsigned dead = 0;
  if constexpr (kMeans) {
    if (status_in) {
#pragma unroll
      for (int p = 0; p < kPasses; ++p) {
        const int r = p * 64 + g.wr;
        if (r < g.rows_here && status_in[g.row0 + r] != 0) dead |= 1u << p;
      }
    }
  }
  // this thread's share of the scales block at c0: gather_stage.h's fetch_block, written out.  With the matrix as an
  // argument the instantiations without means took 94 registers for 91 and the gather measured 0.6 % slower (1157 against
  // 1150 us at B = 1024, C = 512); the means block, whose base may be aligned otherwise, goes through the shared one.
  auto fetch = [&](int c0, float4 (&q)[kPasses]) {
    const int c = c0 + 4 * g.wj;
#pragma unroll
    for (int p = 0; p < kPasses; ++p) {
      const int r = p * 64 + g.wr;
      q[p] = float4{0.f, 0.f, 0.f, 0.f};
      if (r < g.rows_here && c < C) {
        if (kMeans && ((dead >> p) & 1u)) continue;
        load4(q[p], scales + (size_t)(g.row0 + r) * ld_scales + c, vec_in, c, C);
      }
    }
  };
  [[maybe_unused]] const float *mbase = mean_row(0, means...);
  [[maybe_unused]] const size_t ld_means = mean_ld(means...);
  [[maybe_unused]] const bool vec_mn = ((reinterpret_cast<uintptr_t>(mbase) & 15u) == 0) && (ld_means % 4 == 0);

  float4 nx[kPasses];
  [[maybe_unused]] float4 mx[kPasses];
  fetch(0, nx);
  park_block(sstage, g, nx);
  if constexpr (kMeans) {
    fetch_block(mbase, ld_means, vec_mn, g, 0, C, dead, mx);
    park_block(mstage, g, mx);
  }
  __syncthreads();

  int grp = 0;
  for (int c0 = 0; c0 < C; c0 += kGatherG, ++grp) {
    const float4 *sbuf = sstage + (size_t)(grp & 1) * kEncThreads * kChunks;
    const bool more = c0 + kGatherG < C;               // (uniform)
    if (more) fetch(c0 + kGatherG, nx);                // in flight under this group's decode
    [[maybe_unused]] const float4 *mbuf = mstage + (size_t)(grp & 1) * kEncThreads * kChunks;
    [[maybe_unused]] float4 qm;
    if constexpr (kMeans) {
      if (more) fetch_block(mbase, ld_means, vec_mn, g, c0 + kGatherG, C, dead, mx);
      qm = mbuf[own_slot(lane, 0)];
    }

    // the lane's own line, one 16-byte chunk (four channels) at a time as gaussian_decode_kernel walks a row: the rows
    // of four elements are counted together, the next chunk's scales are requested ahead of the serial decode.  (Not
    // unrolled over the chunks: sixteen copies of the tree search would not help a chain that waits on the LDS.)
    float4 qs = sbuf[own_slot(lane, 0)];
#pragma unroll 1
    for (int j = 0; j < kChunks; ++j) {
      const float sv[4] = {qs.x, qs.y, qs.z, qs.w};
      if (j + 1 < kChunks) qs = sbuf[own_slot(lane, j + 1)];
      [[maybe_unused]] float mv[4];
      if constexpr (kMeans) {
        mv[0] = qm.x, mv[1] = qm.y, mv[2] = qm.z, mv[3] = qm.w;
        if (j + 1 < kChunks) qm = mbuf[own_slot(lane, j + 1)];
      }
      float v[4] = {0.f, 0.f, 0.f, 0.f};
      if (live) {
        int t[4];
        scale_rows<4>(stab, T, scale_bound, sv, t);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int c = c0 + 4 * j + k;
          if (c >= C) break;
          const int32_t sym = decode_row(s, rows, t[k], cdf, W, cdf_len, offset);
          const AffineParams a = aff[c];
          float mean = sv[k];
          if constexpr (kMeans) mean = mv[k];
          v[k] = dequantise_one((float)sym, a.bias, a.es, mean);   // (sym + mean) / exp_scale - bias
        }
      }
      park_own(stage, lane, j, float4{v[0], v[1], v[2], v[3]});
    }
    if (more) park_block(sstage + (size_t)((grp + 1) & 1) * kEncThreads * kChunks, g, nx);
    if constexpr (kMeans) {
      if (more) park_block(mstage + (size_t)((grp + 1) & 1) * kEncThreads * kChunks, g, mx);
    }
    __syncthreads();
    write_out(stage, out, ld_out, g, c0, C, vec_ok);
    __syncthreads();
  }

  if (live && s.pos > s.nwords) st = 1;
  if (img < B && status) status[img] = st;
  zero_overrun(vote, live && st == 1, out, ld_out, img, C);
}

// (with_means, z_dtype) as compile-time tags: f(Fetch<..>, MeanRows) with means, f(Fetch<..>) without -- the kernels' `Means...` pack
// stays a pack, empty for the entry points without means.  dispatch_means alone where no dtype is involved.
template <typename F>
inline void dispatch_means(bool with_means, const float *means, size_t ld_means, F &&f) {
  if (with_means) f(MeanRows{means, ld_means});
  else f();
}
template <typename F>
inline void dispatch_gauss(int z_dtype, bool with_means, const float *means, size_t ld_means, F &&f) {
  dispatch_means(with_means, means, ld_means, [&](auto... m) { with_z(z_dtype, [&](auto zt) { f(zt, m...); }); });
}

}  // namespace
}  // namespace lla

using namespace lla;

extern "C" {

// The three conditional entry points and their _means siblings share argument checks and launch; `means` = NULL is the
// entry point without means (the kernels' instantiations with an empty pack).
static int gaussian_encode(const void *z, int z_dtype, int B, int C, const float *bias, const float *exp_scale,
                           const float *scales, size_t ld_scales, const float *means, size_t ld_means, bool with_means,
                           const float *scale_table, float scale_bound, const int32_t *cdf, int T, int W,
                           const int32_t *cdf_len, const int32_t *offset, uint8_t *scratch, size_t stride,
                           uint32_t *lengths, int32_t *symbols_out, int32_t *indexes_out, void *stream) {
  if (B == 0) return LLA_OK;
  if (with_means && (!means || ld_means < (size_t)(C > 0 ? C : 0))) return LLA_EINVAL;
  if (B < 0 || C <= 0 || T <= 0 || W < 3 || !z || !bias || !exp_scale || !scales || ld_scales < (size_t)C ||
      !scale_table || !cdf || !cdf_len || !offset || !scratch || !lengths)
    return LLA_EINVAL;
  if (z_dtype != LLA_Z_F16 && z_dtype != LLA_Z_F32) return LLA_EINVAL;
  if (stride < lla_rans_max_encoded_bytes(C) || (stride & 3u)) return LLA_ECAP;
  const size_t lds = gauss_head_bytes(C, T) + (size_t)T * sizeof(int2);
  if (lds > 64 * 1024) return LLA_EINVAL;
  const int grid = (B + kEncThreads - 1) / kEncThreads;
  dispatch_gauss(z_dtype, with_means, means, ld_means, [&](auto zt, auto... m) {
    gaussian_encode_kernel<decltype(zt)::mode, decltype(m)...><<<grid, kEncThreads, lds, as_stream(stream)>>>(
        z, B, C, bias, exp_scale, scales, ld_scales, scale_table, scale_bound, cdf, T, W, cdf_len, offset, scratch,
        stride, lengths, symbols_out, indexes_out, m...);
  });
  return check_launch();
}

int lla_gaussian_quantise_encode(const void *z, int z_dtype, int B, int C, const float *bias,
                                 const float *exp_scale, const float *scales, size_t ld_scales,
                                 const float *scale_table, float scale_bound, const int32_t *cdf, int T, int W,
                                 const int32_t *cdf_len, const int32_t *offset, uint8_t *scratch, size_t stride,
                                 uint32_t *lengths, int32_t *symbols_out, int32_t *indexes_out, void *stream) {
  return gaussian_encode(z, z_dtype, B, C, bias, exp_scale, scales, ld_scales, nullptr, 0, false, scale_table, scale_bound,
                         cdf, T, W, cdf_len, offset, scratch, stride, lengths, symbols_out, indexes_out, stream);
}

int lla_gaussian_quantise_encode_means(const void *z, int z_dtype, int B, int C, const float *bias,
                                       const float *exp_scale, const float *scales, size_t ld_scales,
                                       const float *means, size_t ld_means, const float *scale_table,
                                       float scale_bound, const int32_t *cdf, int T, int W, const int32_t *cdf_len,
                                       const int32_t *offset, uint8_t *scratch, size_t stride, uint32_t *lengths,
                                       int32_t *symbols_out, int32_t *indexes_out, void *stream) {
  return gaussian_encode(z, z_dtype, B, C, bias, exp_scale, scales, ld_scales, means, ld_means, true, scale_table,
                         scale_bound, cdf, T, W, cdf_len, offset, scratch, stride, lengths, symbols_out, indexes_out, stream);
}

static int gaussian_decode(const uint8_t *payload, const uint64_t *off, int record_prefix, int off_first, int off_step,
                           int B, int C, const float *bias, const float *exp_scale, const float *scales,
                           size_t ld_scales, const float *means, size_t ld_means, bool with_means,
                           const float *scale_table, float scale_bound, const int32_t *cdf, int T, int W,
                           const int32_t *cdf_len, const int32_t *offset, float *z_hat, int32_t *status, void *stream) {
  if (B == 0) return LLA_OK;
  if (with_means && (!means || ld_means < (size_t)(C > 0 ? C : 0))) return LLA_EINVAL;
  if (B < 0 || C <= 0 || T <= 0 || W < 3 || !payload || !off || off_first < 0 || off_step < 1 || !bias ||
      !exp_scale || !scales || ld_scales < (size_t)C || !scale_table || !cdf || !cdf_len || !offset || !z_hat)
    return LLA_EINVAL;
  const size_t front = gauss_head_bytes(C, T);
  if (front > 32 * 1024) return LLA_EINVAL;
  const int grid = (B + kEncThreads - 1) / kEncThreads;
  dispatch_means(with_means, means, ld_means, [&](auto... m) {
    const unsigned lds = packed_rows_lds(reinterpret_cast<const void *>(gaussian_decode_kernel<decltype(m)...>), front, T, W);
    gaussian_decode_kernel<decltype(m)...><<<grid, kEncThreads, lds, as_stream(stream)>>>(
        payload, off + off_first, record_prefix ? 4 : 0, off_step, B, C, bias, exp_scale, scales, ld_scales,
        scale_table, scale_bound, cdf, T, W, cdf_len, offset, z_hat, status, lds, m...);
  });
  return check_launch();
}

int lla_gaussian_decode_dequantise(const uint8_t *payload, const uint64_t *off, int record_prefix, int off_first,
                                   int off_step, int B, int C, const float *bias, const float *exp_scale,
                                   const float *scales, size_t ld_scales, const float *scale_table,
                                   float scale_bound, const int32_t *cdf, int T, int W, const int32_t *cdf_len,
                                   const int32_t *offset, float *z_hat, int32_t *status, void *stream) {
  return gaussian_decode(payload, off, record_prefix, off_first, off_step, B, C, bias, exp_scale, scales, ld_scales,
                         nullptr, 0, false, scale_table, scale_bound, cdf, T, W, cdf_len, offset, z_hat, status, stream);
}

int lla_gaussian_decode_dequantise_means(const uint8_t *payload, const uint64_t *off, int record_prefix, int off_first,
                                         int off_step, int B, int C, const float *bias, const float *exp_scale,
                                         const float *scales, size_t ld_scales, const float *means, size_t ld_means,
                                         const float *scale_table, float scale_bound, const int32_t *cdf, int T, int W,
                                         const int32_t *cdf_len, const int32_t *offset, float *z_hat, int32_t *status,
                                         void *stream) {
  return gaussian_decode(payload, off, record_prefix, off_first, off_step, B, C, bias, exp_scale, scales, ld_scales,
                         means, ld_means, true, scale_table, scale_bound, cdf, T, W, cdf_len, offset, z_hat, status, stream);
}

static size_t gaussian_gather_lds(int C, int T, int W, int z_dtype, size_t *front, bool with_means) {
  if (front) *front = 0;
  if ((z_dtype != LLA_Z_F16 && z_dtype != LLA_Z_F32) || C <= 0 || T <= 0 || W < 3 || gauss_head_bytes(C, T) > 32 * 1024)
    return 0;
  const size_t fr = gauss_gather_front(C, T, with_means ? 5 : 3);
  const void *kernel = nullptr;
  dispatch_gauss(z_dtype, with_means, nullptr, 0, [&](auto zt, auto... m) {
    kernel = reinterpret_cast<const void *>(gaussian_decode_gather_kernel<typename decltype(zt)::elem, decltype(m)...>);
  });
  if (fr > dynamic_lds_limit(kernel)) return 0;
  if (front) *front = fr;
  return packed_rows_lds(kernel, fr, T, W);
}

size_t lla_gaussian_decode_gather_lds_bytes(int C, int T, int W, int z_dtype, size_t *front) {
  return gaussian_gather_lds(C, T, W, z_dtype, front, false);
}

size_t lla_gaussian_decode_gather_means_lds_bytes(int C, int T, int W, int z_dtype, size_t *front) {
  return gaussian_gather_lds(C, T, W, z_dtype, front, true);
}

static int gaussian_gather(const uint8_t *payload, const uint64_t *off, int record_prefix, int off_first, int off_step,
                           int N, const int64_t *index, int B, int C, const float *bias, const float *exp_scale,
                           const float *scales, size_t ld_scales, const float *means, size_t ld_means, bool with_means,
                           const float *scale_table, float scale_bound, const int32_t *cdf, int T, int W,
                           const int32_t *cdf_len, const int32_t *offset, void *z_hat, int z_dtype, size_t ld_out,
                           const int32_t *status_in, int32_t *status, void *stream) {
  if (z_dtype != LLA_Z_F16 && z_dtype != LLA_Z_F32) return LLA_EINVAL;
  if (off_first < 0 || off_step < 1) return LLA_EINVAL;
  if (B == 0) return LLA_OK;
  if (with_means && (!means || ld_means < (size_t)(C > 0 ? C : 0))) return LLA_EINVAL;
  if (B < 0 || N < 0 || C <= 0 || T <= 0 || W < 3 || !payload || !off || !index || !bias || !exp_scale || !scales ||
      ld_scales < (size_t)C || !scale_table || !cdf || !cdf_len || !offset || !z_hat || ld_out < (size_t)C || !status)
    return LLA_EINVAL;
  // (52 KiB in front of the rows, 84 KiB with means: a gfx950 has 160; 0 = the head or the front does not fit)
  const unsigned lds = (unsigned)gaussian_gather_lds(C, T, W, z_dtype, nullptr, with_means);
  if (lds == 0) return LLA_EINVAL;
  const int grid = (B + kEncThreads - 1) / kEncThreads;
  const int skip = record_prefix ? 4 : 0;
  dispatch_gauss(z_dtype, with_means, means, ld_means, [&](auto zt, auto... m) {
    using OutT = typename decltype(zt)::elem;
    gaussian_decode_gather_kernel<OutT, decltype(m)...><<<grid, kEncThreads, lds, as_stream(stream)>>>(
        payload, off, skip, off_first, off_step, N, index, B, C, bias, exp_scale, scales, ld_scales, scale_table,
        scale_bound, cdf, T, W, cdf_len, offset, reinterpret_cast<OutT *>(z_hat), ld_out, status_in, status, lds, m...);
  });
  return check_launch();
}

int lla_gaussian_decode_gather(const uint8_t *payload, const uint64_t *off, int record_prefix, int off_first,
                               int off_step, int N, const int64_t *index, int B, int C, const float *bias,
                               const float *exp_scale, const float *scales, size_t ld_scales,
                               const float *scale_table, float scale_bound, const int32_t *cdf, int T, int W,
                               const int32_t *cdf_len, const int32_t *offset, void *z_hat, int z_dtype,
                               size_t ld_out, const int32_t *status_in, int32_t *status, void *stream) {
  return gaussian_gather(payload, off, record_prefix, off_first, off_step, N, index, B, C, bias, exp_scale, scales,
                         ld_scales, nullptr, 0, false, scale_table, scale_bound, cdf, T, W, cdf_len, offset, z_hat, z_dtype,
                         ld_out, status_in, status, stream);
}

int lla_gaussian_decode_gather_means(const uint8_t *payload, const uint64_t *off, int record_prefix, int off_first,
                                     int off_step, int N, const int64_t *index, int B, int C, const float *bias,
                                     const float *exp_scale, const float *scales, size_t ld_scales, const float *means,
                                     size_t ld_means, const float *scale_table, float scale_bound, const int32_t *cdf,
                                     int T, int W, const int32_t *cdf_len, const int32_t *offset, void *z_hat,
                                     int z_dtype, size_t ld_out, const int32_t *status_in, int32_t *status,
                                     void *stream) {
  return gaussian_gather(payload, off, record_prefix, off_first, off_step, N, index, B, C, bias, exp_scale, scales,
                         ld_scales, means, ld_means, true, scale_table, scale_bound, cdf, T, W, cdf_len, offset, z_hat,
                         z_dtype, ld_out, status_in, status, stream);
}

}  // extern "C"
