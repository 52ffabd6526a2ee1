// Entropy stage of the compress_dataset hot path on gfx950: quantise, rANS encode,
// stream compaction, rANS decode, dequantise.  Integer / bit-manipulation work, no
// MFMA.  One image per lane: a wave64 carries 64 independent rANS states through
// the 512-symbol dependency chain in lock-step over the channel index, so every
// lane of a wave reads the SAME table row at the same time (LDS broadcast / no
// bank conflicts), and the table (u16 [C][W], <= 34 KB) lives in LDS.
//
// Reference behaviour being replaced (compressai==1.1.5, not vendored):
//   RansEncoder.encode_with_indexes / RansDecoder.decode_with_indexes
//   (cpp_exts/rans/rans_interface.cpp, third_party/ryg_rans/rans64.h), called per
//   image from hub/compressor.py:98,124.  Algorithm: SURVEY.md 8(a) A13 / A14.
#include "common.h"

#include <hip/hip_fp16.h>

#include <cstdlib>
#include <type_traits>

namespace lla {

thread_local int g_last_hip_error = 0;

namespace {

constexpr uint32_t kProbBits = 16;
constexpr uint64_t kStateLow = 1ull << 31;
constexpr int kEncThreads = 256;  // 4 waves = 256 images per workgroup

// ---------------------------------------------------------------------------
// table staging: int32 cdf[C][W] (global) -> u16 [C][W] (LDS).  65536 wraps to 0,
// which is harmless: it is only ever used as the upper edge of the last bin and
// (hi - lo) & 0xffff recovers the frequency (< 65536 by construction).
// ---------------------------------------------------------------------------
__device__ __forceinline__ void stage_table(uint16_t *lds, const int32_t *__restrict__ cdf,
                                            int n_entries) {
  // 16-byte loads, four in flight per thread: written as `lds[i] = cdf[i]` the loop waits for every
  // 4-byte load before its ds_write (64 dependent L2 round trips per thread for a 512 x 32 table =
  // ~15 % of the encoder's time at batch 1024)
  const int quads = ((reinterpret_cast<uintptr_t>(cdf) & 15u) == 0) ? n_entries >> 2 : 0;
  const int4 *src = reinterpret_cast<const int4 *>(cdf);
  for (int i0 = threadIdx.x; i0 < quads; i0 += 4 * blockDim.x) {
    int4 q[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = i0 + u * blockDim.x;
      q[u] = i < quads ? src[i] : int4{0, 0, 0, 0};
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = i0 + u * blockDim.x;
      if (i < quads) {
        typedef unsigned short u16x4 __attribute__((ext_vector_type(4)));
        *reinterpret_cast<u16x4 *>(lds + 4 * i) =
            u16x4{(unsigned short)q[u].x, (unsigned short)q[u].y, (unsigned short)q[u].z, (unsigned short)q[u].w};
      }
    }
  }
  for (int i = 4 * quads + threadIdx.x; i < n_entries; i += blockDim.x) lds[i] = (uint16_t)cdf[i];
  __syncthreads();
}

// t / f and t % f for t < f * 2^16 (so the quotient is < 2^16), 1 <= f < 2^16.
// hipcc expands a u32 division into ~40 dependent instructions; here the quotient is
// estimated in fp32 and corrected, ~12 instructions.  Exactness: float(t) and v_rcp_f32 are
// each within 2^-23 relative, so the estimate is within q * 2^-21 < 1/32 of t / f and its
// floor is q - 1, q or q + 1; the remainder test below moves it to q in either case.
__device__ __forceinline__ void divmod16(uint32_t t, uint32_t f, uint32_t &q, uint32_t &r) {
  uint32_t qe = (uint32_t)((float)t * __builtin_amdgcn_rcpf((float)f));
  int32_t rem = (int32_t)(t - qe * f);  // |rem| < 2 f: fits, wrap-around is harmless
  if (rem < 0) { --qe; rem += (int32_t)f; }
  if (rem >= (int32_t)f) { ++qe; rem -= (int32_t)f; }
  q = qe;
  r = (uint32_t)rem;
}

// x / f and x % f for x < 2^47 * f, 1 <= f < 2^16, as three long-division steps in base 2^16
// (each partial dividend is < f * 2^16, which is what divmod16 needs).
// Returns (q << 16) + r, i.e. the rANS state before `start` is added.
__device__ __forceinline__ uint64_t div_step(uint64_t x, uint32_t f) {
  const uint32_t hi = (uint32_t)(x >> 32);
  const uint32_t lo = (uint32_t)x;
  uint32_t q1, r1, q2, r2, q3, r3;
  divmod16(hi, f, q1, r1);
  divmod16((r1 << 16) | (lo >> 16), f, q2, r2);
  divmod16((r2 << 16) | (lo & 0xffffu), f, q3, r3);
  // q = q1 * 2^32 + q2 * 2^16 + q3 ; result = q * 2^16 + r3
  return ((uint64_t)q1 << 48) | ((uint64_t)q2 << 32) | ((uint64_t)q3 << 16) | (uint64_t)r3;
}

struct __attribute__((aligned(16))) ChanParams {
  float bias, es, med;
  int32_t off;
  int32_t len;
  int32_t pad[3];
};
__host__ __device__ inline size_t enc_table_bytes(int C, int W) {
  return ((size_t)C * W * sizeof(uint16_t) + 15u) & ~(size_t)15u;
}
__host__ __device__ inline size_t enc_lds_bytes(int C, int W) {
  return enc_table_bytes(C, W) + (size_t)C * sizeof(ChanParams);
}

struct EncState {
  uint64_t x;
  uint32_t *wp;  // next free word is wp[-1]; stream grows towards lower addresses
};

__device__ __forceinline__ void put_symbol(EncState &s, uint32_t start, uint32_t freq) {
  // x >= ((2^31 >> 16) << 32) * freq = freq << 47; the bound's low word is 0: compare high words
  if ((uint32_t)(s.x >> 32) >= (freq << 15)) {
    *--s.wp = (uint32_t)s.x;
    s.x >>= 32;
  }
  s.x = div_step(s.x, freq) + start;
}

__device__ __forceinline__ void put_digit(EncState &s, uint32_t d) {
  if ((uint32_t)(s.x >> 32) >= (1u << 27)) {  // x >= ((2^31 >> 16) << 32) * 2^12 = 2^59
    *--s.wp = (uint32_t)s.x;
    s.x >>= 32;
  }
  s.x = (s.x << 4) | d;
}

// One channel of one image, in two halves so that the caller can run the state-independent half
// (table look-ups) for a whole group of channels before the serial state updates of that group:
// the LDS round trips of a group then overlap instead of sitting in the 512-step dependency chain.
struct Prepared {
  uint32_t start, freq, raw;
  int nd;  // -1: regular symbol; 0..8: escape with that many 4-bit payload digits
};

template <typename RowT>
__device__ __forceinline__ Prepared prepare_channel(const RowT *row, int len, int off, int32_t sym) {
  const int esc = len - 2;
  const int v0 = sym - off;
  const bool neg = v0 < 0, over = v0 >= esc, escaped = neg || over;
  Prepared p;
  p.raw = neg ? (uint32_t)(-2 * v0 - 1) : (over ? (uint32_t)(2 * (v0 - esc)) : 0u);
  // raw fits 32 bits -> at most 8 digits -> the count is a single digit (< 15)
  const int nd = p.raw ? (35 - __clz((int)p.raw)) >> 2 : 0;
  p.nd = escaped ? nd : -1;
  const int v = escaped ? esc : v0;
  p.start = (uint32_t)row[v];
  p.freq = ((uint32_t)row[v + 1] - p.start) & 0xffffu;  // 65536 (or its u16 wrap 0) minus start
  return p;
}

// Symbols are consumed last-to-first, so for an escaped value the payload digits go in
// most-significant first, then the digit count, then the escape symbol itself -- the mirror
// image of the decoder's read order.
__device__ __forceinline__ void emit_channel(EncState &s, const Prepared &p) {
  if (p.nd >= 0) {
    for (int d = p.nd - 1; d >= 0; --d) put_digit(s, (p.raw >> (4 * d)) & 15u);
    put_digit(s, (uint32_t)p.nd);
  }
  put_symbol(s, p.start, p.freq);
}

__device__ __forceinline__ int32_t quantise_one(float z, float bias, float es, float med) {
  // three separately rounded fp32 operations, then round-half-even
  const float t = __fadd_rn(z, bias);
  const float u = __fmul_rn(t, es);
  const float d = __fsub_rn(u, med);
  return (int32_t)rintf(d);
}

// ZMODE 0: int32 symbols, 1: fp16 z, 2: fp32 z.  G = channels fetched per 16-byte load.
template <int ZMODE>
struct Fetch;
template <>
struct Fetch<0> {
  static constexpr int G = 4;
  using elem = int32_t;
};
template <>
struct Fetch<1> {
  static constexpr int G = 8;
  using elem = __half;
};
template <>
struct Fetch<2> {
  static constexpr int G = 4;
  using elem = float;
};

template <int ZMODE>
__global__ __launch_bounds__(kEncThreads) void rans_encode_kernel(
    const void *__restrict__ in, int B, int C, const float *__restrict__ bias,
    const float *__restrict__ exp_scale, const float *__restrict__ median,
    const int32_t *__restrict__ cdf, int W, const int32_t *__restrict__ cdf_len,
    const int32_t *__restrict__ offset, uint8_t *__restrict__ scratch, size_t stride,
    uint32_t *__restrict__ lengths, int32_t *__restrict__ symbols_out) {
  kernel_acquire();
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  uint16_t *tab = reinterpret_cast<uint16_t *>(smem);
  // per-channel scalars next to the table: as uniform global reads they become s_load_dword,
  // which shares lgkmcnt with the LDS and returns out of order, so every use forced
  // s_waitcnt lgkmcnt(0) -- two scalar-memory round trips per symbol in the serial loop
  ChanParams *par = reinterpret_cast<ChanParams *>(smem + enc_table_bytes(C, W));
  for (int c = threadIdx.x; c < C; c += blockDim.x) {
    ChanParams q;
    q.bias = ZMODE ? bias[c] : 0.f;
    q.es = ZMODE ? exp_scale[c] : 0.f;
    q.med = ZMODE ? median[c] : 0.f;
    q.off = offset[c];
    q.len = cdf_len[c];
    par[c] = q;
  }
  stage_table(tab, cdf, C * W);

  const int img = blockIdx.x * kEncThreads + threadIdx.x;
  if (img >= B) return;

  using F = Fetch<ZMODE>;
  constexpr int G = F::G;
  using elem = typename F::elem;
  const elem *src = reinterpret_cast<const elem *>(in) + (size_t)img * C;

  uint8_t *end = scratch + (size_t)img * stride + stride;
  EncState s;
  s.x = kStateLow;
  s.wp = reinterpret_cast<uint32_t *>(end);

  auto prep = [&](int c, elem raw_in) {
    const ChanParams q = par[c];
    int32_t sym;
    if constexpr (ZMODE == 0) {
      sym = raw_in;
    } else if constexpr (ZMODE == 1) {
      sym = quantise_one(__half2float(raw_in), q.bias, q.es, q.med);
    } else {
      sym = quantise_one(raw_in, q.bias, q.es, q.med);
    }
    if (symbols_out) symbols_out[(size_t)img * C + c] = sym;
    return prepare_channel(tab + c * W, q.len, q.off, sym);
  };

  const int tail = C % G;
  for (int c = C - 1; c >= C - tail; --c) emit_channel(s, prep(c, src[c]));
  const bool vec_ok = ((reinterpret_cast<uintptr_t>(src) & 15u) == 0) && ((C - tail) > 0);
  for (int g = (C - tail) / G - 1; g >= 0; --g) {
    elem v[G];
    if (vec_ok) {
      *reinterpret_cast<uint4 *>(v) = *reinterpret_cast<const uint4 *>(src + g * G);
    } else {
#pragma unroll
      for (int k = 0; k < G; ++k) v[k] = src[g * G + k];
    }
    Prepared pr[G];
#pragma unroll
    for (int k = 0; k < G; ++k) pr[k] = prep(g * G + k, v[k]);
#pragma unroll
    for (int k = G - 1; k >= 0; --k) emit_channel(s, pr[k]);
  }

  s.wp -= 2;
  s.wp[0] = (uint32_t)s.x;
  s.wp[1] = (uint32_t)(s.x >> 32);
  lengths[img] = (uint32_t)(end - reinterpret_cast<uint8_t *>(s.wp));
}

// ---------------------------------------------------------------------------
// decode
// ---------------------------------------------------------------------------
struct DecState {
  uint64_t x;
  const uint32_t *w;
  uint32_t pos, nwords;
};

// (A 16-byte word window reloaded every fourth renormalisation, and four symbols per store, were both
// tried: the extra selects and divergent blocks on the serial per-symbol chain cost more than the
// vector-memory round trips they save -- 2.7 vs 3.1 M img/s at batch 1024.)
__device__ __forceinline__ void refill(DecState &s) {
  if (s.x < kStateLow) {
    const uint32_t word = s.pos < s.nwords ? s.w[s.pos] : 0u;
    s.x = (s.x << 32) | word;
    ++s.pos;
  }
}

__device__ __forceinline__ uint32_t take_digit(DecState &s) {
  const uint32_t d = (uint32_t)s.x & 15u;
  s.x >>= 4;
  refill(s);
  return d;
}

// Slot search over one CDF row: largest k in [0, len-2] with row[k] <= cf (row[len-1] stands for 65536
// and is never read; entries at or beyond it count as 65536).  The row sits in LDS (u16) or in global
// memory (int32); either way a classic binary search is a chain of log2(len) DEPENDENT reads, and with
// one stream per lane nothing else hides their latency.  Here three tree levels are resolved per round
// trip: the seven candidates at lo + step * {1..7} are requested together, then picked by compares and
// selects (span / 8 per round; the last round handles span 4 or 2).  A 32-entry row (every shipped
// table) takes 2 round trips instead of 5 + 1, a 3133-entry scale-table row 4 instead of 12.
// Returns the slot and the two edges it lies between.
template <typename RowT>
__device__ __forceinline__ int search_row(const RowT *row, int len, uint32_t cf, uint32_t &start,
                                          uint32_t &next) {
  const int last = len - 1;   // first index that counts as 65536
  int span = 2;               // smallest power of two >= len - 1 (>= 2): wave-uniform
  while (span < last) span <<= 1;
  int lo = 0;
  uint32_t vlo = 0u, vhi = 65536u;
  // candidates lo + step * (j + 1), j < N: ALL reads are issued before the first value is looked at
  // (left to itself hipcc waits for each read in front of the select that patches the 65536 sentinel in)
  auto fetch = [&](auto n_c, int step, uint32_t (&v)[7]) {
    constexpr int N = decltype(n_c)::value;
    uint32_t raw[7];
#pragma unroll
    for (int j = 0; j < N; ++j) {
      const int i = lo + step * (j + 1);
      raw[j] = (uint32_t)row[i < last ? i : 0];
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int j = 0; j < N; ++j) v[j] = lo + step * (j + 1) < last ? raw[j] : 65536u;
  };
  auto take = [&](bool le, uint32_t v) {
    vlo = le ? v : vlo;
    vhi = le ? vhi : v;
  };
  uint32_t v[7];
  while (span >= 8) {
    const int step = span >> 3;
    fetch(std::integral_constant<int, 7>{}, step, v);
    const bool c4 = v[3] <= cf;
    take(c4, v[3]);
    const uint32_t m2 = c4 ? v[5] : v[1];
    const bool c2 = m2 <= cf;
    take(c2, m2);
    const uint32_t m1 = c4 ? (c2 ? v[6] : v[4]) : (c2 ? v[2] : v[0]);
    const bool c1 = m1 <= cf;
    take(c1, m1);
    lo += step * ((c4 ? 4 : 0) + (c2 ? 2 : 0) + (c1 ? 1 : 0));
    span = step;
  }
  if (span == 4) {
    fetch(std::integral_constant<int, 3>{}, 1, v);
    const bool c2 = v[1] <= cf;
    take(c2, v[1]);
    const uint32_t m1 = c2 ? v[2] : v[0];
    const bool c1 = m1 <= cf;
    take(c1, m1);
    lo += (c2 ? 2 : 0) + (c1 ? 1 : 0);
  } else if (span == 2) {
    fetch(std::integral_constant<int, 1>{}, 1, v);
    const bool c1 = v[0] <= cf;
    take(c1, v[0]);
    lo += c1 ? 1 : 0;
  }
  start = vlo;
  next = vhi;
  return lo;
}

// The plain binary search: for the short rows of the factorized model (<= 33 entries in LDS, 5 steps)
// it measured faster than the three-levels-per-round-trip search above (3.1 vs 2.7 M img/s at batch
// 1024: fewer instructions on the serial chain matter more than two LDS round trips).
template <typename RowT>
__device__ __forceinline__ int search_row_binary(const RowT *row, int len, uint32_t cf, uint32_t &start,
                                                 uint32_t &next) {
  int lo = 0, hi = len - 1;
  uint32_t vlo = 0u, vhi = 65536u;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    const uint32_t v = (uint32_t)row[mid];   // mid <= len-2: the 65536 entry is never read
    const bool le = v <= cf;
    lo = le ? mid : lo;
    hi = le ? hi : mid;
    vlo = le ? v : vlo;
    vhi = le ? vhi : v;
  }
  start = vlo;
  next = vhi;
  return lo;
}

// One symbol off the stream: search the row, advance the state, read escape digits.
template <bool TREE, typename RowT>
__device__ __forceinline__ int32_t decode_symbol(DecState &s, const RowT *row, int len) {
  const int esc = len - 2;
  const uint32_t cf = (uint32_t)s.x & 0xffffu;
  uint32_t start, next;
  const int lo = TREE ? search_row(row, len, cf, start, next) : search_row_binary(row, len, cf, start, next);
  const uint32_t freq = next - start;
  s.x = (uint64_t)freq * (s.x >> kProbBits) + cf - start;
  refill(s);
  int32_t v = lo;
  if (lo == esc) {
    uint32_t d = take_digit(s);
    uint32_t nd = d;
    while (d == 15u && nd < 64u) {
      d = take_digit(s);
      nd += d;
    }
    uint32_t raw = 0;
    for (uint32_t j = 0; j < nd; ++j) {
      d = take_digit(s);
      if (j < 8) raw |= d << (4 * j);
    }
    const int32_t sraw = (int32_t)raw;
    v = sraw >> 1;
    v = (sraw & 1) ? -v - 1 : v + esc;
  }
  return v;
}

__device__ __forceinline__ bool open_stream(DecState &s, const uint8_t *payload, const uint64_t *off,
                                            int skip, size_t i) {
  const uint64_t begin = off[i] + (uint64_t)skip;
  const uint64_t endb = off[i + 1];
  s.w = reinterpret_cast<const uint32_t *>(payload + begin);
  s.nwords = endb > begin ? (uint32_t)((endb - begin) >> 2) : 0u;
  if (s.nwords < 2 || ((endb - begin) & 3u) || (reinterpret_cast<uintptr_t>(s.w) & 3u)) return false;
  s.x = (uint64_t)s.w[0] | ((uint64_t)s.w[1] << 32);
  s.pos = 2;
  return true;
}

__global__ __launch_bounds__(kEncThreads) void rans_decode_kernel(
    const uint8_t *__restrict__ payload, const uint64_t *__restrict__ off, int skip, int off_step, int B, int C,
    const int32_t *__restrict__ cdf, int W, const int32_t *__restrict__ cdf_len,
    const int32_t *__restrict__ offset, int32_t *__restrict__ out, int32_t *__restrict__ status) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  uint16_t *tab = reinterpret_cast<uint16_t *>(smem);
  // (cdf length, offset) per channel in LDS: see the encoder for why not uniform global reads
  int2 *par = reinterpret_cast<int2 *>(smem + enc_table_bytes(C, W));
  for (int c = threadIdx.x; c < C; c += blockDim.x) par[c] = make_int2(cdf_len[c], offset[c]);
  stage_table(tab, cdf, C * W);

  const int img = blockIdx.x * kEncThreads + threadIdx.x;
  if (img >= B) return;

  DecState s;
  int32_t *dst = out + (size_t)img * C;
  if (!open_stream(s, payload, off, skip & 0xff, img * off_step)) {
    for (int c = 0; c < C; ++c) dst[c] = 0;
    if (status) status[img] = 1;
    return;
  }
  for (int c = 0; c < C; ++c) {
    const int2 q = par[c];
    dst[c] = decode_symbol<false>(s, tab + c * W, q.x) + q.y;
  }
  if (status) status[img] = s.pos > s.nwords ? 1 : 0;
}

// ---------------------------------------------------------------------------
// Gather + decode + dequantise: lane b of the launch decodes record index[b] (random access into a container
// body that stays compressed in device memory) and the workgroup writes the dequantised rows.  One stream per
// lane as above; the symbols never leave the registers.  A lane that stored its own row would put 64 separate
// cache lines behind every store of a wave (rows are 2 KB apart), so the values take the indexed decoder's
// LDS staging in the opposite direction: every lane parks kGatherG channels of its row in LDS, then the
// workgroup writes them out with four consecutive lanes covering the 64 contiguous bytes (fp32) one row has in
// the group.
//   staging: [256 lanes][kGatherG floats] in 16-byte chunks; lane L's chunk j sits at slot (j + (L >> 1)) & 3 of
//   its 64-byte line.  A ds_write_b128 is served in groups of 8 consecutive lanes over 32 banks; their lines are 64
//   bytes apart, so without the rotation lanes L, L+2, L+4, L+6 meet in the same four banks (4-way conflict); with it
//   the eight chunks cover the 32 banks once.  The write-out reads whole lines (4 threads per line, every chunk once).
// LDS at C = 512, W = 33: table 33 792 + parameters 512 x 20 = 10 240 + staging 16 384 = 60 416 bytes.
// ---------------------------------------------------------------------------
constexpr int kGatherG = 16;
__device__ __forceinline__ float dequantise_one(float q, float bias, float es, float med);   // (with the elementwise kernels, below)
struct __attribute__((aligned(16))) GatherParams {
  float bias, es, med;
  int32_t off;
};
__host__ __device__ inline size_t gather_lds_bytes(int C, int W) {
  return enc_table_bytes(C, W) + (size_t)C * sizeof(GatherParams) + (((size_t)C * sizeof(int32_t) + 15u) & ~(size_t)15u) +
         (size_t)kEncThreads * kGatherG * sizeof(float);
}

__device__ __forceinline__ void store_out(float *p, float v) { *p = v; }
__device__ __forceinline__ void store_out(__half *p, float v) { *p = __float2half_rn(v); }
__device__ __forceinline__ void store_out4(float *p, const float4 &v) { *reinterpret_cast<float4 *>(p) = v; }
__device__ __forceinline__ void store_out4(__half *p, const float4 &v) {
  const __half2 a = __floats2half2_rn(v.x, v.y), b = __floats2half2_rn(v.z, v.w);
  *reinterpret_cast<uint2 *>(p) = uint2{__builtin_bit_cast(uint32_t, a), __builtin_bit_cast(uint32_t, b)};
}

template <typename OutT>
__global__ __launch_bounds__(kEncThreads) void rans_decode_gather_kernel(
    const uint8_t *__restrict__ payload, const uint64_t *__restrict__ off, int skip, int off_first, int off_step, int N,
    const int64_t *__restrict__ index, int B, int C, const int32_t *__restrict__ cdf, int W,
    const int32_t *__restrict__ cdf_len, const int32_t *__restrict__ offset, const float *__restrict__ bias,
    const float *__restrict__ exp_scale, const float *__restrict__ median, OutT *__restrict__ out, size_t ld_out,
    int32_t *__restrict__ status) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  uint16_t *tab = reinterpret_cast<uint16_t *>(smem);
  GatherParams *par = reinterpret_cast<GatherParams *>(smem + enc_table_bytes(C, W));
  int32_t *len = reinterpret_cast<int32_t *>(par + C);
  float4 *stage = reinterpret_cast<float4 *>(smem + gather_lds_bytes(C, W) -
                                             (size_t)kEncThreads * kGatherG * sizeof(float));
  for (int c = threadIdx.x; c < C; c += blockDim.x) {
    par[c] = GatherParams{bias[c], exp_scale[c], median[c], offset[c]};
    len[c] = cdf_len[c];
  }
  stage_table(tab, cdf, C * W);

  // No lane leaves before the last barrier: one without a record (past B, index out of range, stream unopenable)
  // parks zeros, which is also what its row must hold.
  const int lane = threadIdx.x;
  const int row0 = blockIdx.x * kEncThreads;
  const int img = row0 + lane;
  int st = 0;
  bool live = false;
  DecState s;
  if (img < B) {
    // image index[img] is record off_first + index * off_step: in 64 bits, and only once the index is known to be in
    // [0, N) (the product is then below 2^62)
    const int64_t rec = index[img];
    if (rec < 0 || rec >= (int64_t)N) st = 2;
    else if (!open_stream(s, payload, off, skip, (size_t)((int64_t)off_first + rec * (int64_t)off_step))) st = 1;
    live = st == 0;
  }

  constexpr int kChunks = kGatherG / 4;                 // 16-byte chunks per staged line
  const int rot = lane >> 1;
  // write-out: 4 threads per row (one chunk each), 64 rows per pass
  const int wr = lane >> 2, wj = lane & 3;
  const bool vec_ok = (reinterpret_cast<uintptr_t>(out) % (4 * sizeof(OutT)) == 0) && (ld_out % 4 == 0);
  const int rows_here = min(kEncThreads, B - row0);

  for (int c0 = 0; c0 < C; c0 += kGatherG) {
    float v[kGatherG];
#pragma unroll
    for (int k = 0; k < kGatherG; ++k) {
      const int c = c0 + k;
      v[k] = 0.f;
      if (live && c < C) {
        const GatherParams q = par[c];
        const int32_t sym = decode_symbol<false>(s, tab + c * W, len[c]) + q.off;
        v[k] = dequantise_one((float)sym, q.bias, q.es, q.med);
      }
    }
#pragma unroll
    for (int j = 0; j < kChunks; ++j)
      stage[lane * kChunks + ((j + rot) & 3)] = float4{v[4 * j], v[4 * j + 1], v[4 * j + 2], v[4 * j + 3]};
    __syncthreads();
    const int c = c0 + 4 * wj;
#pragma unroll
    for (int p = 0; p < kEncThreads / 64; ++p) {
      const int r = p * 64 + wr;
      if (r < rows_here && c < C) {
        const float4 q = stage[r * kChunks + ((wj + (r >> 1)) & 3)];
        OutT *dst = out + (size_t)(row0 + r) * ld_out + c;
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
    __syncthreads();
  }

  if (live && s.pos > s.nwords) st = 1;
  if (img < B && status) status[img] = st;
  // A stream that overran is known only now, after other lanes have written its row: once those stores have
  // completed (agent-scope fence in every thread, then the barrier), its own lane zeroes the row.  Rare path.
  if (__syncthreads_or(live && st == 1)) {
    __threadfence();
    __syncthreads();
    if (live && st == 1) {
      OutT *dst = out + (size_t)img * ld_out;
      for (int c = 0; c < C; ++c) store_out(dst + c, 0.f);
    }
  }
}

// ---------------------------------------------------------------------------
// Arbitrary table row per symbol (compressai encode_with_indexes / decode_with_indexes as
// GaussianConditional uses them: lossyless/rates.py:694-729).  One string per lane; rows are
// read from global memory (a 64-level scale table is T x W = 64 x ~3100 int32, too large for
// LDS, and the rows differ per lane anyway).  Row indexes are clamped to [0, T).
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kEncThreads) void rans_encode_indexed_kernel(
    const int32_t *__restrict__ symbols, const int32_t *__restrict__ indexes, int B, int n,
    const int32_t *__restrict__ cdf, int T, int W, const int32_t *__restrict__ cdf_len,
    const int32_t *__restrict__ offset, uint8_t *__restrict__ scratch, size_t stride,
    uint32_t *__restrict__ lengths) {
  const int i = blockIdx.x * kEncThreads + threadIdx.x;
  if (i >= B) return;
  const int32_t *sym = symbols + (size_t)i * n;
  const int32_t *idx = indexes + (size_t)i * n;
  uint8_t *end = scratch + (size_t)i * stride + stride;
  EncState s;
  s.x = kStateLow;
  s.wp = reinterpret_cast<uint32_t *>(end);
  constexpr int G = 4;
  auto prep = [&](int k) {
    const int t = min(max(idx[k], 0), T - 1);
    return prepare_channel(cdf + (size_t)t * W, cdf_len[t], offset[t], sym[k]);
  };
  const int tail = n % G;
  for (int k = n - 1; k >= n - tail; --k) emit_channel(s, prep(k));
  for (int g = (n - tail) / G - 1; g >= 0; --g) {
    Prepared pr[G];
#pragma unroll
    for (int k = 0; k < G; ++k) pr[k] = prep(g * G + k);
#pragma unroll
    for (int k = G - 1; k >= 0; --k) emit_channel(s, pr[k]);
  }
  s.wp -= 2;
  s.wp[0] = (uint32_t)s.x;
  s.wp[1] = (uint32_t)(s.x >> 32);
  lengths[i] = (uint32_t)(end - reinterpret_cast<uint8_t *>(s.wp));
}

// Decoder: the rows are searched, not just indexed, so their latency sits on every symbol's critical
// path.  All T rows are therefore packed back to back into LDS as u16 (only their cdf_len[t] valid
// entries: the 64-level scale table of lossyless/rates.py:567-569 is 64 x 3133 int32 = 800 KB padded
// but ~27 000 valid entries = 54 KB) and searched there; when they do not fit the LDS the kernel was
// given, the rows are searched in global memory (same code, int32 rows).
struct PackedRows {
  uint32_t *rowoff;   // [T+1] row starts (u32)
  int2 *par;          // [T] (len, offset)
  uint16_t *tab;      // packed rows (u16)
  bool in_lds;        // uniform: the rows fit the LDS the kernel was given
};
__host__ __device__ inline size_t packed_rows_head(int T) {
  return (((size_t)(T + 1) * 4 + 7) & ~(size_t)7) + (size_t)T * sizeof(int2);
}
// Called by every thread of the workgroup (barriers inside).  smem must be 8-byte aligned.
__device__ __forceinline__ PackedRows stage_packed_rows(uint8_t *smem, unsigned lds_bytes,
                                                        const int32_t *__restrict__ cdf, int T, int W,
                                                        const int32_t *__restrict__ cdf_len,
                                                        const int32_t *__restrict__ offset) {
  PackedRows r;
  r.rowoff = reinterpret_cast<uint32_t *>(smem);
  r.par = reinterpret_cast<int2 *>(smem + (((size_t)(T + 1) * 4 + 7) & ~(size_t)7));
  r.tab = reinterpret_cast<uint16_t *>(reinterpret_cast<uint8_t *>(r.par) + (size_t)T * sizeof(int2));
  const size_t head = packed_rows_head(T);
  r.in_lds = head < lds_bytes;
  if (r.in_lds) {
    for (int t = threadIdx.x; t < T; t += blockDim.x) r.par[t] = make_int2(min(max(cdf_len[t], 3), W), offset[t]);
    __syncthreads();
    if (threadIdx.x == 0) {
      uint32_t acc = 0;
      for (int t = 0; t < T; ++t) { r.rowoff[t] = acc; acc += (uint32_t)r.par[t].x; }
      r.rowoff[T] = acc;
    }
    __syncthreads();
    r.in_lds = head + (size_t)r.rowoff[T] * 2 <= lds_bytes;   // uniform
    if (r.in_lds) {
      for (int t = 0; t < T; ++t) {
        const int len = r.par[t].x;
        const int32_t *src = cdf + (size_t)t * W;
        uint16_t *dst = r.tab + r.rowoff[t];
        for (int i = threadIdx.x; i < len; i += blockDim.x) dst[i] = (uint16_t)src[i];
      }
      __syncthreads();
    }
  }
  return r;
}

__global__ __launch_bounds__(kEncThreads) void rans_decode_indexed_kernel(
    const uint8_t *__restrict__ payload, const uint64_t *__restrict__ off, int skip, int B, int n,
    const int32_t *__restrict__ indexes, const int32_t *__restrict__ cdf, int T, int W,
    const int32_t *__restrict__ cdf_len, const int32_t *__restrict__ offset,
    int32_t *__restrict__ out, int32_t *__restrict__ status, unsigned lds_bytes) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const PackedRows rows = stage_packed_rows(smem, lds_bytes, cdf, T, W, cdf_len, offset);
  const bool in_lds = rows.in_lds;
  const uint32_t *rowoff = rows.rowoff;
  const int2 *par = rows.par;
  const uint16_t *tab = rows.tab;
  const int i = blockIdx.x * kEncThreads + threadIdx.x;
  if (i >= B) return;
  DecState s;
  int32_t *dst = out + (size_t)i * n;
  if (!open_stream(s, payload, off, skip, i)) {
    for (int k = 0; k < n; ++k) dst[k] = 0;
    if (status) status[i] = 1;
    return;
  }
  const int32_t *idx = indexes + (size_t)i * n;
  if (in_lds) {
    int t_next = min(max(idx[0], 0), T - 1);
    for (int k = 0; k < n; ++k) {
      const int t = t_next;
      if (k + 1 < n) t_next = min(max(idx[k + 1], 0), T - 1);   // (requested one symbol ahead)
      const int2 q = par[t];
      dst[k] = decode_symbol<true>(s, tab + rowoff[t], q.x) + q.y;
    }
  } else {
    for (int k = 0; k < n; ++k) {
      const int t = min(max(idx[k], 0), T - 1);
      dst[k] = decode_symbol<true>(s, cdf + (size_t)t * W, min(max(cdf_len[t], 3), W)) + offset[t];   // (same clamp as the LDS path)
    }
  }
  if (status) status[i] = s.pos > s.nwords ? 1 : 0;
}

// ---------------------------------------------------------------------------
// elementwise: quantise / dequantise / represent
// ---------------------------------------------------------------------------
template <int ZMODE>
__global__ void quantise_kernel(const void *__restrict__ z, size_t n, int C,
                                const float *__restrict__ bias, const float *__restrict__ es,
                                const float *__restrict__ med, int32_t *__restrict__ sym) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (size_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % (size_t)C);
    float v;
    if constexpr (ZMODE == 1) v = __half2float(reinterpret_cast<const __half *>(z)[i]);
    else v = reinterpret_cast<const float *>(z)[i];
    sym[i] = quantise_one(v, bias[c], es[c], med[c]);
  }
}

__device__ __forceinline__ float dequantise_one(float q, float bias, float es, float med) {
  const float zh = __fadd_rn(q, med);
  return __fsub_rn(__fdiv_rn(zh, es), bias);
}

__global__ void dequantise_kernel(const int32_t *__restrict__ sym, size_t n, int C,
                                  const float *__restrict__ bias, const float *__restrict__ es,
                                  const float *__restrict__ med, float *__restrict__ out) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (size_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % (size_t)C);
    out[i] = dequantise_one((float)sym[i], bias[c], es[c], med[c]);
  }
}

template <int ZMODE>
__global__ void represent_kernel(const void *__restrict__ z, size_t n, int C,
                                 const float *__restrict__ bias, const float *__restrict__ es,
                                 const float *__restrict__ med, float *__restrict__ out) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (size_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % (size_t)C);
    float v;
    if constexpr (ZMODE == 1) v = __half2float(reinterpret_cast<const __half *>(z)[i]);
    else v = reinterpret_cast<const float *>(z)[i];
    const float t = __fadd_rn(v, bias[c]);
    const float u = __fmul_rn(t, es[c]);
    const float q = rintf(__fsub_rn(u, med[c]));  // EntropyBottleneck.forward, eval mode
    out[i] = dequantise_one(q, bias[c], es[c], med[c]);
  }
}

// ---------------------------------------------------------------------------
// Scale hyperprior, conditional part (lossyless/rates.py:694-729): the table row AND the mean of every element
// come from the predicted scale, so subtract / round / build_indexes / code (and decode / add / process_z_out)
// are one kernel each.  One image per lane as above; rows are read from global memory by the encoder (one
// look-up per symbol, off the state's dependency chain) and searched in LDS by the decoder.
// ---------------------------------------------------------------------------
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
__device__ __forceinline__ void scale_rows(const float *stab, int T, float bound, const float (&scale)[G],
                                           int (&row)[G]) {
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
  for (int t = threadIdx.x; t < T; t += blockDim.x) par[t] = make_int2(min(max(cdf_len[t], 3), W), offset[t]);
  __syncthreads();

  const int img = blockIdx.x * kEncThreads + threadIdx.x;
  if (img >= B) return;

  using F = Fetch<ZMODE>;
  constexpr int G = F::G;
  using elem = typename F::elem;
  const elem *src = reinterpret_cast<const elem *>(in) + (size_t)img * C;
  const float *sc = scales + (size_t)img * ld_scales;
  [[maybe_unused]] const float *mn = mean_row((size_t)img, means...);

  uint8_t *end = scratch + (size_t)img * stride + stride;
  EncState s;
  s.x = kStateLow;
  s.wp = reinterpret_cast<uint32_t *>(end);

  auto prep = [&](int c, elem raw_in, float mean, int t) {
    const AffineParams a = aff[c];
    float zf;
    if constexpr (ZMODE == 1) zf = __half2float(raw_in);
    else zf = raw_in;
    // (z + bias) * exp_scale - mean, three separately rounded operations; without kMeans the mean IS the predicted
    // scale, unbounded
    const int32_t sym = quantise_one(zf, a.bias, a.es, mean);
    if (symbols_out) symbols_out[(size_t)img * C + c] = sym;
    if (indexes_out) indexes_out[(size_t)img * C + c] = t;
    const int2 q = par[t];
    return prepare_channel(cdf + (size_t)t * W, q.x, q.y, sym);
  };

  const int tail = C % G;
  for (int c = C - 1; c >= C - tail; --c) {
    const float sv[1] = {sc[c]};
    int t[1];
    scale_rows<1>(stab, T, scale_bound, sv, t);
    float mean = sv[0];
    if constexpr (kMeans) mean = mn[c];
    emit_channel(s, prep(c, src[c], mean, t[0]));
  }
  const bool vec_z = (reinterpret_cast<uintptr_t>(src) & 15u) == 0;
  const bool vec_s = (reinterpret_cast<uintptr_t>(sc) & 15u) == 0;
  // (means = scales + C is the caller's layout: for C % 4 != 0 the two rows are not aligned alike)
  [[maybe_unused]] const bool vec_m = (reinterpret_cast<uintptr_t>(mn) & 15u) == 0;
  for (int g = (C - tail) / G - 1; g >= 0; --g) {
    elem v[G];
    float sv[G];
    if (vec_z) {
      *reinterpret_cast<uint4 *>(v) = *reinterpret_cast<const uint4 *>(src + g * G);
    } else {
#pragma unroll
      for (int k = 0; k < G; ++k) v[k] = src[g * G + k];
    }
    if (vec_s) {
#pragma unroll
      for (int k = 0; k < G; k += 4)
        *reinterpret_cast<float4 *>(sv + k) = *reinterpret_cast<const float4 *>(sc + g * G + k);
    } else {
#pragma unroll
      for (int k = 0; k < G; ++k) sv[k] = sc[g * G + k];
    }
    int t[G];
    scale_rows<G>(stab, T, scale_bound, sv, t);
    Prepared pr[G];
    if constexpr (kMeans) {
      float mv[G];
      if (vec_m) {
#pragma unroll
        for (int k = 0; k < G; k += 4)
          *reinterpret_cast<float4 *>(mv + k) = *reinterpret_cast<const float4 *>(mn + g * G + k);
      } else {
#pragma unroll
        for (int k = 0; k < G; ++k) mv[k] = mn[g * G + k];
      }
#pragma unroll
      for (int k = 0; k < G; ++k) pr[k] = prep(g * G + k, v[k], mv[k], t[k]);
    } else {
#pragma unroll
      for (int k = 0; k < G; ++k) pr[k] = prep(g * G + k, v[k], sv[k], t[k]);
    }
#pragma unroll
    for (int k = G - 1; k >= 0; --k) emit_channel(s, pr[k]);
  }

  s.wp -= 2;
  s.wp[0] = (uint32_t)s.x;
  s.wp[1] = (uint32_t)(s.x >> 32);
  lengths[img] = (uint32_t)(end - reinterpret_cast<uint8_t *>(s.wp));
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
      int32_t sym;
      if (rows.in_lds) {
        const int2 q = rows.par[t[k]];
        sym = decode_symbol<true>(s, rows.tab + rows.rowoff[t[k]], q.x) + q.y;
      } else {
        sym = decode_symbol<true>(s, cdf + (size_t)t[k] * W, min(max(cdf_len[t[k]], 3), W)) + offset[t[k]];
      }
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
// go lane by lane through 2 KB-apart rows.  Both take rans_decode_gather_kernel's staging (same 16-byte chunks, same
// rotation by lane >> 1, four threads per 64-byte line):
//   scales  global -> LDS: the workgroup reads the 256 x kGatherG block of group g + 1 with 16-byte loads (four
//           consecutive threads cover the 64 contiguous bytes a row has in the group) BEFORE it decodes group g, and
//           parks it after; every lane then takes its own row from LDS.  Two buffers: a fast wave parks group g + 1
//           while a slow one may still be reading group g.
//   values  LDS -> global: as in rans_decode_gather_kernel.
// LDS in front of the packed rows: gauss_head_bytes + 16 + 3 x 256 x kGatherG x 4 = 4 352 + 16 + 49 152 bytes at C = 512,
// T = 64.  No static LDS (the vote is a word of the dynamic block, not __syncthreads_or's array): the launch may ask for
// the whole opt-in limit, as gaussian_decode_kernel does.
// Every lane reaches every barrier; a lane without a record (past B, status_in set, index out of range, stream
// unopenable) skips the decode and parks zeros.
// ---------------------------------------------------------------------------
// With means (MeanRows, see gaussian_encode_kernel) they take the scales' road through two buffers of their own, in front
// of the scales' (+ 32 768 bytes), and a row whose status_in is set is left out of BOTH block reads.
constexpr size_t kGatherStageBytes = (size_t)kEncThreads * kGatherG * sizeof(float);
__host__ __device__ inline size_t gauss_gather_front(int C, int T, int stages = 3) {
  return ((gauss_head_bytes(C, T) + 15u) & ~(size_t)15u) + 16 + stages * kGatherStageBytes;   // (16: the overrun vote)
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
  int *vote = reinterpret_cast<int *>(smem + front - kStages * kGatherStageBytes - 16);
  stage_gauss_head(smem, C, T, bias, exp_scale, scale_table);
  if (threadIdx.x == 0) *vote = 0;
  __syncthreads();
  const PackedRows rows = stage_packed_rows(smem + front, lds_bytes - (unsigned)front, cdf, T, W, cdf_len, offset);

  const int lane = threadIdx.x;
  const int row0 = blockIdx.x * kEncThreads;
  const int img = row0 + lane;
  int st = 0;
  bool live = false;
  DecState s;
  if (img < B) {
    const int64_t rec = index[img];
    if (status_in && status_in[img] != 0) st = status_in[img];
    else if (rec < 0 || rec >= (int64_t)N) st = 2;
    else if (!open_stream(s, payload, off, skip, (size_t)((int64_t)off_first + rec * (int64_t)off_step))) st = 1;
    live = st == 0;
  }

  constexpr int kChunks = kGatherG / 4;                 // 16-byte chunks per staged line
  constexpr int kPasses = kEncThreads / 64;             // 4 threads per row, 64 rows per pass
  const int rot = lane >> 1;
  const int wr = lane >> 2, wj = lane & 3;
  const bool vec_ok = (reinterpret_cast<uintptr_t>(out) % (4 * sizeof(OutT)) == 0) && (ld_out % 4 == 0);
  const bool vec_in = ((reinterpret_cast<uintptr_t>(scales) & 15u) == 0) && (ld_scales % 4 == 0);
  const int rows_here = min(kEncThreads, B - row0);
  // kMeans: bit p = row p * 64 + wr has its status_in set, and neither block read touches it
  [[maybe_unused]] unsigned dead = 0;
  if constexpr (kMeans) {
    if (status_in) {
#pragma unroll
      for (int p = 0; p < kPasses; ++p) {
        const int r = p * 64 + wr;
        if (r < rows_here && status_in[row0 + r] != 0) dead |= 1u << p;
      }
    }
  }

  // this thread's share of the scales block of the group at c0: chunk wj of rows p * 64 + wr (zeros outside B x C)
  auto fetch = [&](int c0, float4 (&q)[kPasses]) {
    const int c = c0 + 4 * wj;
#pragma unroll
    for (int p = 0; p < kPasses; ++p) {
      const int r = p * 64 + wr;
      q[p] = float4{0.f, 0.f, 0.f, 0.f};
      if (r < rows_here && c < C) {
        if constexpr (kMeans) {
          if ((dead >> p) & 1u) continue;
        }
        const float *src = scales + (size_t)(row0 + r) * ld_scales + c;
        if (vec_in && c + 3 < C) {
          q[p] = *reinterpret_cast<const float4 *>(src);
        } else {
          q[p].x = src[0];
          if (c + 1 < C) q[p].y = src[1];
          if (c + 2 < C) q[p].z = src[2];
          if (c + 3 < C) q[p].w = src[3];
        }
      }
    }
  };
  // ... and of the means block (kMeans), whose base may be aligned otherwise: the same walk.  (A second lambda, not one
  // with the matrix as an argument: that form changed the register allocation of the instantiations without means.)
  [[maybe_unused]] const float *mbase = mean_row(0, means...);
  [[maybe_unused]] const size_t ld_means = mean_ld(means...);
  [[maybe_unused]] const bool vec_mn = ((reinterpret_cast<uintptr_t>(mbase) & 15u) == 0) && (ld_means % 4 == 0);
  [[maybe_unused]] auto fetch_means = [&](int c0, float4 (&q)[kPasses]) {
    const int c = c0 + 4 * wj;
#pragma unroll
    for (int p = 0; p < kPasses; ++p) {
      const int r = p * 64 + wr;
      q[p] = float4{0.f, 0.f, 0.f, 0.f};
      if (r < rows_here && c < C && !((dead >> p) & 1u)) {
        const float *src = mbase + (size_t)(row0 + r) * ld_means + c;
        if (vec_mn && c + 3 < C) {
          q[p] = *reinterpret_cast<const float4 *>(src);
        } else {
          q[p].x = src[0];
          if (c + 1 < C) q[p].y = src[1];
          if (c + 2 < C) q[p].z = src[2];
          if (c + 3 < C) q[p].w = src[3];
        }
      }
    }
  };
  auto park = [&](float4 *buf, const float4 (&q)[kPasses]) {
#pragma unroll
    for (int p = 0; p < kPasses; ++p) {
      const int r = p * 64 + wr;
      buf[r * kChunks + ((wj + (r >> 1)) & 3)] = q[p];
    }
  };

  float4 nx[kPasses];
  [[maybe_unused]] float4 mx[kPasses];
  fetch(0, nx);
  park(sstage, nx);
  if constexpr (kMeans) {
    fetch_means(0, mx);
    park(mstage, mx);
  }
  __syncthreads();

  int g = 0;
  for (int c0 = 0; c0 < C; c0 += kGatherG, ++g) {
    const float4 *sbuf = sstage + (size_t)(g & 1) * kEncThreads * kChunks;
    const bool more = c0 + kGatherG < C;               // (uniform)
    if (more) fetch(c0 + kGatherG, nx);                // in flight under this group's decode
    [[maybe_unused]] const float4 *mbuf = mstage + (size_t)(g & 1) * kEncThreads * kChunks;
    [[maybe_unused]] float4 qm;
    if constexpr (kMeans) {
      if (more) fetch_means(c0 + kGatherG, mx);
      qm = mbuf[lane * kChunks + (rot & 3)];
    }

    // the lane's own line, one 16-byte chunk (four channels) at a time as gaussian_decode_kernel walks a row: the rows
    // of four elements are counted together, the next chunk's scales are requested ahead of the serial decode.  (Not
    // unrolled over the chunks: sixteen copies of the tree search would not help a chain that waits on the LDS.)
    float4 qs = sbuf[lane * kChunks + (rot & 3)];
#pragma unroll 1
    for (int j = 0; j < kChunks; ++j) {
      const float sv[4] = {qs.x, qs.y, qs.z, qs.w};
      if (j + 1 < kChunks) qs = sbuf[lane * kChunks + ((j + 1 + rot) & 3)];
      [[maybe_unused]] float mv[4];
      if constexpr (kMeans) {
        mv[0] = qm.x, mv[1] = qm.y, mv[2] = qm.z, mv[3] = qm.w;
        if (j + 1 < kChunks) qm = mbuf[lane * kChunks + ((j + 1 + rot) & 3)];
      }
      float v[4] = {0.f, 0.f, 0.f, 0.f};
      if (live) {
        int t[4];
        scale_rows<4>(stab, T, scale_bound, sv, t);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int c = c0 + 4 * j + k;
          if (c >= C) break;
          int32_t sym;
          if (rows.in_lds) {
            const int2 q = rows.par[t[k]];
            sym = decode_symbol<true>(s, rows.tab + rows.rowoff[t[k]], q.x) + q.y;
          } else {
            sym = decode_symbol<true>(s, cdf + (size_t)t[k] * W, min(max(cdf_len[t[k]], 3), W)) + offset[t[k]];
          }
          const AffineParams a = aff[c];
          float mean = sv[k];
          if constexpr (kMeans) mean = mv[k];
          v[k] = dequantise_one((float)sym, a.bias, a.es, mean);   // (sym + mean) / exp_scale - bias
        }
      }
      stage[lane * kChunks + ((j + rot) & 3)] = float4{v[0], v[1], v[2], v[3]};
    }
    if (more) park(sstage + (size_t)((g + 1) & 1) * kEncThreads * kChunks, nx);
    if constexpr (kMeans) {
      if (more) park(mstage + (size_t)((g + 1) & 1) * kEncThreads * kChunks, mx);
    }
    __syncthreads();
    const int c = c0 + 4 * wj;
#pragma unroll
    for (int p = 0; p < kPasses; ++p) {
      const int r = p * 64 + wr;
      if (r < rows_here && c < C) {
        const float4 q = stage[r * kChunks + ((wj + (r >> 1)) & 3)];
        OutT *dst = out + (size_t)(row0 + r) * ld_out + c;
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
    __syncthreads();
  }

  if (live && s.pos > s.nwords) st = 1;
  if (img < B && status) status[img] = st;
  // an overrun is known only now, after other lanes have written the row: vote, fence, zero (rans_decode_gather_kernel)
  if (live && st == 1) *vote = 1;
  __syncthreads();
  if (*vote) {
    __threadfence();
    __syncthreads();
    if (live && st == 1) {
      OutT *dst = out + (size_t)img * ld_out;
      for (int c = 0; c < C; ++c) store_out(dst + c, 0.f);
    }
  }
}

// ---------------------------------------------------------------------------
// compaction: lengths -> exclusive offsets (wave scans) -> wave-per-image copy
// ---------------------------------------------------------------------------
constexpr int kScanThreads = 1024;

// Inclusive scan across the workgroup (Hillis-Steele through LDS memory, double-buffered); returns this
// thread's inclusive value and the workgroup total.  buf must hold 2 * blockDim.x entries of LDS.  At 16 Ki
// lengths per launch the scan's latency does not matter; ten barrier-separated steps are the simplest
// thing that is obviously right.
__device__ __forceinline__ uint64_t block_inclusive_scan(uint64_t v, uint64_t *buf, uint64_t *total) {
  const int t = threadIdx.x, n = blockDim.x;
  int cur = 0;
  buf[t] = v;
  __syncthreads();
  for (int d = 1; d < n; d <<= 1) {
    uint64_t x = buf[cur * n + t];
    if (t >= d) x += buf[cur * n + t - d];
    cur ^= 1;
    buf[cur * n + t] = x;
    __syncthreads();
  }
  *total = buf[cur * n + n - 1];
  return buf[cur * n + t];
}

__global__ __launch_bounds__(kScanThreads) void block_sums_kernel(
    const uint32_t *__restrict__ lengths, int B, uint32_t extra, uint64_t *__restrict__ sums) {
  __shared__ uint64_t wave_tot[2 * kScanThreads];
  const int i = blockIdx.x * kScanThreads + threadIdx.x;
  const uint64_t v = i < B ? (uint64_t)lengths[i] + extra : 0;
  uint64_t total;
  block_inclusive_scan(v, wave_tot, &total);
  if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// single workgroup: exclusive scan of sums[0..n) in place, total -> *grand
__global__ __launch_bounds__(kScanThreads) void scan_sums_kernel(uint64_t *__restrict__ sums,
                                                                 int n,
                                                                 uint64_t *__restrict__ grand) {
  __shared__ uint64_t wave_tot[2 * kScanThreads];
  uint64_t carry = 0;
  for (int base = 0; base < n; base += kScanThreads) {
    const int i = base + threadIdx.x;
    const uint64_t v = i < n ? sums[i] : 0;
    uint64_t total;
    const uint64_t inc = block_inclusive_scan(v, wave_tot, &total);
    if (i < n) sums[i] = carry + inc - v;
    carry += total;
    __syncthreads();
  }
  if (threadIdx.x == 0) *grand = carry;
}

__global__ __launch_bounds__(kScanThreads) void final_offsets_kernel(
    const uint32_t *__restrict__ lengths, int B, uint32_t extra,
    const uint64_t *__restrict__ sums_ex, uint64_t *__restrict__ out_off) {
  __shared__ uint64_t wave_tot[2 * kScanThreads];
  const int i = blockIdx.x * kScanThreads + threadIdx.x;
  const uint64_t v = i < B ? (uint64_t)lengths[i] + extra : 0;
  uint64_t total;
  const uint64_t inc = block_inclusive_scan(v, wave_tot, &total);
  if (i < B) out_off[i] = sums_ex[blockIdx.x] + inc - v;
}

// one wave copies one stream (4-byte words) to out + o, behind its big-endian length if record_prefix
__device__ __forceinline__ void copy_record(const uint8_t *__restrict__ stream_end, uint32_t len, int record_prefix,
                                            uint8_t *__restrict__ out, size_t cap, uint64_t o, int lane) {
  const uint64_t need = o + len + (record_prefix ? 4u : 0u);
  if (need > cap) return;  // caller learns the required size from the last offset
  const uint32_t *src = reinterpret_cast<const uint32_t *>(stream_end - len);
  uint32_t *dst = reinterpret_cast<uint32_t *>(out + o);
  if (record_prefix) {
    if (lane == 0) dst[0] = __builtin_bswap32(len);  // big-endian u32, hub/compressor.py:258
    ++dst;
  }
  const uint32_t nw = len >> 2;
  for (uint32_t w = lane; w < nw; w += kWave) dst[w] = src[w];
}

__global__ __launch_bounds__(256) void copy_streams_kernel(
    const uint8_t *__restrict__ scratch, size_t stride, const uint32_t *__restrict__ lengths,
    int B, int record_prefix, uint8_t *__restrict__ out, size_t cap,
    const uint64_t *__restrict__ out_off) {
  const int img = blockIdx.x * 4 + (threadIdx.x / kWave);
  const int lane = threadIdx.x & (kWave - 1);
  if (img >= B) return;
  copy_record(scratch + (size_t)img * stride + stride, lengths[img], record_prefix, out, cap, out_off[img], lane);
}

// (z, side) pairs: record 2i is image i's stream of scratch_a, record 2i+1 its stream of scratch_b
__global__ __launch_bounds__(256) void interleave_lengths_kernel(const uint32_t *__restrict__ a,
                                                                 const uint32_t *__restrict__ b, int B,
                                                                 uint32_t *__restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= B) return;
  out[2 * i] = a[i];
  out[2 * i + 1] = b[i];
}

__global__ __launch_bounds__(256) void copy_pairs_kernel(
    const uint8_t *__restrict__ scratch_a, size_t stride_a, const uint8_t *__restrict__ scratch_b,
    size_t stride_b, const uint32_t *__restrict__ lengths2, int B, uint8_t *__restrict__ out, size_t cap,
    const uint64_t *__restrict__ out_off) {
  const int rec = blockIdx.x * 4 + (threadIdx.x / kWave);
  const int lane = threadIdx.x & (kWave - 1);
  if (rec >= 2 * B) return;
  const int img = rec >> 1;
  const uint8_t *end = (rec & 1) ? scratch_b + (size_t)img * stride_b + stride_b
                                 : scratch_a + (size_t)img * stride_a + stride_a;
  copy_record(end, lengths2[rec], 1, out, cap, out_off[rec], lane);
}

inline int grid_for(size_t n, int threads, int cap = 2048) {
  size_t g = (n + threads - 1) / threads;
  if (g > (size_t)cap) g = cap;
  if (g < 1) g = 1;
  return (int)g;
}

// LDS for a decoder that packs the T rows (stage_packed_rows) behind `front` bytes of its own: the rows' valid entries number
// at most T*W (known exactly only on the device), so the launch asks for min(device limit, front + header + 2*T*W) -- small
// tables leave room for several workgroups per CU.  The limit and the kernel's opt-in to > 48 KiB are per DEVICE (a process
// may drive several GPUs).  Returns `front` alone when not even the header fits (absurdly many rows: global-memory search).
unsigned packed_rows_lds(const void *kernel, size_t front, int T, int W) {
  const unsigned lds_max = dynamic_lds_limit(kernel);
  const size_t head = front + packed_rows_head(T);
  const size_t want = head + 2 * (size_t)T * (size_t)W + 64;
  return head + 64 > lds_max ? (unsigned)front
                             : (unsigned)(want < lds_max ? ((want + 255) & ~(size_t)255) : lds_max);
}

bool table_args_ok(int B, int C, int W, const void *cdf, const void *cdf_len, const void *off) {
  return B >= 0 && C > 0 && W >= 3 && (size_t)C * W * 2 <= 64 * 1024 && cdf && cdf_len && off;
}

}  // namespace
}  // namespace lla

using namespace lla;

extern "C" {

int lla_abi_version(void) { return LLA_ABI_VERSION; }
int lla_last_hip_error(void) { return g_last_hip_error; }

size_t lla_rans_max_encoded_bytes(int C) {
  // per symbol at most 16 bits for the escape symbol + 1 count digit + 8 payload
  // digits = 52 bits; +2 flush words; +1 word of slack; rounded up to 16 bytes
  const size_t bits = (size_t)C * 52u;
  const size_t bytes = 4u * ((bits + 31u) / 32u) + 8u + 4u;
  return (bytes + 15u) & ~(size_t)15u;
}

int lla_quantise(const void *z, int z_dtype, int B, int C, const float *bias,
                 const float *exp_scale, const float *median, int32_t *symbols, void *stream) {
  if (!z || !bias || !exp_scale || !median || !symbols || B < 0 || C <= 0) return LLA_EINVAL;
  if (z_dtype != LLA_Z_F16 && z_dtype != LLA_Z_F32) return LLA_EINVAL;
  const size_t n = (size_t)B * C;
  if (n == 0) return LLA_OK;
  const int g = grid_for(n, 256);
  if (z_dtype == LLA_Z_F16)
    quantise_kernel<1><<<g, 256, 0, as_stream(stream)>>>(z, n, C, bias, exp_scale, median, symbols);
  else
    quantise_kernel<2><<<g, 256, 0, as_stream(stream)>>>(z, n, C, bias, exp_scale, median, symbols);
  return check_launch();
}

int lla_rans_encode_batch(const int32_t *symbols, int B, int C, const int32_t *cdf, int W,
                          const int32_t *cdf_len, const int32_t *offset, uint8_t *scratch,
                          size_t stride, uint32_t *lengths, void *stream) {
  if (B == 0) return LLA_OK;
  if (!symbols || !scratch || !lengths || !table_args_ok(B, C, W, cdf, cdf_len, offset))
    return LLA_EINVAL;
  if (stride < lla_rans_max_encoded_bytes(C) || (stride & 3u)) return LLA_ECAP;
  const int grid = (B + kEncThreads - 1) / kEncThreads;
  const size_t lds = enc_lds_bytes(C, W);
  if (lds > 64 * 1024) return LLA_EINVAL;
  rans_encode_kernel<0><<<grid, kEncThreads, lds, as_stream(stream)>>>(
      symbols, B, C, nullptr, nullptr, nullptr, cdf, W, cdf_len, offset, scratch, stride, lengths,
      nullptr);
  return check_launch();
}

int lla_quantise_encode(const void *z, int z_dtype, int B, int C, const float *bias,
                        const float *exp_scale, const float *median, const int32_t *cdf, int W,
                        const int32_t *cdf_len, const int32_t *offset, uint8_t *scratch,
                        size_t stride, uint32_t *lengths, int32_t *symbols_out, void *stream) {
  if (B == 0) return LLA_OK;
  if (!z || !bias || !exp_scale || !median || !scratch || !lengths ||
      !table_args_ok(B, C, W, cdf, cdf_len, offset))
    return LLA_EINVAL;
  if (z_dtype != LLA_Z_F16 && z_dtype != LLA_Z_F32) return LLA_EINVAL;
  if (stride < lla_rans_max_encoded_bytes(C) || (stride & 3u)) return LLA_ECAP;
  const int grid = (B + kEncThreads - 1) / kEncThreads;
  const size_t lds = enc_lds_bytes(C, W);
  if (lds > 64 * 1024) return LLA_EINVAL;
  if (z_dtype == LLA_Z_F16)
    rans_encode_kernel<1><<<grid, kEncThreads, lds, as_stream(stream)>>>(
        z, B, C, bias, exp_scale, median, cdf, W, cdf_len, offset, scratch, stride, lengths,
        symbols_out);
  else
    rans_encode_kernel<2><<<grid, kEncThreads, lds, as_stream(stream)>>>(
        z, B, C, bias, exp_scale, median, cdf, W, cdf_len, offset, scratch, stride, lengths,
        symbols_out);
  return check_launch();
}

size_t lla_rans_compact_workspace_bytes(int B) {
  const size_t nblk = ((size_t)(B > 0 ? B : 1) + kScanThreads - 1) / kScanThreads;
  return (nblk + 1) * sizeof(uint64_t);
}

int lla_rans_compact(const uint8_t *scratch, size_t stride, const uint32_t *lengths, int B,
                     int record_prefix, uint8_t *out, size_t cap, uint64_t *out_off,
                     void *workspace, size_t workspace_bytes, void *stream) {
  hipStream_t st = as_stream(stream);
  if (B == 0) {
    if (!out_off) return LLA_EINVAL;
    hipError_t e = hipMemsetAsync(out_off, 0, sizeof(uint64_t), st);
    return e == hipSuccess ? LLA_OK : hip_fail(e);
  }
  if (!scratch || !lengths || !out || !out_off || !workspace || B < 0) return LLA_EINVAL;
  if (workspace_bytes < lla_rans_compact_workspace_bytes(B)) return LLA_ECAP;
  if ((reinterpret_cast<uintptr_t>(out) & 3u) || (stride & 3u)) return LLA_EINVAL;
  uint64_t *sums = reinterpret_cast<uint64_t *>(workspace);
  const int nblk = (B + kScanThreads - 1) / kScanThreads;
  const uint32_t extra = record_prefix ? 4u : 0u;
  block_sums_kernel<<<nblk, kScanThreads, 0, st>>>(lengths, B, extra, sums);
  scan_sums_kernel<<<1, kScanThreads, 0, st>>>(sums, nblk, out_off + B);
  final_offsets_kernel<<<nblk, kScanThreads, 0, st>>>(lengths, B, extra, sums, out_off);
  copy_streams_kernel<<<(B + 3) / 4, 256, 0, st>>>(scratch, stride, lengths, B, record_prefix, out,
                                                   cap, out_off);
  return check_launch();
}

size_t lla_rans_compact_pairs_workspace_bytes(int B) {
  const size_t b2 = 2 * (size_t)(B > 0 ? B : 1);     // (2B records; B is below 2^30 where this is used, so b2 fits an int)
  const size_t nblk = (b2 + kScanThreads - 1) / kScanThreads;
  return ((b2 * sizeof(uint32_t) + 7) & ~(size_t)7) + (nblk + 1) * sizeof(uint64_t);
}

int lla_rans_compact_pairs(const uint8_t *scratch_a, size_t stride_a, const uint32_t *lengths_a,
                           const uint8_t *scratch_b, size_t stride_b, const uint32_t *lengths_b, int B,
                           uint8_t *out, size_t cap, uint64_t *out_off, void *workspace,
                           size_t workspace_bytes, void *stream) {
  hipStream_t st = as_stream(stream);
  if (B == 0) {
    if (!out_off) return LLA_EINVAL;
    hipError_t e = hipMemsetAsync(out_off, 0, sizeof(uint64_t), st);
    return e == hipSuccess ? LLA_OK : hip_fail(e);
  }
  if (!scratch_a || !lengths_a || !scratch_b || !lengths_b || !out || !out_off || !workspace || B < 0 ||
      B >= (1 << 30))     // (2B records are counted in an int)
    return LLA_EINVAL;
  if (workspace_bytes < lla_rans_compact_pairs_workspace_bytes(B)) return LLA_ECAP;
  if ((reinterpret_cast<uintptr_t>(out) & 3u) || (stride_a & 3u) || (stride_b & 3u) ||
      (reinterpret_cast<uintptr_t>(workspace) & 7u))
    return LLA_EINVAL;
  // the two length arrays interleaved are the lengths of 2B records: the scans of lla_rans_compact do the rest
  const int B2 = 2 * B;
  uint32_t *lengths2 = reinterpret_cast<uint32_t *>(workspace);
  uint64_t *sums = reinterpret_cast<uint64_t *>(reinterpret_cast<uint8_t *>(workspace) +
                                                (((size_t)B2 * sizeof(uint32_t) + 7) & ~(size_t)7));
  const int nblk = (B2 + kScanThreads - 1) / kScanThreads;
  interleave_lengths_kernel<<<(B + 255) / 256, 256, 0, st>>>(lengths_a, lengths_b, B, lengths2);
  block_sums_kernel<<<nblk, kScanThreads, 0, st>>>(lengths2, B2, 4u, sums);
  scan_sums_kernel<<<1, kScanThreads, 0, st>>>(sums, nblk, out_off + B2);
  final_offsets_kernel<<<nblk, kScanThreads, 0, st>>>(lengths2, B2, 4u, sums, out_off);
  copy_pairs_kernel<<<(B2 + 3) / 4, 256, 0, st>>>(scratch_a, stride_a, scratch_b, stride_b, lengths2, B, out, cap,
                                                  out_off);
  return check_launch();
}

int lla_rans_decode_batch_strided(const uint8_t *payload, const uint64_t *off, int record_prefix,
                                  int off_first, int off_step, int B, int C, const int32_t *cdf, int W,
                                  const int32_t *cdf_len, const int32_t *offset, int32_t *symbols_out,
                                  int32_t *status, void *stream) {
  if (B == 0) return LLA_OK;
  if (!payload || !off || !symbols_out || off_first < 0 || off_step < 1 ||
      !table_args_ok(B, C, W, cdf, cdf_len, offset))
    return LLA_EINVAL;
  const int grid = (B + kEncThreads - 1) / kEncThreads;
  const size_t lds = enc_table_bytes(C, W) + (size_t)C * sizeof(int2);
  if (lds > 64 * 1024) return LLA_EINVAL;
  int skip = record_prefix ? 4 : 0;
  rans_decode_kernel<<<grid, kEncThreads, lds, as_stream(stream)>>>(
      payload, off + off_first, skip, off_step, B, C, cdf, W, cdf_len, offset, symbols_out, status);
  return check_launch();
}

int lla_rans_decode_batch(const uint8_t *payload, const uint64_t *off, int record_prefix, int B,
                          int C, const int32_t *cdf, int W, const int32_t *cdf_len,
                          const int32_t *offset, int32_t *symbols_out, int32_t *status,
                          void *stream) {
  return lla_rans_decode_batch_strided(payload, off, record_prefix, 0, 1, B, C, cdf, W, cdf_len, offset,
                                       symbols_out, status, stream);
}

int lla_rans_decode_gather_strided(const uint8_t *payload, const uint64_t *off, int record_prefix, int off_first,
                                   int off_step, int N, const int64_t *index, int B, int C, const int32_t *cdf,
                                   int W, const int32_t *cdf_len, const int32_t *offset, const float *bias,
                                   const float *exp_scale, const float *median, void *z_hat, int z_dtype,
                                   size_t ld_out, int32_t *status, void *stream) {
  if (z_dtype != LLA_Z_F16 && z_dtype != LLA_Z_F32) return LLA_EINVAL;
  if (off_first < 0 || off_step < 1) return LLA_EINVAL;
  if (B == 0) return LLA_OK;
  if (!payload || !off || !index || !bias || !exp_scale || !median || !z_hat || !status || N < 0 ||
      !table_args_ok(B, C, W, cdf, cdf_len, offset) || ld_out < (size_t)C)
    return LLA_EINVAL;
  const int grid = (B + kEncThreads - 1) / kEncThreads;
  const size_t lds = gather_lds_bytes(C, W);
  if (lds > 64 * 1024) return LLA_EINVAL;
  const int skip = record_prefix ? 4 : 0;
  if (z_dtype == LLA_Z_F16)
    rans_decode_gather_kernel<__half><<<grid, kEncThreads, lds, as_stream(stream)>>>(
        payload, off, skip, off_first, off_step, N, index, B, C, cdf, W, cdf_len, offset, bias, exp_scale, median,
        reinterpret_cast<__half *>(z_hat), ld_out, status);
  else
    rans_decode_gather_kernel<float><<<grid, kEncThreads, lds, as_stream(stream)>>>(
        payload, off, skip, off_first, off_step, N, index, B, C, cdf, W, cdf_len, offset, bias, exp_scale, median,
        reinterpret_cast<float *>(z_hat), ld_out, status);
  return check_launch();
}

int lla_rans_decode_gather(const uint8_t *payload, const uint64_t *off, int record_prefix, int N,
                           const int64_t *index, int B, int C, const int32_t *cdf, int W,
                           const int32_t *cdf_len, const int32_t *offset, const float *bias,
                           const float *exp_scale, const float *median, void *z_hat, int z_dtype,
                           size_t ld_out, int32_t *status, void *stream) {
  return lla_rans_decode_gather_strided(payload, off, record_prefix, 0, 1, N, index, B, C, cdf, W, cdf_len, offset,
                                        bias, exp_scale, median, z_hat, z_dtype, ld_out, status, stream);
}

int lla_rans_encode_indexed(const int32_t *symbols, const int32_t *indexes, int B, int n,
                            const int32_t *cdf, int T, int W, const int32_t *cdf_len,
                            const int32_t *offset, uint8_t *scratch, size_t stride,
                            uint32_t *lengths, void *stream) {
  if (B == 0) return LLA_OK;
  if (B < 0 || n <= 0 || T <= 0 || W < 3 || !symbols || !indexes || !cdf || !cdf_len || !offset ||
      !scratch || !lengths)
    return LLA_EINVAL;
  if (stride < lla_rans_max_encoded_bytes(n) || (stride & 3u)) return LLA_ECAP;
  const int grid = (B + kEncThreads - 1) / kEncThreads;
  rans_encode_indexed_kernel<<<grid, kEncThreads, 0, as_stream(stream)>>>(
      symbols, indexes, B, n, cdf, T, W, cdf_len, offset, scratch, stride, lengths);
  return check_launch();
}

int lla_rans_decode_indexed(const uint8_t *payload, const uint64_t *off, int record_prefix, int B,
                            int n, const int32_t *indexes, const int32_t *cdf, int T, int W,
                            const int32_t *cdf_len, const int32_t *offset, int32_t *symbols_out,
                            int32_t *status, void *stream) {
  if (B == 0) return LLA_OK;
  if (B < 0 || n <= 0 || T <= 0 || W < 3 || !payload || !off || !indexes || !cdf || !cdf_len ||
      !offset || !symbols_out)
    return LLA_EINVAL;
  const int grid = (B + kEncThreads - 1) / kEncThreads;
  const unsigned lds = packed_rows_lds(reinterpret_cast<const void *>(rans_decode_indexed_kernel), 0, T, W);
  rans_decode_indexed_kernel<<<grid, kEncThreads, lds, as_stream(stream)>>>(
      payload, off, record_prefix ? 4 : 0, B, n, indexes, cdf, T, W, cdf_len, offset, symbols_out,
      status, lds);
  return check_launch();
}

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
  const MeanRows mr{means, ld_means};
  if (with_means && z_dtype == LLA_Z_F16)
    gaussian_encode_kernel<1><<<grid, kEncThreads, lds, as_stream(stream)>>>(
        z, B, C, bias, exp_scale, scales, ld_scales, scale_table, scale_bound, cdf, T, W, cdf_len, offset, scratch,
        stride, lengths, symbols_out, indexes_out, mr);
  else if (with_means)
    gaussian_encode_kernel<2><<<grid, kEncThreads, lds, as_stream(stream)>>>(
        z, B, C, bias, exp_scale, scales, ld_scales, scale_table, scale_bound, cdf, T, W, cdf_len, offset, scratch,
        stride, lengths, symbols_out, indexes_out, mr);
  else if (z_dtype == LLA_Z_F16)
    gaussian_encode_kernel<1><<<grid, kEncThreads, lds, as_stream(stream)>>>(
        z, B, C, bias, exp_scale, scales, ld_scales, scale_table, scale_bound, cdf, T, W, cdf_len, offset, scratch,
        stride, lengths, symbols_out, indexes_out);
  else
    gaussian_encode_kernel<2><<<grid, kEncThreads, lds, as_stream(stream)>>>(
        z, B, C, bias, exp_scale, scales, ld_scales, scale_table, scale_bound, cdf, T, W, cdf_len, offset, scratch,
        stride, lengths, symbols_out, indexes_out);
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
  if (with_means) {
    const unsigned lds = packed_rows_lds(reinterpret_cast<const void *>(gaussian_decode_kernel<MeanRows>), front, T, W);
    gaussian_decode_kernel<<<grid, kEncThreads, lds, as_stream(stream)>>>(
        payload, off + off_first, record_prefix ? 4 : 0, off_step, B, C, bias, exp_scale, scales, ld_scales,
        scale_table, scale_bound, cdf, T, W, cdf_len, offset, z_hat, status, lds, MeanRows{means, ld_means});
  } else {
    const unsigned lds = packed_rows_lds(reinterpret_cast<const void *>(gaussian_decode_kernel<>), front, T, W);
    gaussian_decode_kernel<<<grid, kEncThreads, lds, as_stream(stream)>>>(
        payload, off + off_first, record_prefix ? 4 : 0, off_step, B, C, bias, exp_scale, scales, ld_scales,
        scale_table, scale_bound, cdf, T, W, cdf_len, offset, z_hat, status, lds);
  }
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
  const void *kernel =
      with_means ? (z_dtype == LLA_Z_F16 ? reinterpret_cast<const void *>(gaussian_decode_gather_kernel<__half, MeanRows>)
                                         : reinterpret_cast<const void *>(gaussian_decode_gather_kernel<float, MeanRows>))
                 : (z_dtype == LLA_Z_F16 ? reinterpret_cast<const void *>(gaussian_decode_gather_kernel<__half>)
                                         : reinterpret_cast<const void *>(gaussian_decode_gather_kernel<float>));
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
  const MeanRows mr{means, ld_means};
  if (with_means && z_dtype == LLA_Z_F16)
    gaussian_decode_gather_kernel<__half><<<grid, kEncThreads, lds, as_stream(stream)>>>(
        payload, off, skip, off_first, off_step, N, index, B, C, bias, exp_scale, scales, ld_scales, scale_table,
        scale_bound, cdf, T, W, cdf_len, offset, reinterpret_cast<__half *>(z_hat), ld_out, status_in, status, lds, mr);
  else if (with_means)
    gaussian_decode_gather_kernel<float><<<grid, kEncThreads, lds, as_stream(stream)>>>(
        payload, off, skip, off_first, off_step, N, index, B, C, bias, exp_scale, scales, ld_scales, scale_table,
        scale_bound, cdf, T, W, cdf_len, offset, reinterpret_cast<float *>(z_hat), ld_out, status_in, status, lds, mr);
  else if (z_dtype == LLA_Z_F16)
    gaussian_decode_gather_kernel<__half><<<grid, kEncThreads, lds, as_stream(stream)>>>(
        payload, off, skip, off_first, off_step, N, index, B, C, bias, exp_scale, scales, ld_scales, scale_table,
        scale_bound, cdf, T, W, cdf_len, offset, reinterpret_cast<__half *>(z_hat), ld_out, status_in, status, lds);
  else
    gaussian_decode_gather_kernel<float><<<grid, kEncThreads, lds, as_stream(stream)>>>(
        payload, off, skip, off_first, off_step, N, index, B, C, bias, exp_scale, scales, ld_scales, scale_table,
        scale_bound, cdf, T, W, cdf_len, offset, reinterpret_cast<float *>(z_hat), ld_out, status_in, status, lds);
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

int lla_dequantise(const int32_t *symbols, int B, int C, const float *bias,
                   const float *exp_scale, const float *median, float *z_hat, void *stream) {
  if (!symbols || !bias || !exp_scale || !median || !z_hat || B < 0 || C <= 0) return LLA_EINVAL;
  const size_t n = (size_t)B * C;
  if (n == 0) return LLA_OK;
  dequantise_kernel<<<grid_for(n, 256), 256, 0, as_stream(stream)>>>(symbols, n, C, bias, exp_scale,
                                                                     median, z_hat);
  return check_launch();
}

int lla_represent(const void *z, int z_dtype, int B, int C, const float *bias,
                  const float *exp_scale, const float *median, float *z_hat, void *stream) {
  if (!z || !bias || !exp_scale || !median || !z_hat || B < 0 || C <= 0) return LLA_EINVAL;
  if (z_dtype != LLA_Z_F16 && z_dtype != LLA_Z_F32) return LLA_EINVAL;
  const size_t n = (size_t)B * C;
  if (n == 0) return LLA_OK;
  const int g = grid_for(n, 256);
  if (z_dtype == LLA_Z_F16)
    represent_kernel<1><<<g, 256, 0, as_stream(stream)>>>(z, n, C, bias, exp_scale, median, z_hat);
  else
    represent_kernel<2><<<g, 256, 0, as_stream(stream)>>>(z, n, C, bias, exp_scale, median, z_hat);
  return check_launch();
}

}  // extern "C"
