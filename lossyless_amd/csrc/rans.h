// The rANS coder's device primitives, one copy each, for entropy.hip (factorized and indexed coders) and
// entropy_gaussian.hip (scale-hyperprior coder): table staging, the encoder's state update and its walk over a string,
// the decoder's state, row search and symbol read, the rows packed into LDS, and the launchers' small host helpers.
// Every container the project writes is promised byte-equal to compressai's and every random-access read bit-equal to a
// full decode: the coders share THESE functions, and the byte stream depends on the order stated at encode_walk (which
// rans_encode_kernel keeps written out, for the reason given there).
#pragma once
#include "common.h"

#include <hip/hip_fp16.h>

#include <cstdlib>
#include <type_traits>

namespace lla {
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

__device__ __forceinline__ float as_float(__half v) { return __half2float(v); }   // z as read: Fetch<1 / 2>::elem
__device__ __forceinline__ float as_float(float v) { return v; }

__device__ __forceinline__ float dequantise_one(float q, float bias, float es, float med) {
  const float zh = __fadd_rn(q, med);
  return __fsub_rn(__fdiv_rn(zh, es), bias);
}

// ZMODE 0: int32 symbols, 1: fp16 z, 2: fp32 z.  G = channels fetched per 16-byte load.
template <int ZMODE>
struct Fetch {
  static constexpr int mode = ZMODE;
  using elem = std::conditional_t<ZMODE == 0, int32_t, std::conditional_t<ZMODE == 1, __half, float>>;
  static constexpr int G = 16 / sizeof(elem);
};

// N elements of a row into registers: in 16-byte loads where `vec` says the row is aligned for them, else one by one
template <int N, typename T>
__device__ __forceinline__ void load_group(T (&d)[N], const T *src, bool vec) {
  if (vec) {
#pragma unroll
    for (int k = 0; k < N; k += 16 / sizeof(T)) *reinterpret_cast<uint4 *>(d + k) = *reinterpret_cast<const uint4 *>(src + k);
  } else {
#pragma unroll
    for (int k = 0; k < N; ++k) d[k] = src[k];
  }
}

// A length read from cdf_len, as every coder uses it for a row it was not given per channel: at least the three entries
// of a one-symbol row, at most the row's pitch.
__device__ __forceinline__ int row_len(int len, int W) { return min(max(len, 3), W); }

// String `i` of a launch is written backwards from the end of its `stride` bytes of scratch; returns that end.
__device__ __forceinline__ uint8_t *open_encoder(EncState &s, uint8_t *scratch, size_t stride, int i) {
  uint8_t *end = scratch + (size_t)i * stride + stride;
  s.x = kStateLow;
  s.wp = reinterpret_cast<uint32_t *>(end);
  return end;
}

// ... and closed with the two words of the state in front; lengths[i] = bytes from there to `end`.
__device__ __forceinline__ void close_encoder(EncState &s, const uint8_t *end, uint32_t *lengths, int i) {
  s.wp -= 2;
  s.wp[0] = (uint32_t)s.x;
  s.wp[1] = (uint32_t)(s.x >> 32);
  lengths[i] = (uint32_t)(end - reinterpret_cast<uint8_t *>(s.wp));
}

// The walk of an encoder over the n symbols of a string, last symbol first (the decoder reads them first to last):
// the n % G tail symbols one by one, then the groups of G from the last to the first; within a group `prep` runs for
// all G symbols in ASCENDING order (table look-ups, off the state's dependency chain) before they are emitted in
// DESCENDING order.  The byte stream depends on exactly this order.
//   load(c0, std::integral_constant<int, N>)  fetches what symbols [c0, c0 + N) need: N = 1 in the tail, N = G in a group
//   prep(c, k) -> Prepared                    symbol c, the k-th of what the last load fetched
template <int G, typename Load, typename Prep>
__device__ __forceinline__ void encode_walk(EncState &s, int n, Load &&load, Prep &&prep) {
  const int tail = n % G;
  for (int c = n - 1; c >= n - tail; --c) {
    load(c, std::integral_constant<int, 1>{});
    emit_channel(s, prep(c, 0));
  }
  for (int g = (n - tail) / G - 1; g >= 0; --g) {
    load(g * G, std::integral_constant<int, G>{});
    Prepared pr[G];
#pragma unroll
    for (int k = 0; k < G; ++k) pr[k] = prep(g * G + k, k);
#pragma unroll
    for (int k = G - 1; k >= 0; --k) emit_channel(s, pr[k]);
  }
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
    for (int t = threadIdx.x; t < T; t += blockDim.x) r.par[t] = make_int2(row_len(cdf_len[t], W), offset[t]);
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

// One symbol of row t off the stream, offset added: from the packed rows where they fit the LDS, else from the int32 table
// in global memory (the same search, the same clamp of the row's length).
__device__ __forceinline__ int32_t decode_row(DecState &s, const PackedRows &rows, int t, const int32_t *__restrict__ cdf,
                                              int W, const int32_t *__restrict__ cdf_len,
                                              const int32_t *__restrict__ offset) {
  if (rows.in_lds) {
    const int2 q = rows.par[t];
    return decode_symbol<true>(s, rows.tab + rows.rowoff[t], q.x) + q.y;
  }
  return decode_symbol<true>(s, cdf + (size_t)t * W, row_len(cdf_len[t], W)) + offset[t];
}

__device__ __forceinline__ void store_out(float *p, float v) { *p = v; }
__device__ __forceinline__ void store_out(__half *p, float v) { *p = __float2half_rn(v); }
__device__ __forceinline__ void store_out4(float *p, const float4 &v) { *reinterpret_cast<float4 *>(p) = v; }
__device__ __forceinline__ void store_out4(__half *p, const float4 &v) {
  const __half2 a = __floats2half2_rn(v.x, v.y), b = __floats2half2_rn(v.z, v.w);
  *reinterpret_cast<uint2 *>(p) = uint2{__builtin_bit_cast(uint32_t, a), __builtin_bit_cast(uint32_t, b)};
}

// ---------------------------------------------------------------------------
// host side: what the launchers of both files share
// ---------------------------------------------------------------------------
// z_dtype (checked by the caller: LLA_Z_F16 or LLA_Z_F32) as a compile-time tag, f(Fetch<1>{}) or f(Fetch<2>{}), so that an
// entry point holds ONE launch expression
template <typename F>
inline void with_z(int z_dtype, F &&f) {
  if (z_dtype == LLA_Z_F16) f(Fetch<1>{});
  else f(Fetch<2>{});
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
inline unsigned packed_rows_lds(const void *kernel, size_t front, int T, int W) {
  const unsigned lds_max = dynamic_lds_limit(kernel);
  const size_t head = front + packed_rows_head(T);
  const size_t want = head + 2 * (size_t)T * (size_t)W + 64;
  return head + 64 > lds_max ? (unsigned)front
                             : (unsigned)(want < lds_max ? ((want + 255) & ~(size_t)255) : lds_max);
}

inline bool table_args_ok(int B, int C, int W, const void *cdf, const void *cdf_len, const void *off) {
  return B >= 0 && C > 0 && W >= 3 && (size_t)C * W * 2 <= 64 * 1024 && cdf && cdf_len && off;
}

}  // namespace
}  // namespace lla
