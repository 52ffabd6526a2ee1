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
// The coder's primitives are rans.h's and the gathered decoder's staging gather_stage.h's, shared with the
// scale-hyperprior coder (entropy_gaussian.hip).
#include "gather_stage.h"

namespace lla {

thread_local int g_last_hip_error = 0;

namespace {

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

  EncState s;
  uint8_t *end = open_encoder(s, scratch, stride, img);

  auto prep = [&](int c, elem raw_in) {
    const ChanParams q = par[c];
    int32_t sym;
    if constexpr (ZMODE == 0) sym = raw_in;
    else sym = quantise_one(as_float(raw_in), q.bias, q.es, q.med);
    if (symbols_out) symbols_out[(size_t)img * C + c] = sym;
    return prepare_channel(tab + c * W, q.len, q.off, sym);
  };

  // rans.h's encode_walk, written out: tail, groups descending, prep ascending, emit descending.  Through the shared
  // function the instructions are the same but for the operand order of divmod16's multiplies and the place of one
  // address update per symbol, and the fp16 encoder measured 1.2 % slower (6.93 against 7.01 M img/s at batch 1024).
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
  close_encoder(s, end, lengths, img);
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
// lane as above; the symbols never leave the registers.  The values reach global memory through gather_stage.h's
// LDS staging: every lane parks kGatherG channels of its row, then the workgroup writes whole lines.
// LDS at C = 512, W = 33: table 33 792 + parameters 512 x 20 = 10 240 + vote 16 + staging 16 384 = 60 432 bytes.
// ---------------------------------------------------------------------------
struct __attribute__((aligned(16))) GatherParams {
  float bias, es, med;
  int32_t off;
};
__host__ __device__ inline size_t gather_lds_bytes(int C, int W) {
  return enc_table_bytes(C, W) + (size_t)C * sizeof(GatherParams) + (((size_t)C * sizeof(int32_t) + 15u) & ~(size_t)15u) +
         kVoteBytes + kGatherStageBytes;
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
  float4 *stage = reinterpret_cast<float4 *>(smem + gather_lds_bytes(C, W) - kGatherStageBytes);
  int *vote = reinterpret_cast<int *>(smem + gather_lds_bytes(C, W) - kGatherStageBytes - kVoteBytes);
  for (int c = threadIdx.x; c < C; c += blockDim.x) {
    par[c] = GatherParams{bias[c], exp_scale[c], median[c], offset[c]};
    len[c] = cdf_len[c];
  }
  if (threadIdx.x == 0) *vote = 0;
  stage_table(tab, cdf, C * W);

  // a lane without a record (past B, index out of range, stream unopenable) decodes nothing and parks zeros
  const GatherLanes g = gather_lanes(B);
  const int lane = g.lane, img = g.img;
  int st;
  DecState s;
  const bool live = pick_record(s, st, img, B, index, N, payload, off, skip, off_first, off_step);
  const bool vec_ok = out_vec_ok(out, ld_out);

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
      park_own(stage, lane, j, float4{v[4 * j], v[4 * j + 1], v[4 * j + 2], v[4 * j + 3]});
    __syncthreads();
    write_out(stage, out, ld_out, g, c0, C, vec_ok);
    __syncthreads();
  }

  if (live && s.pos > s.nwords) st = 1;
  if (img < B && status) status[img] = st;
  zero_overrun(vote, live && st == 1, out, ld_out, img, C);
}

// ---------------------------------------------------------------------------
// The three kernels above for a table of any width: the rows and the per-channel parameters pass
// through LDS in WINDOWS of `wc` channels, two buffers, instead of being resident.  All lanes of a workgroup walk the
// channel index in lock-step, so the workgroup needs one window at a time; window k holds channels [k * wc,
// min(C, (k + 1) * wc)), wc a multiple of 4: the borders lie on encode_walk<4>'s group grid counted from channel 0 and
// the C % 4 tail belongs to the last window.  The encoder walks the windows (and the channels in each) DESCENDING, the
// decoders ascending; a symbol's arithmetic is rans.h's, so the streams are the resident kernels' byte for byte,
// whatever wc is.
// One barrier per window.  In iteration w: the loads of window w' (the next one) are issued into registers
// (window_fetch: kWinQuads 16-byte loads of rows and one channel's parameters per thread), what the registers do not
// hold is written straight into the other buffer (window_rest: the rows past the first kWinRegEntries entries), window w
// is coded from its buffer, the registers are parked in the other buffer (window_park), barrier.  The other buffer is
// free all that time: its last readers passed the barrier that ended the previous iteration.
// NO lane leaves before the last barrier: one without a record (past B, bad index, unopenable stream) skips the
// coding and nothing else.
// ---------------------------------------------------------------------------
constexpr int kWinQuads = 4;                              // 16-byte loads per thread in flight across a window's coding
constexpr int kWinMaxChannels = kEncThreads;              // one thread fetches one channel's parameters
constexpr int kWinRegEntries = kWinQuads * 4 * kEncThreads;   // table entries the registers of a workgroup hold
constexpr size_t kWideLdsMax = 64 * 1024;      // what a launch may ask for
constexpr size_t kWideLdsBudget = 56 * 1024;   // what the library's own choice of window stays within

struct WindowRegs {
  int4 q[kWinQuads];
  ChanParams p;
};
struct WindowSrc {   // bias / es / med may be null (no quantiser): zeros
  const int32_t *cdf, *cdf_len, *offset;
  const float *bias, *es, *med;
  int W, C;
};
struct WindowBuf {
  uint16_t *tab;     // [n][W]
  ChanParams *par;   // [n]
};
__host__ __device__ inline size_t window_buf_bytes(int wc, int W) { return enc_table_bytes(wc, W) + (size_t)wc * sizeof(ChanParams); }
__host__ __device__ inline size_t wide_lds_bytes(int wc, int W, bool gather) {
  return 2 * window_buf_bytes(wc, W) + (gather ? kVoteBytes + kGatherStageBytes : 0);
}
__device__ __forceinline__ WindowBuf window_buf(uint8_t *smem, int b, int wc, int W) {
  uint8_t *base = smem + (size_t)b * window_buf_bytes(wc, W);
  return WindowBuf{reinterpret_cast<uint16_t *>(base), reinterpret_cast<ChanParams *>(base + enc_table_bytes(wc, W))};
}
// rows of channels [c_lo, c_lo + n) are n * W consecutive entries; c_lo * W * 4 bytes is a multiple of 16 (c_lo of 4)
__device__ __forceinline__ int window_quads(const WindowSrc &t, int n) {
  return ((reinterpret_cast<uintptr_t>(t.cdf) & 15u) == 0) ? (n * t.W) >> 2 : 0;
}
__device__ __forceinline__ void window_fetch(WindowRegs &r, const WindowSrc &t, int c_lo, int n) {
  const int4 *src = reinterpret_cast<const int4 *>(t.cdf + (size_t)c_lo * t.W);
  const int quads = window_quads(t, n);
#pragma unroll
  for (int u = 0; u < kWinQuads; ++u) {
    const int i = (int)threadIdx.x + u * kEncThreads;
    r.q[u] = i < quads ? src[i] : int4{0, 0, 0, 0};
  }
  if ((int)threadIdx.x < n) {
    const int c = c_lo + (int)threadIdx.x;
    r.p.bias = t.bias ? t.bias[c] : 0.f;
    r.p.es = t.es ? t.es[c] : 0.f;
    r.p.med = t.med ? t.med[c] : 0.f;
    r.p.off = t.offset[c];
    r.p.len = t.cdf_len[c];
  }
}
__device__ __forceinline__ void put_quad(uint16_t *tab, int i, const int4 &q) {
  typedef unsigned short u16x4 __attribute__((ext_vector_type(4)));
  *reinterpret_cast<u16x4 *>(tab + 4 * i) = u16x4{(unsigned short)q.x, (unsigned short)q.y, (unsigned short)q.z, (unsigned short)q.w};
}
__device__ __forceinline__ void window_park(const WindowRegs &r, const WindowBuf &b, const WindowSrc &t, int n) {
  const int quads = window_quads(t, n);
#pragma unroll
  for (int u = 0; u < kWinQuads; ++u) {
    const int i = (int)threadIdx.x + u * kEncThreads;
    if (i < quads) put_quad(b.tab, i, r.q[u]);
  }
  if ((int)threadIdx.x < n) b.par[threadIdx.x] = r.p;
}
__device__ __forceinline__ void window_rest(const WindowBuf &b, const WindowSrc &t, int c_lo, int n) {
  const int32_t *cdf = t.cdf + (size_t)c_lo * t.W;
  const int4 *src = reinterpret_cast<const int4 *>(cdf);
  const int quads = window_quads(t, n);
  for (int i = kWinRegEntries / 4 + (int)threadIdx.x; i < quads; i += kEncThreads) put_quad(b.tab, i, src[i]);
  for (int i = 4 * quads + (int)threadIdx.x; i < n * t.W; i += kEncThreads) b.tab[i] = (uint16_t)cdf[i];
}
// window k of a C-channel string
__device__ __forceinline__ int window_lo(int k, int wc) { return k * wc; }
__device__ __forceinline__ int window_n(int k, int wc, int C) { return min(wc, C - k * wc); }

// Calls code(buf, c_lo, n) for every window, from `first` in steps of `step` (+1 / -1), nwin of them, with the
// staging described above around it.  Every thread of the workgroup calls it.
template <typename Code>
__device__ __forceinline__ void walk_windows(uint8_t *smem, const WindowSrc &t, int wc, int first, int step, int nwin,
                                             Code &&code) {
  WindowRegs r;
  {
    const WindowBuf b0 = window_buf(smem, 0, wc, t.W);
    const int lo = window_lo(first, wc), n = window_n(first, wc, t.C);
    window_fetch(r, t, lo, n);
    window_rest(b0, t, lo, n);
    window_park(r, b0, t, n);
  }
  __syncthreads();
  for (int i = 0, k = first; i < nwin; ++i, k += step) {
    const WindowBuf cur = window_buf(smem, i & 1, wc, t.W), nxt = window_buf(smem, (i & 1) ^ 1, wc, t.W);
    const bool more = i + 1 < nwin;   // uniform
    int lo2 = 0, n2 = 0;
    if (more) {
      lo2 = window_lo(k + step, wc), n2 = window_n(k + step, wc, t.C);
      window_fetch(r, t, lo2, n2);
      window_rest(nxt, t, lo2, n2);
    }
    code(cur, window_lo(k, wc), window_n(k, wc, t.C));
    if (more) window_park(r, nxt, t, n2);
    __syncthreads();
  }
}

template <int ZMODE>
__global__ __launch_bounds__(kEncThreads) void rans_encode_wide_kernel(
    const void *__restrict__ in, int B, int C, const float *__restrict__ bias, const float *__restrict__ exp_scale,
    const float *__restrict__ median, const int32_t *__restrict__ cdf, int W, const int32_t *__restrict__ cdf_len,
    const int32_t *__restrict__ offset, uint8_t *__restrict__ scratch, size_t stride, uint32_t *__restrict__ lengths,
    int32_t *__restrict__ symbols_out, int wc) {
  kernel_acquire();
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  using elem = typename Fetch<ZMODE>::elem;
  constexpr int G = 4;   // encode_walk's group here, for every input type: the window borders' grid
  const WindowSrc t{cdf, cdf_len, offset, ZMODE ? bias : nullptr, ZMODE ? exp_scale : nullptr, ZMODE ? median : nullptr, W, C};
  const int nwin = (C + wc - 1) / wc;

  const int img = blockIdx.x * kEncThreads + threadIdx.x;
  const bool live = img < B;
  const elem *src = reinterpret_cast<const elem *>(in) + (size_t)(live ? img : 0) * C;
  const bool vec_ok = (reinterpret_cast<uintptr_t>(src) & (G * sizeof(elem) - 1)) == 0;
  EncState s;
  uint8_t *end = nullptr;
  if (live) end = open_encoder(s, scratch, stride, img);

  walk_windows(smem, t, wc, nwin - 1, -1, nwin, [&](const WindowBuf &b, int c_lo, int n) {
    if (!live) return;
    elem v[G];
    auto load = [&](int c0, auto n_c) {
      constexpr int N = decltype(n_c)::value;
      const elem *p = src + c_lo + c0;
      if constexpr (N == 1) {
        v[0] = p[0];
      } else if (vec_ok) {
        using vec = std::conditional_t<sizeof(elem) == 2, uint2, uint4>;
        *reinterpret_cast<vec *>(v) = *reinterpret_cast<const vec *>(p);
      } else {
#pragma unroll
        for (int k = 0; k < G; ++k) v[k] = p[k];
      }
    };
    auto prep = [&](int c, int k) {
      const ChanParams q = b.par[c];
      int32_t sym;
      if constexpr (ZMODE == 0) sym = v[k];
      else sym = quantise_one(as_float(v[k]), q.bias, q.es, q.med);
      if (symbols_out) symbols_out[(size_t)img * C + c_lo + c] = sym;
      return prepare_channel(b.tab + c * W, q.len, q.off, sym);
    };
    encode_walk<G>(s, n, load, prep);
  });
  if (live) close_encoder(s, end, lengths, img);
}

__global__ __launch_bounds__(kEncThreads) void rans_decode_wide_kernel(
    const uint8_t *__restrict__ payload, const uint64_t *__restrict__ off, int skip, int off_step, int B, int C,
    const int32_t *__restrict__ cdf, int W, const int32_t *__restrict__ cdf_len, const int32_t *__restrict__ offset,
    int32_t *__restrict__ out, int32_t *__restrict__ status, int wc) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const WindowSrc t{cdf, cdf_len, offset, nullptr, nullptr, nullptr, W, C};
  const int nwin = (C + wc - 1) / wc;

  const int img = blockIdx.x * kEncThreads + threadIdx.x;
  DecState s;
  int32_t *dst = out + (size_t)(img < B ? img : 0) * C;
  bool live = false;
  if (img < B) {
    live = open_stream(s, payload, off, skip, (size_t)img * (size_t)off_step);
    if (!live) {
      for (int c = 0; c < C; ++c) dst[c] = 0;
      if (status) status[img] = 1;
    }
  }
  walk_windows(smem, t, wc, 0, 1, nwin, [&](const WindowBuf &b, int c_lo, int n) {
    if (!live) return;
    for (int c = 0; c < n; ++c) {
      const ChanParams q = b.par[c];
      dst[c_lo + c] = decode_symbol<false>(s, b.tab + c * W, q.len) + q.off;
    }
  });
  if (live && status) status[img] = s.pos > s.nwords ? 1 : 0;
}

template <typename OutT>
__global__ __launch_bounds__(kEncThreads) void rans_decode_gather_wide_kernel(
    const uint8_t *__restrict__ payload, const uint64_t *__restrict__ off, int skip, int off_first, int off_step, int N,
    const int64_t *__restrict__ index, int B, int C, const int32_t *__restrict__ cdf, int W,
    const int32_t *__restrict__ cdf_len, const int32_t *__restrict__ offset, const float *__restrict__ bias,
    const float *__restrict__ exp_scale, const float *__restrict__ median, OutT *__restrict__ out, size_t ld_out,
    int32_t *__restrict__ status, int wc) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const WindowSrc t{cdf, cdf_len, offset, bias, exp_scale, median, W, C};
  const int nwin = (C + wc - 1) / wc;
  int *vote = reinterpret_cast<int *>(smem + 2 * window_buf_bytes(wc, W));
  float4 *stage = reinterpret_cast<float4 *>(smem + 2 * window_buf_bytes(wc, W) + kVoteBytes);
  if (threadIdx.x == 0) *vote = 0;   // (walk_windows' first barrier comes before any use)

  const GatherLanes g = gather_lanes(B);
  const int lane = g.lane, img = g.img;
  int st;
  DecState s;
  const bool live = pick_record(s, st, img, B, index, N, payload, off, skip, off_first, off_step);
  const bool vec_ok = out_vec_ok(out, ld_out);

  // blocks of kGatherG channels from the window's first channel (a multiple of 4: 16-byte stores stay aligned); the
  // last block of a window may be short, and write_out is told the window's end as the row's
  walk_windows(smem, t, wc, 0, 1, nwin, [&](const WindowBuf &b, int c_lo, int n) {
    for (int c0 = 0; c0 < n; c0 += kGatherG) {
      float v[kGatherG];
#pragma unroll
      for (int k = 0; k < kGatherG; ++k) {
        const int c = c0 + k;
        v[k] = 0.f;
        if (live && c < n) {
          const ChanParams q = b.par[c];
          const int32_t sym = decode_symbol<false>(s, b.tab + c * W, q.len) + q.off;
          v[k] = dequantise_one((float)sym, q.bias, q.es, q.med);
        }
      }
#pragma unroll
      for (int j = 0; j < kChunks; ++j)
        park_own(stage, lane, j, float4{v[4 * j], v[4 * j + 1], v[4 * j + 2], v[4 * j + 3]});
      __syncthreads();
      write_out(stage, out, ld_out, g, c_lo + c0, c_lo + n, vec_ok);
      __syncthreads();
    }
  });

  if (live && s.pos > s.nwords) st = 1;
  if (img < B && status) status[img] = st;
  zero_overrun(vote, live && st == 1, out, ld_out, img, C);
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
  EncState s;
  uint8_t *end = open_encoder(s, scratch, stride, i);
  auto load = [](int, auto) {};   // (symbol and row index are read where they are used)
  auto prep = [&](int k, int) {
    const int t = min(max(idx[k], 0), T - 1);
    return prepare_channel(cdf + (size_t)t * W, cdf_len[t], offset[t], sym[k]);
  };
  encode_walk<4>(s, n, load, prep);
  close_encoder(s, end, lengths, i);
}

__global__ __launch_bounds__(kEncThreads) void rans_decode_indexed_kernel(
    const uint8_t *__restrict__ payload, const uint64_t *__restrict__ off, int skip, int B, int n,
    const int32_t *__restrict__ indexes, const int32_t *__restrict__ cdf, int T, int W,
    const int32_t *__restrict__ cdf_len, const int32_t *__restrict__ offset,
    int32_t *__restrict__ out, int32_t *__restrict__ status, unsigned lds_bytes) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const PackedRows rows = stage_packed_rows(smem, lds_bytes, cdf, T, W, cdf_len, offset);
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
  // Two loops, not decode_row's own branch inside one: with the uniform branch per symbol the LDS path measured 7 %
  // slower (0.93 against 0.87 ms for 1024 x 512 symbols); under each arm decode_row's test of rows.in_lds folds away.
  if (rows.in_lds) {
    int t_next = min(max(idx[0], 0), T - 1);
    for (int k = 0; k < n; ++k) {
      const int t = t_next;
      if (k + 1 < n) t_next = min(max(idx[k + 1], 0), T - 1);   // (requested one symbol ahead)
      dst[k] = decode_row(s, rows, t, cdf, W, cdf_len, offset);
    }
  } else {
    for (int k = 0; k < n; ++k) dst[k] = decode_row(s, rows, min(max(idx[k], 0), T - 1), cdf, W, cdf_len, offset);
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
    const float v = as_float(reinterpret_cast<const typename Fetch<ZMODE>::elem *>(z)[i]);
    sym[i] = quantise_one(v, bias[c], es[c], med[c]);
  }
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
    const float v = as_float(reinterpret_cast<const typename Fetch<ZMODE>::elem *>(z)[i]);
    const float t = __fadd_rn(v, bias[c]);
    const float u = __fmul_rn(t, es[c]);
    const float q = rintf(__fsub_rn(u, med[c]));  // EntropyBottleneck.forward, eval mode
    out[i] = dequantise_one(q, bias[c], es[c], med[c]);
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
  with_z(z_dtype, [&](auto zt) {
    quantise_kernel<decltype(zt)::mode><<<g, 256, 0, as_stream(stream)>>>(z, n, C, bias, exp_scale, median, symbols);
  });
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
  with_z(z_dtype, [&](auto zt) {
    rans_encode_kernel<decltype(zt)::mode><<<grid, kEncThreads, lds, as_stream(stream)>>>(
        z, B, C, bias, exp_scale, median, cdf, W, cdf_len, offset, scratch, stride, lengths, symbols_out);
  });
  return check_launch();
}

// compaction of no records: the one offset, 0
static int no_records(uint64_t *out_off, hipStream_t st) {
  if (!out_off) return LLA_EINVAL;
  hipError_t e = hipMemsetAsync(out_off, 0, sizeof(uint64_t), st);
  return e == hipSuccess ? LLA_OK : hip_fail(e);
}

size_t lla_rans_compact_workspace_bytes(int B) {
  const size_t nblk = ((size_t)(B > 0 ? B : 1) + kScanThreads - 1) / kScanThreads;
  return (nblk + 1) * sizeof(uint64_t);
}

int lla_rans_compact(const uint8_t *scratch, size_t stride, const uint32_t *lengths, int B,
                     int record_prefix, uint8_t *out, size_t cap, uint64_t *out_off,
                     void *workspace, size_t workspace_bytes, void *stream) {
  hipStream_t st = as_stream(stream);
  if (B == 0) return no_records(out_off, st);
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
  if (B == 0) return no_records(out_off, st);
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
  with_z(z_dtype, [&](auto zt) {
    using OutT = typename decltype(zt)::elem;
    rans_decode_gather_kernel<OutT><<<grid, kEncThreads, lds, as_stream(stream)>>>(
        payload, off, skip, off_first, off_step, N, index, B, C, cdf, W, cdf_len, offset, bias, exp_scale, median,
        reinterpret_cast<OutT *>(z_hat), ld_out, status);
  });
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

// --- the windowed coder ---
int lla_rans_table_fits(int C, int W, int kind) {
  // the resident launchers' own tests: table_args_ok's bound on the table, then the launch's LDS
  if (C <= 0 || W < 3 || (size_t)C * W * 2 > 64 * 1024) return 0;
  size_t lds;
  if (kind == LLA_CODER_ENCODE) lds = enc_lds_bytes(C, W);
  else if (kind == LLA_CODER_DECODE) lds = enc_table_bytes(C, W) + (size_t)C * sizeof(int2);
  else if (kind == LLA_CODER_GATHER) lds = gather_lds_bytes(C, W);
  else return 0;
  return lds <= 64 * 1024 ? 1 : 0;
}

int lla_rans_wide_window(int C, int W, int kind, int window_channels, size_t *lds_bytes) {
  if (C <= 0 || W < 3 || W > LLA_WIDE_MAX_W || kind < LLA_CODER_ENCODE || kind > LLA_CODER_GATHER || window_channels < 0 ||
      (window_channels & 3))
    return LLA_EINVAL;
  const bool gather = kind == LLA_CODER_GATHER;
  const int cap = C >= kWinMaxChannels ? kWinMaxChannels : (C + 3) & ~3;
  int wc;
  if (window_channels) {
    wc = window_channels < cap ? window_channels : cap;
    if (wide_lds_bytes(wc, W, gather) > kWideLdsMax) return LLA_EINVAL;
  } else {
    // the largest multiple of 16, up to kWinMaxChannels, whose launch stays within kWideLdsBudget (56 KiB: two workgroups
    // on a CU with room to spare, no opt-in above 64 KiB); measured (profiles/wide_coder.txt): fewer, larger windows win --
    // a window costs a barrier and the part of its loads that window_fetch's registers do not keep in flight costs less
    // than that -- and LDS is free at one record per lane (B = 65536 is one workgroup per CU).  16 for rows too long for
    // that, fewer where even those do not fit (W <= LLA_WIDE_MAX_W: 4 channels do)
    wc = cap & ~15;
    while (wc > 16 && wide_lds_bytes(wc, W, gather) > kWideLdsBudget) wc -= 16;
    if (wc < 16) wc = cap < 16 ? cap : 16;
    while (wide_lds_bytes(wc, W, gather) > kWideLdsMax) wc -= 4;
  }
  if (lds_bytes) *lds_bytes = wide_lds_bytes(wc, W, gather);
  return wc;
}

int lla_quantise_encode_wide(const void *z, int z_dtype, int B, int C, const float *bias, const float *exp_scale,
                             const float *median, const int32_t *cdf, int W, const int32_t *cdf_len,
                             const int32_t *offset, uint8_t *scratch, size_t stride, uint32_t *lengths,
                             int32_t *symbols_out, int window_channels, void *stream) {
  if (z_dtype != LLA_Z_SYMBOLS && z_dtype != LLA_Z_F16 && z_dtype != LLA_Z_F32) return LLA_EINVAL;
  size_t lds = 0;
  const int wc = lla_rans_wide_window(C, W, LLA_CODER_ENCODE, window_channels, &lds);
  if (wc < 0 || B < 0) return LLA_EINVAL;
  if (B == 0) return LLA_OK;
  if (!z || !cdf || !cdf_len || !offset || !scratch || !lengths) return LLA_EINVAL;
  if (z_dtype != LLA_Z_SYMBOLS && (!bias || !exp_scale || !median)) return LLA_EINVAL;
  if (stride < lla_rans_max_encoded_bytes(C) || (stride & 3u)) return LLA_ECAP;
  const int grid = (B + kEncThreads - 1) / kEncThreads;
  auto launch = [&](auto zt) {
    rans_encode_wide_kernel<decltype(zt)::mode><<<grid, kEncThreads, lds, as_stream(stream)>>>(
        z, B, C, bias, exp_scale, median, cdf, W, cdf_len, offset, scratch, stride, lengths, symbols_out, wc);
  };
  if (z_dtype == LLA_Z_SYMBOLS) launch(Fetch<0>{});
  else with_z(z_dtype, launch);
  return check_launch();
}

int lla_rans_decode_batch_wide(const uint8_t *payload, const uint64_t *off, int record_prefix, int off_first,
                               int off_step, int B, int C, const int32_t *cdf, int W, const int32_t *cdf_len,
                               const int32_t *offset, int32_t *symbols_out, int32_t *status, int window_channels,
                               void *stream) {
  size_t lds = 0;
  const int wc = lla_rans_wide_window(C, W, LLA_CODER_DECODE, window_channels, &lds);
  if (wc < 0 || B < 0 || off_first < 0 || off_step < 1) return LLA_EINVAL;
  if (B == 0) return LLA_OK;
  if (!payload || !off || !symbols_out || !cdf || !cdf_len || !offset) return LLA_EINVAL;
  const int grid = (B + kEncThreads - 1) / kEncThreads;
  rans_decode_wide_kernel<<<grid, kEncThreads, lds, as_stream(stream)>>>(
      payload, off + off_first, record_prefix ? 4 : 0, off_step, B, C, cdf, W, cdf_len, offset, symbols_out, status, wc);
  return check_launch();
}

int lla_rans_decode_gather_wide(const uint8_t *payload, const uint64_t *off, int record_prefix, int off_first,
                                int off_step, int N, const int64_t *index, int B, int C, const int32_t *cdf, int W,
                                const int32_t *cdf_len, const int32_t *offset, const float *bias,
                                const float *exp_scale, const float *median, void *z_hat, int z_dtype, size_t ld_out,
                                int32_t *status, int window_channels, void *stream) {
  if (z_dtype != LLA_Z_F16 && z_dtype != LLA_Z_F32) return LLA_EINVAL;
  size_t lds = 0;
  const int wc = lla_rans_wide_window(C, W, LLA_CODER_GATHER, window_channels, &lds);
  if (wc < 0 || B < 0 || off_first < 0 || off_step < 1) return LLA_EINVAL;
  if (B == 0) return LLA_OK;
  if (!payload || !off || !index || !bias || !exp_scale || !median || !z_hat || !status || N < 0 || !cdf || !cdf_len ||
      !offset || ld_out < (size_t)C)
    return LLA_EINVAL;
  const int grid = (B + kEncThreads - 1) / kEncThreads;
  const int skip = record_prefix ? 4 : 0;
  with_z(z_dtype, [&](auto zt) {
    using OutT = typename decltype(zt)::elem;
    rans_decode_gather_wide_kernel<OutT><<<grid, kEncThreads, lds, as_stream(stream)>>>(
        payload, off, skip, off_first, off_step, N, index, B, C, cdf, W, cdf_len, offset, bias, exp_scale, median,
        reinterpret_cast<OutT *>(z_hat), ld_out, status, wc);
  });
  return check_launch();
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
  with_z(z_dtype, [&](auto zt) {
    represent_kernel<decltype(zt)::mode><<<g, 256, 0, as_stream(stream)>>>(z, n, C, bias, exp_scale, median, z_hat);
  });
  return check_launch();
}

}  // extern "C"
