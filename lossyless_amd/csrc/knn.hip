// One data pass of a weighted k-nearest-neighbour classifier on the compressed representations (gfx950): the training-free
// protocol for judging frozen features (Wu et al. 2018, sec. 3.4; DINO, Caron et al. 2021, sec. 4.1) -- cosine similarity,
// the k best train rows of every query, each voting exp(s / T) for its class.  The reference has no k-NN; the rows come
// from a decode group of CompressedLatents / HyperpriorLatents, as in probe.hip.
//
//   s_ij = q_i . z_j   (metric 1: times 1 / |z_j|; the caller normalises the queries)
//   list_i = the k best (s_ij, j) over all rows shown so far, ordered by (score descending, global index ascending)
//
// Shape of the pass kernel.  A persistent workgroup (4 waves) owns one tile of 32 queries and walks row tiles of 32 rows:
//   0. once: its share of the query tile goes to REGISTERS -- lane l of wave w holds columns 8 g + 4 (l >> 5) .. + 3 of query
//      l & 31 for the column groups g = w, w + 4, ... (C / 8 floats per lane: 64 VGPRs at C = 512, 128 at C = 1024), so the
//      queries are read from memory once per call, not once per row tile;
//   1. the row tile is staged in LDS once, as fp32 (fp16 rows are widened exactly), pitch C + 4 floats (row_tile.h);
//      cosine: eight threads per row take the row's sum of squares over their columns, in an order fixed by C;
//   2. scores: S[32 queries][32 rows] = Q_tile Z_tile^T on v_mfma_f32_32x32x2_f32, the C dimension dealt to the four waves
//      in groups of 8 and their partial tiles added through LDS in a fixed order ((w0 + w2) + (w1 + w3));
//   3. selection: wave w owns queries 8 w .. 8 w + 7 of the tile and keeps their lists in REGISTERS -- entry t of a list is
//      slot t & 3 of lane t >> 2 (256 entries: 8 VGPRs per query, 64 per wave) -- next to each list's k-th entry.  Lane r reads
//      the score of row r, scales it by 1 / |z_r| and compares it with the k-th entry: one ballot per query.  Only a winner is
//      inserted (two cross-lane shifts and four selects per slot), and the k-th entry is read again.  After the first tiles
//      almost every ballot is empty: a walker that sees m rows inserts about k (1 + ln(m / k)) of them per query.
// Scores never leave the chip; a staged tile is read from HBM / L2 once per query tile.  LDS: 32 (C + 4) + 2 * 1024 + 256
// floats -- 76.5 KB at C = 512 (two workgroups per CU: one's staging runs beside the other's MFMAs), 140.5 KB at C = 1024.
//
// Every walker of a split train range keeps its own lists in the workspace ([query tile][walker][32][k] scores, then the
// same shape of indexes); the number of walkers is a function of Q alone.  knn_finish_kernel merges a query's lists in walker
// order by the same insertion, writes them out and takes the votes serially in rank order, one thread per class.
//
// Determinism: a score's bits depend on (q_i, z_j, C, metric) alone -- the MFMA chain of a wave runs over its column groups
// in ascending order, the four partial tiles and the eight partial sums of squares are added in a fixed order, and none of it
// depends on where row j falls in a tile, a call or a walker's range.  The order (score descending, index ascending) is
// total, a walker's list is the top k of the rows it saw, and the top k of a union is the top k of the parts' top k: the
// result is a pure function of the rows shown.  No floating-point atomics (the insertion counter is an integer).
#include "row_tile.h"

#include <limits.h>

namespace lla {
namespace {

constexpr int kQueries = kClasses; // queries per workgroup: the "classes" of row_tile.h's score tile
constexpr int kSlots = 4;          // list entries per lane: 64 lanes x 4 = kMaxK
constexpr int kMaxK = 256;
constexpr int kWalkersMax = 64;    // lists a query's merge reads at the most

__host__ __device__ inline int lds_floats(int C) { return kRows * (C + kZPad) + 2 * kRows * kQueries + kRows * 8; }
inline int query_tiles(int Q) { return class_tiles(Q); }
inline int walkers_of(int nqt) { const int w = tile_walkers(nqt); return w > kWalkersMax ? kWalkersMax : w; }

// entry (ev, ei) stands before the candidate (cs, cj) in the order (score descending, index ascending)
__device__ __forceinline__ bool before(float ev, int ei, float cs, int cj) { return ev > cs || (ev == cs && ei < cj); }

// A sorted list of 256 entries across the wave: entry t is (v[t & 3], ix[t & 3]) of lane t >> 2.  Inserts the candidate at
// its place; every entry behind it moves one place back and the last falls off.  All 64 lanes must be active.
__device__ __forceinline__ void list_insert(float (&v)[kSlots], int (&ix)[kSlots], float cs, int cj, int lane) {
  float pv = __shfl_up(v[kSlots - 1], 1);          // the entry before this lane's first
  int pi = __shfl_up(ix[kSlots - 1], 1);
  bool pb = lane == 0 ? true : before(pv, pi, cs, cj);
#pragma unroll
  for (int s = 0; s < kSlots; ++s) {
    const bool b = before(v[s], ix[s], cs, cj);    // stays where it is
    const float nv = b ? v[s] : (pb ? cs : pv);
    const int ni = b ? ix[s] : (pb ? cj : pi);
    pv = v[s], pi = ix[s], pb = b;
    v[s] = nv, ix[s] = ni;
  }
}

// entry t of the list, in every lane
__device__ __forceinline__ void list_entry(const float (&v)[kSlots], const int (&ix)[kSlots], int t, float &ev, int &ei) {
  const int s = t & 3;
  const float sv = s == 0 ? v[0] : s == 1 ? v[1] : s == 2 ? v[2] : v[3];
  const int si = s == 0 ? ix[0] : s == 1 ? ix[1] : s == 2 ? ix[2] : ix[3];
  ev = __shfl(sv, t >> 2);
  ei = __shfl(si, t >> 2);
}

// this lane's entries of a list of k in memory; the entries from k on are empty
__device__ __forceinline__ void list_load(float (&v)[kSlots], int (&ix)[kSlots], const float *__restrict__ vals,
                                          const int32_t *__restrict__ idx, int k, int lane) {
#pragma unroll
  for (int s = 0; s < kSlots; ++s) {
    const int t = kSlots * lane + s;
    v[s] = (vals && t < k) ? vals[t] : -INFINITY;
    ix[s] = (vals && t < k) ? idx[t] : -1;
  }
}

// NG: column groups of 8 per wave (C <= 32 NG).  Workspace: vals [query tile][walker][32][k], idx the same, a counter.
template <int NG>
__global__ __launch_bounds__(256) void knn_pass_kernel(const float *__restrict__ q, int ld_q, int Q,
                                                       const void *__restrict__ z, int z_f16, int ld_z, int n, int C,
                                                       int row_base, int k, int cosine,
                                                       const int32_t *__restrict__ q_self, int accumulate,
                                                       float *__restrict__ ws_val, int32_t *__restrict__ ws_idx,
                                                       unsigned long long *__restrict__ inserted) {
  extern __shared__ __align__(16) float lds[];
  const int pitch = C + kZPad, ngroups = C >> 3;
  float *Zs = lds;                               // [32 rows][pitch]
  float *Sp = Zs + kRows * pitch;                // [slot][32 queries][32 rows]
  float *Np = Sp + 2 * kRows * kQueries;         // [32 rows][8] partial sums of squares

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int r32 = lane & 31, hk = lane >> 5;
  const int qt = blockIdx.y, P = gridDim.x, p = blockIdx.x;
  const int q0 = qt * kQueries;
  const int ntiles = (n + kRows - 1) / kRows;
  if (accumulate && p >= ntiles) return;         // nothing to add to this walker's lists

  // 0. the query tile: "A" lane l = Q[q0 + (l & 31)][c + (l >> 5)]  (gemm_f32.hip); clamped queries are computed and unused
  f32x4 qreg[NG];
  {
    const int qrow = q0 + r32 < Q ? q0 + r32 : Q - 1;
    const float *qp = q + (size_t)qrow * ld_q + 4 * hk;
#pragma unroll
    for (int i = 0; i < NG; ++i) {
      const int g = wid + 4 * i;
      qreg[i] = g < ngroups ? *reinterpret_cast<const f32x4 *>(qp + 8 * g) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
  }

  // the lists of this wave's eight queries, their k-th entries and the indexes they skip
  float lv[8][kSlots], tv[8];
  int li[8][kSlots], ti[8], self[8];
  const size_t list0 = ((size_t)(qt * P + p) * kQueries + 8 * wid) * k;
#pragma unroll
  for (int qi = 0; qi < 8; ++qi) {
    const int qg = q0 + 8 * wid + qi;
    const bool load = accumulate && qg < Q;
    list_load(lv[qi], li[qi], load ? ws_val + list0 + (size_t)qi * k : nullptr, ws_idx + list0 + (size_t)qi * k, k, lane);
    list_entry(lv[qi], li[qi], k - 1, tv[qi], ti[qi]);
    self[qi] = (q_self && qg < Q) ? q_self[qg] : -1;
  }
  unsigned count = 0;

  for (int tile = p; tile < ntiles; tile += P) {
    const int row0 = tile * kRows;
    stage_rows(Zs, z, z_f16, ld_z, row0, n, C, tid);                 // 1.
    __syncthreads();
    if (cosine) row_squares(Zs, Np, C, tid);     // (read after the barriers of step 2)

    // 2. scores: "B" lane l = Z[row (l & 31)][c + (l >> 5)]; the query operand is in registers, so the MFMA loop is this
    // file's and only the merge of the partial tiles is row_tile.h's
    f32x16 s;
#pragma unroll
    for (int r = 0; r < 16; ++r) s[r] = 0.f;
#pragma unroll
    for (int i = 0; i < NG; ++i) {
      const int g = wid + 4 * i;
      if (g < ngroups) {
        const f32x4 a = *reinterpret_cast<const f32x4 *>(Zs + r32 * pitch + 8 * g + 4 * hk);
#pragma unroll
        for (int j = 0; j < 4; ++j) s = __builtin_amdgcn_mfma_f32_32x32x2f32(qreg[i][j], a[j], s, 0, 0, 0);
      }
    }
    merge_score_slots<false>(Sp, s, s, r32, hk, wid);

    // 3. selection: lane r < 32 holds the candidate of row r
    const float rinv = cosine ? inv_norm(row_n2(Np, r32)) : 1.f;
    const bool row_ok = hk == 0 && row0 + r32 < n;
    const int j = row_base + row0 + r32;
#pragma unroll
    for (int qi = 0; qi < 8; ++qi) {
      const int ql = 8 * wid + qi;
      if (q0 + ql >= Q) continue;
      float sc = Sp[ql * kRows + r32] + Sp[kRows * kQueries + ql * kRows + r32];
      if (cosine) sc *= rinv;
      bool win = row_ok && j != self[qi] && before(sc, j, tv[qi], ti[qi]);
      unsigned long long mask = __ballot(win);
      while (mask) {
        const int b = __ffsll((long long)mask) - 1;
        list_insert(lv[qi], li[qi], __shfl(sc, b), row_base + row0 + b, lane);
        list_entry(lv[qi], li[qi], k - 1, tv[qi], ti[qi]);
        ++count;
        win = win && lane != b && before(sc, j, tv[qi], ti[qi]);     // the k-th entry moved up: some winners no longer are
        mask = __ballot(win);
      }
    }
    // (the next tile's staging writes Zs only; a barrier follows it before Sp and Np are written again)
  }

  // this walker's lists -> workspace
#pragma unroll
  for (int qi = 0; qi < 8; ++qi) {
    if (q0 + 8 * wid + qi >= Q) continue;
#pragma unroll
    for (int sl = 0; sl < kSlots; ++sl) {
      const int t = kSlots * lane + sl;
      if (t < k) {
        ws_val[list0 + (size_t)qi * k + t] = lv[qi][sl];
        ws_idx[list0 + (size_t)qi * k + t] = li[qi][sl];
      }
    }
  }
  if (lane == 0 && count) atomicAdd(inserted, (unsigned long long)count);
}

// One wave per query: the lists of walkers 0 .. P-1 merged in that order, written out, and the votes.
__global__ __launch_bounds__(64) void knn_finish_kernel(int Q, int k, int k_out, int P, const float *__restrict__ ws_val,
                                                        const int32_t *__restrict__ ws_idx,
                                                        const int32_t *__restrict__ labels, int K, float inv_T,
                                                        float *__restrict__ top_val, int32_t *__restrict__ top_idx,
                                                        float *__restrict__ votes) {
  __shared__ float wgt[kMaxK];
  __shared__ int cls[kMaxK];
  const int lane = threadIdx.x, i = blockIdx.x;
  const int qt = i / kQueries, ql = i - qt * kQueries;
  float v[kSlots], wv[kSlots], tv, ev;
  int ix[kSlots], wi[kSlots], ti, ei;
  const size_t at0 = ((size_t)qt * P * kQueries + ql) * k;
  list_load(v, ix, ws_val + at0, ws_idx + at0, k, lane);
  list_entry(v, ix, k - 1, tv, ti);
  for (int p = 1; p < P; ++p) {
    const size_t at = ((size_t)(qt * P + p) * kQueries + ql) * k;
    list_load(wv, wi, ws_val + at, ws_idx + at, k, lane);
    for (int t = 0; t < k; ++t) {                // a sorted list: behind its first loser everything loses
      list_entry(wv, wi, t, ev, ei);
      if (ei < 0 || !before(ev, ei, tv, ti)) break;
      list_insert(v, ix, ev, ei, lane);
      list_entry(v, ix, k - 1, tv, ti);
    }
  }
  const float best = __shfl(v[0], 0);
#pragma unroll
  for (int s = 0; s < kSlots; ++s) {
    const int t = kSlots * lane + s;
    if (t < k_out) {                             // (the top k_out of a query are the first k_out of its top k)
      top_val[(size_t)i * k_out + t] = v[s];
      top_idx[(size_t)i * k_out + t] = ix[s];
      if (labels) {
        const int c = ix[s] >= 0 ? labels[ix[s]] : -1;
        cls[t] = c;
        wgt[t] = (c >= 0 && c < K) ? expf((v[s] - best) * inv_T) : 0.f;
      }
    }
  }
  if (!labels) return;
  __syncthreads();
  for (int c = lane; c < K; c += 64) {           // serially in rank order
    float sum = 0.f;
    for (int r = 0; r < k_out; ++r)
      if (cls[r] == c) sum += wgt[r];
    votes[(size_t)i * K + c] = sum;
  }
}

const void *pass_kernel(int C) {
  if (C <= 128) return reinterpret_cast<const void *>(&knn_pass_kernel<4>);
  if (C <= 256) return reinterpret_cast<const void *>(&knn_pass_kernel<8>);
  if (C <= 512) return reinterpret_cast<const void *>(&knn_pass_kernel<16>);
  return reinterpret_cast<const void *>(&knn_pass_kernel<32>);
}

bool lists_ok(int Q, int k) { return Q >= 1 && k >= 1 && k <= kMaxK && query_tiles(Q) <= 65535; }
size_t list_entries(int Q, int k) {
  const int nqt = query_tiles(Q);
  return (size_t)nqt * walkers_of(nqt) * kQueries * k;
}

}  // namespace
}  // namespace lla

using namespace lla;

extern "C" size_t lla_knn_pass_workspace_bytes(int Q, int k) {
  if (!lists_ok(Q, k)) return 0;
  return list_entries(Q, k) * (sizeof(float) + sizeof(int32_t)) + sizeof(unsigned long long);
}

extern "C" int lla_knn_pass(const float *q, int ld_q, int Q, const void *z, int z_dtype, int ld_z, int n, int C, int row_base,
                            int k, int metric, const int32_t *q_self, int accumulate, void *workspace, void *stream) {
  if (!lists_ok(Q, k) || !cols_ok(C) || !rows_ok(z, z_dtype, ld_z, n, C) || row_base < 0 ||
      (long long)row_base + n > INT_MAX || (metric != 0 && metric != 1) || ld_q < C || (ld_q & 3))
    return LLA_EINVAL;
  if (!q || !workspace || ((uintptr_t)q & 15) || ((uintptr_t)workspace & 7)) return LLA_EINVAL;
  if (n == 0) return LLA_OK;

  const int nqt = query_tiles(Q), P = walkers_of(nqt);
  const size_t entries = list_entries(Q, k);
  float *ws_val = static_cast<float *>(workspace);
  int32_t *ws_idx = reinterpret_cast<int32_t *>(ws_val + entries);
  unsigned long long *inserted = reinterpret_cast<unsigned long long *>(ws_idx + entries);
  const void *kernel = pass_kernel(C);
  const size_t lds_bytes = (size_t)lds_floats(C) * sizeof(float);
  if (lds_bytes > dynamic_lds_limit(kernel)) return LLA_ECAP;
  const int z_f16 = z_dtype == LLA_Z_F16;
  void *args[] = {(void *)&q, (void *)&ld_q, (void *)&Q, (void *)&z, (void *)&z_f16, (void *)&ld_z, (void *)&n, (void *)&C,
                  (void *)&row_base, (void *)&k, (void *)&metric, (void *)&q_self, (void *)&accumulate, (void *)&ws_val,
                  (void *)&ws_idx, (void *)&inserted};
  hipError_t e = hipLaunchKernel(kernel, dim3(P, nqt), dim3(256), args, lds_bytes, as_stream(stream));
  return e == hipSuccess ? LLA_OK : hip_fail(e);
}

extern "C" int lla_knn_finish(int Q, int k, int k_out, const int32_t *labels, int K, float inv_T, float *top_val,
                              int32_t *top_idx, float *votes, const void *workspace, void *stream) {
  if (!lists_ok(Q, k) || k_out < 1 || k_out > k || !top_val || !top_idx || !workspace || ((uintptr_t)workspace & 7)) return LLA_EINVAL;
  if (labels && (K < 1 || !votes)) return LLA_EINVAL;
  const int nqt = query_tiles(Q), P = walkers_of(nqt);
  const size_t entries = list_entries(Q, k);
  const float *ws_val = static_cast<const float *>(workspace);
  const int32_t *ws_idx = reinterpret_cast<const int32_t *>(ws_val + entries);
  knn_finish_kernel<<<Q, 64, 0, as_stream(stream)>>>(Q, k, k_out, P, ws_val, ws_idx, labels, K, inv_T, top_val, top_idx, votes);
  return check_launch();
}
