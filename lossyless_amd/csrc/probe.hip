// One data pass of a linear probe on the compressed representations (gfx950): the squared-hinge sums that
// `LinearSVC(C).fit(Z, Y)` needs -- the third step of the reference's published workflow, after compress_dataset and
// decompress_dataset (README.md:74-82 of the reference; notebooks/Hub.ipynb:415) -- for all K one-vs-rest
// classifiers at once, from rows that a decode group of CompressedLatents / HyperpriorLatents has just left in HBM.
//
//   s_ik = z_i . W_k + b_k      y_ik = +1 iff y[i] == k      m_ik = max(0, 1 - y_ik s_ik)
//   gradient mode (V == NULL):   out_loss[k] = sum_i m_ik^2,   out_W[k] = sum_i (-2 y_ik m_ik) z_i,   out_b[k] = sum_i (-2 y_ik m_ik)
//   Hessian-vector mode:         t_ik = [m_ik > 0] (z_i . V_k + vb_k),   out_W[k] = sum_i 2 t_ik z_i,   out_b[k] = sum_i 2 t_ik
//
// Shape of the kernel.  A persistent workgroup (4 waves) owns one tile of 32 classes and walks row tiles of 32 rows:
//   1. the row tile is staged in LDS once, as fp32 (fp16 rows are widened exactly), pitch C + 4 floats;
//   2. scores: S[32 classes][32 rows] = W_tile Z_tile^T on v_mfma_f32_32x32x2_f32, the C dimension dealt to the four waves
//      in groups of 8 and their partial tiles added through LDS in a fixed order;
//   3. residuals r_ik (-2 y m, or 2 t) in registers, one (row, 4 classes) per thread, written to LDS [row][class];
//   4. gradient: G[32 classes][C] += R^T Z_tile, a second MFMA whose operands are both in LDS; each wave keeps its
//      C / 4 columns of the slice in accumulator registers over ALL its row tiles (64 VGPRs at C = 512).
// Steps 1, 2 and 4 and the ordered sum of the partials are row_tile.h's, shared with knn.hip and kmeans.hip; step 3 is here.
// z is read from HBM once per class tile; scores and residuals never leave the chip.  At C <= 512 the workgroup needs
// 78.6 KB of LDS, so two of them share a CU and one's staging runs beside the other's MFMAs.
//
// Determinism: no floating-point atomics.  Every workgroup writes its partial sums to the workspace and
// svm_reduce_kernel adds them in workgroup order (the loss in double); the number of workgroups is a function of
// (B, K) alone, so two calls on the same inputs give the same bits.
//
// Arithmetic: exact fp32 products, fp32 accumulation (the MFMA is an fma chain), as gemm_f32.hip.
//
// The grid pass (lla_svm_grid_pass; GRID below) is the same walk over J independent problems in the place of the K
// classes: problem j has its own positive class, its own held-out fold and one weight per sign,
//   y_ij = +1 iff y[i] == col_class[j]      c_ij = 0 if fold[i] == col_held[j], else col_cpos[j] / col_cneg[j] by the sign
//   out_loss[j] = sum_i c_ij m_ij^2,   residual c_ij (-2 y_ij m_ij)   or   c_ij 2 t_ij
// -- every (candidate, fold, class) of a cross-validated search over C and class_weight in the passes of one fit.  The
// four numbers of a column live in registers next to its intercept; the weight is one multiply of the residual and of
// the loss term in step 3, so unit weights and no fold give the bits of lla_svm_pass.
//
// The softmax pass (lla_softmax_pass; kSoftmax below) is the same walk for L2-regularised multinomial logistic regression
// (CLIP's linear-probe protocol; the cross-entropy of the reference's predictors, lossyless/predictors.py:172-186):
//   lse_i = log sum_k exp(s_ik)      p_ik = exp(s_ik - lse_i)      w_i = class_weight[y_i]  (0 for a label outside [0, K))
//   gradient mode:        r_ik = w_i (p_ik - [y_i = k]),   out_loss[k] = sum_{i: y_i = k} w_i (lse_i - s_ik)
//   Hessian-vector mode:  a_i = sum_k p_ik t_ik,   r_ik = w_i p_ik (t_ik - a_i)
// Only step 3 differs, and it needs two numbers per row that couple all K classes.  K <= 32: the tile's 32 x 32 scores are
// in LDS after step 2, so every thread reads the real classes of its row and takes max, sum and a_i itself -- K more expf
// per thread, no barrier, no second kernel.  K > 32: softmax_rows_kernel runs first -- the same staging and the same score
// MFMA over ALL class tiles of a row tile, a running (max, sum exp(s - max), sum exp(s - max) t) per thread over its classes,
// merged per row at the end of the row tile -- and leaves lse[B], a[B] in the workspace for step 3 to read.
//
// The softmax grid pass (lla_softmax_grid_pass; kSoftGrid below) is that walk over G classifiers ("groups") of K <= 32
// classes each -- every (candidate, fold) of a cross-validated search -- which see the same rows: group g leaves the rows of
// fold group_held[g] out and weighs the others by group_class_weight[g][y_i] (selected, not multiplied: no rounding is added).
// A 32-column tile holds gpt = 32 / K whole groups: tile ct starts at column ct gpt K of the dense [G K] layout, column cl of
// it is class cl % K of group ct gpt + cl / K, and the columns from gpt K on (and those of groups >= G) are dead: clamped
// for the loads, residual 0.  Only step 3 differs: a thread's four columns lie in up to four groups, and it takes
// (max, sum exp, sum exp t) of each of them itself from that group's K scores in LDS, in class order -- the loop of the
// softmax pass over another range, so a group's outputs are the bits lla_softmax_pass gives when the grids agree.
#include "row_tile.h"

namespace lla {
namespace {

constexpr int kRPitch = kClasses + 1;

// what step 3 computes: lla_svm_pass, lla_svm_grid_pass, lla_softmax_pass, lla_softmax_grid_pass
enum { kHinge = 0, kGrid = 1, kSoftmax = 2, kSoftGrid = 3 };

// (the softmax pass keeps the tile's 32 b and 32 vb behind Rs)
__host__ __device__ inline int lds_floats(int C, bool softmax = false) {
  return kRows * (C + kZPad) + 2 * kRows * kClasses + kRows * kRPitch + (softmax ? 2 * kClasses : 0);
}
inline int walkers_max(int K) { return tile_walkers(class_tiles(K)); }
// softmax grid pass: the columns of a tile that hold whole groups of K classes, and the tiles G groups take
inline int group_tile_cols(int K) { return (kClasses / K) * K; }
inline long long group_tiles(int K, int G) { const int gpt = kClasses / K; return ((long long)G + gpt - 1) / gpt; }

// The columns of a grid pass: what makes problem j of lla_svm_grid_pass differ from class j of lla_svm_pass.
struct GridCols {
  const int32_t *fold;       // [B] or NULL: no row is held out
  const int32_t *col_class;  // [J]
  const int32_t *col_held;   // [J]
  const float *col_cpos;     // [J]
  const float *col_cneg;     // [J]
};

// What makes a softmax pass differ: the row weights, and for K > 32 the row statistics softmax_rows_kernel left.
struct SoftmaxRows {
  const float *class_weight;  // [K] or NULL: every row weighs 1
  const float *lse;           // [B]; NULL when one class tile holds all K classes: step 3 takes the statistics itself
  const float *a;             // [B] (Hessian-vector mode)
  // kSoftGrid: class_weight is [G][classes]; the row's fold id and the groups' held-out folds come in GridCols
  // (fold, col_held [G]), and K is the number of real columns, G classes
  int classes;                // classes per group
};

// HV: Hessian-vector mode.  NT: 32-column tiles of the gradient slice per wave (C <= 128 NT).  OBJ: kHinge -- column k is
// class k, nothing is held out and every weight is 1; kGrid -- the columns are the problems of `cols` (K is their number J);
// kSoftmax -- column k is class k and step 3 is the softmax residual of `sm`; kSoftGrid -- a tile's first
// (32 / sm.classes) sm.classes columns are whole groups of sm.classes classes (K is the number of real columns, G classes),
// the row's fold id and the groups' held-out folds are in `cols`, and step 3 is the softmax residual per group.
// Workspace: part_W [class tile][walker][32][C], part_b / part_l [class tile][walker][32].
template <bool HV, int NT, int OBJ>
__global__ __launch_bounds__(256) void svm_pass_kernel(const void *__restrict__ z, int z_f16, int ld_z,
                                                       const int32_t *__restrict__ y, int B, int C,
                                                       const float *__restrict__ W, const float *__restrict__ bias,
                                                       const float *__restrict__ V, const float *__restrict__ vbias,
                                                       int K, int ld_w, float *__restrict__ part_W,
                                                       float *__restrict__ part_b, float *__restrict__ part_l,
                                                       GridCols cols, SoftmaxRows sm) {
  extern __shared__ __align__(16) float lds[];
  constexpr int NSLOT = HV ? 1 : 2;            // score partials kept apart in LDS (HV holds two products: same bytes)
  constexpr bool GRID = OBJ == kGrid, SOFTMAX = OBJ == kSoftmax, SOFTGRID = OBJ == kSoftGrid;
  const int pitch = C + kZPad;
  float *Zs = lds;                             // [32 rows][pitch]
  float *Sp = Zs + kRows * pitch;              // [product][slot][32 classes][32 rows]
  float *Rs = Sp + 2 * kRows * kClasses;       // [32 rows][33]
  float *Bs = Rs + kRows * kRPitch;            // SOFTMAX, SOFTGRID: b and vb of the tile's classes, [2][32]

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int r32 = lane & 31, hk = lane >> 5;
  const int ct = blockIdx.y, P = gridDim.x, p = blockIdx.x;
  const int ncols = SOFTGRID ? (kClasses / sm.classes) * sm.classes : kClasses;      // live columns of a full tile
  const int k0 = ct * ncols;

  // scores: "A" lane l = W[k0 + (l & 31)][c + (l >> 5)], "B" lane l = Z[row (l & 31)][c + (l >> 5)]  (gemm_f32.hip)
  int n = k0 + r32;
  if (n >= K) n = K - 1;                       // clamped classes are computed and masked below
  const float *wp = W + (size_t)n * ld_w + 4 * hk;
  const float *vp = HV ? V + (size_t)n * ld_w + 4 * hk : nullptr;

  // residuals: this thread's row of the tile and its four classes
  const int rr = tid & 31, cl0 = tid >> 5;
  float bk[4], vbk[4];
  bool c_ok[4];
  int ccls[4], cheld[4];                       // GRID: the column's positive class and held-out fold,
  float cpos[4], cneg[4];                      //       its weight for positive and for negative rows
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int c = k0 + cl0 + 8 * j;
    c_ok[j] = c < K && (!SOFTGRID || cl0 + 8 * j < ncols);
    bk[j] = c_ok[j] ? bias[c] : 0.f;
    vbk[j] = (HV && c_ok[j]) ? vbias[c] : 0.f;
    ccls[j] = (GRID && c_ok[j]) ? cols.col_class[c] : c;
    cheld[j] = (GRID && c_ok[j]) ? cols.col_held[c] : 0;
    cpos[j] = (GRID && c_ok[j]) ? cols.col_cpos[c] : 0.f;
    cneg[j] = (GRID && c_ok[j]) ? cols.col_cneg[c] : 0.f;
  }
  const bool folds = GRID && cols.fold != nullptr;
  if ((SOFTMAX || SOFTGRID) && tid < kClasses) {         // (visible after the barrier that follows the first staging)
    const bool real = k0 + tid < K && tid < ncols;
    Bs[tid] = real ? bias[k0 + tid] : 0.f;
    Bs[kClasses + tid] = (HV && real) ? vbias[k0 + tid] : 0.f;
  }
  // SOFTGRID: per column its group's first column in the tile, its held-out fold and its K class weights
  int gcol[4], gheld[4];
  const float *gcw[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    gcol[j] = 0, gheld[j] = 0, gcw[j] = nullptr;
    if (SOFTGRID && c_ok[j]) {
      const int gi = (cl0 + 8 * j) / sm.classes, g = (k0 + cl0 + 8 * j) / sm.classes;
      gcol[j] = gi * sm.classes;
      gheld[j] = cols.fold ? cols.col_held[g] : 0;
      gcw[j] = sm.class_weight ? sm.class_weight + (size_t)g * sm.classes : nullptr;
    }
  }

  f32x16 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
  float lacc[4] = {0.f, 0.f, 0.f, 0.f}, bacc[4] = {0.f, 0.f, 0.f, 0.f};

  const int ntiles = (B + kRows - 1) / kRows;
  for (int tile = p; tile < ntiles; tile += P) {
    const int row0 = tile * kRows;
    stage_rows(Zs, z, z_f16, ld_z, row0, B, C, tid);                 // 1.
    __syncthreads();
    tile_scores<HV>(Zs, Sp, wp, vp, C, lane, wid);                   // 2.

    // 3. residuals
    if constexpr (SOFTGRID) {
      const bool row_ok = row0 + rr < B;
      const int yy = row_ok ? y[row0 + rr] : -1;
      const bool live = yy >= 0 && yy < sm.classes;      // any other row weighs 0 in every group
      const int ff = (cols.fold && row_ok) ? cols.fold[row0 + rr] : 0;
      const auto score = [&](int cl) {         // (as the softmax pass)
        float sc = Sp[cl * kRows + rr];
        if (NSLOT == 2) sc += Sp[kRows * kClasses + cl * kRows + rr];
        return sc + Bs[cl];
      };
      const auto tangent = [&](int cl) { return Sp[kRows * kClasses + cl * kRows + rr] + Bs[kClasses + cl]; };
      int have = -1;                           // the group whose statistics lse / ai hold: the columns' groups ascend with j
      float lse = 0.f, ai = 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int cl = cl0 + 8 * j;
        // the row trains group j: its label is a class and its fold is not the one the group holds out
        const bool on = live && c_ok[j] && !(cols.fold && ff == gheld[j]);
        float r = 0.f;
        if (on) {
          if (gcol[j] != have) {               // the statistics over the group's classes in class order, as the softmax pass
            have = gcol[j];
            float mx = score(have);
            for (int k = 1; k < sm.classes; ++k) mx = fmaxf(mx, score(have + k));
            float se = 0.f, st = 0.f;
            for (int k = 0; k < sm.classes; ++k) {
              const float e = expf(score(have + k) - mx);
              se += e;
              if (HV) st += e * tangent(have + k);
            }
            lse = mx + logf(se);
            if (HV) ai = st / se;
          }
          const float wi = gcw[j] ? gcw[j][yy] : 1.f;
          const float sc = score(cl);
          const bool own = yy == cl - gcol[j];
          const float pk = expf(sc - lse);
          r = HV ? wi * pk * (tangent(cl) - ai) : wi * (pk - (own ? 1.f : 0.f));
          if (!HV && own) lacc[j] += wi * (lse - sc);
        }
        bacc[j] += r;
        Rs[rr * kRPitch + cl] = r;
      }
    } else if constexpr (SOFTMAX) {
      const bool row_ok = row0 + rr < B;
      const int yy = row_ok ? y[row0 + rr] : -1;
      const bool live = yy >= 0 && yy < K;     // any other row weighs 0: it contributes exactly nothing
      const float wi = live ? (sm.class_weight ? sm.class_weight[yy] : 1.f) : 0.f;
      const auto score = [&](int cl) {         // (the additions in the order of the hinge passes)
        float sc = Sp[cl * kRows + rr];
        if (NSLOT == 2) sc += Sp[kRows * kClasses + cl * kRows + rr];
        return sc + Bs[cl];
      };
      const auto tangent = [&](int cl) { return Sp[kRows * kClasses + cl * kRows + rr] + Bs[kClasses + cl]; };
      float lse = 0.f, ai = 0.f;
      if (sm.lse == nullptr) {                 // one class tile: the row's statistics from its real classes' scores in LDS
        const int nreal = K - k0 < kClasses ? K - k0 : kClasses;
        float mx = score(0);
        for (int cl = 1; cl < nreal; ++cl) mx = fmaxf(mx, score(cl));
        float se = 0.f, st = 0.f;
        for (int cl = 0; cl < nreal; ++cl) {
          const float e = expf(score(cl) - mx);
          se += e;
          if (HV) st += e * tangent(cl);
        }
        lse = mx + logf(se);
        if (HV) ai = st / se;
      } else if (row_ok) {
        lse = sm.lse[row0 + rr];
        if (HV) ai = sm.a[row0 + rr];
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int cl = cl0 + 8 * j;
        const float sc = score(cl);
        const bool own = live && yy == k0 + cl;
        float r = 0.f;
        if (live && c_ok[j]) {
          const float pk = expf(sc - lse);
          r = HV ? wi * pk * (tangent(cl) - ai) : wi * (pk - (own ? 1.f : 0.f));
        }
        if (!HV && own) lacc[j] += wi * (lse - sc);
        bacc[j] += r;
        Rs[rr * kRPitch + cl] = r;
      }
    } else {
      const bool row_ok = row0 + rr < B;
      const int yy = row_ok ? y[row0 + rr] : -1;
      const int ff = (folds && row_ok) ? cols.fold[row0 + rr] : 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int cl = cl0 + 8 * j;
        float sc = Sp[cl * kRows + rr];
        if (NSLOT == 2) sc += Sp[kRows * kClasses + cl * kRows + rr];
        sc += bk[j];
        const float ys = (yy == ccls[j]) ? 1.f : -1.f;
        float m = 1.f - ys * sc;
        m = (m > 0.f && row_ok && c_ok[j]) ? m : 0.f;
        const float cw = (folds && ff == cheld[j]) ? 0.f : (ys > 0.f ? cpos[j] : cneg[j]);      // GRID only
        float r;
        if (HV) {
          const float t = Sp[kRows * kClasses + cl * kRows + rr] + vbk[j];
          r = m > 0.f ? 2.f * t : 0.f;
          if (GRID) r *= cw;
        } else {
          r = -2.f * ys * m;
          if (GRID) r *= cw;
          lacc[j] += GRID ? m * m * cw : m * m;
        }
        bacc[j] += r;
        Rs[rr * kRPitch + cl] = r;
      }
    }
    __syncthreads();

    // 4. gradient slice: "A" lane l = R[row 2 s + (l >> 5)][class l & 31]
    slice_mfma(acc, Zs, [&](int row) { return Rs[row * kRPitch + r32]; }, C, lane, wid);
    __syncthreads();                           // the next tile's staging overwrites Zs, Sp and Rs
  }

  // this workgroup's partial sums -> workspace (classes beyond K, and the dead columns from `ncols` on of a kSoftGrid tile,
  // hold exact zeros and are never read: svm_reduce_kernel maps output k to slot k % ncols of tile k / ncols)
  slice_store(acc, part_W + (size_t)(ct * P + p) * kClasses * C, C, lane, wid);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    Sp[(cl0 + 8 * j) * kRows + rr] = bacc[j];
    if (!HV) Sp[kRows * kClasses + (cl0 + 8 * j) * kRows + rr] = lacc[j];
  }
  __syncthreads();
  if (tid < (HV ? 32 : 64)) {
    const float *src = Sp + (tid >> 5) * (kRows * kClasses) + (tid & 31) * kRows;
    float sum = 0.f;
    for (int r = 0; r < kRows; ++r) sum += src[r];
    (tid < 32 ? part_b : part_l)[(size_t)(ct * P + p) * kClasses + (tid & 31)] = sum;
  }
}

// The row statistics of a softmax pass over more than one class tile: lse[i] = log sum_k exp(s_ik) and, in Hessian-vector
// mode, a[i] = sum_k p_ik t_ik.  A persistent workgroup stages a row tile as step 1 does and takes the scores of every class
// tile with the MFMA of step 2 (the same bits the pass kernel will see).  Thread (row, q) sees classes q + 8 j of every
// tile -- at least four real ones in the first, which is full -- and keeps a running max m, sum exp(s - m) and
// sum exp(s - m) t over them, rescaled when the max moves; classes beyond K are skipped, so m is finite from the first
// tile on and no exponent is ever formed from two infinities.  The eight partial triples of a row are merged in the order
// of q once per row tile.  The grid is a function of B alone.
template <bool HV>
__global__ __launch_bounds__(256) void softmax_rows_kernel(const void *__restrict__ z, int z_f16, int ld_z, int B, int C,
                                                           const float *__restrict__ W, const float *__restrict__ bias,
                                                           const float *__restrict__ V, const float *__restrict__ vbias,
                                                           int K, int ld_w, float *__restrict__ lse,
                                                           float *__restrict__ a) {
  extern __shared__ __align__(16) float lds[];
  constexpr int NSLOT = HV ? 1 : 2;
  float *Zs = lds;
  float *Sp = Zs + kRows * (C + kZPad);
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int r32 = lane & 31, hk = lane >> 5;
  const int rr = tid & 31, cl0 = tid >> 5;
  const int nct = (K + kClasses - 1) / kClasses, ntiles = (B + kRows - 1) / kRows;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int row0 = tile * kRows;
    stage_rows(Zs, z, z_f16, ld_z, row0, B, C, tid);
    __syncthreads();
    float mx = -INFINITY, se = 0.f, st = 0.f;
    for (int ct = 0; ct < nct; ++ct) {
      const int k0 = ct * kClasses;
      int n = k0 + r32;
      if (n >= K) n = K - 1;
      float bk[4], vbk[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {            // (asked for before the MFMAs, used after them)
        const int c = k0 + cl0 + 8 * j;
        bk[j] = c < K ? bias[c] : 0.f;
        vbk[j] = (HV && c < K) ? vbias[c] : 0.f;
      }
      tile_scores<HV>(Zs, Sp, W + (size_t)n * ld_w + 4 * hk, HV ? V + (size_t)n * ld_w + 4 * hk : nullptr, C, lane, wid);
      float sc[4], top = mx;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int cl = cl0 + 8 * j;
        sc[j] = Sp[cl * kRows + rr];
        if (NSLOT == 2) sc[j] += Sp[kRows * kClasses + cl * kRows + rr];
        sc[j] += bk[j];
        if (k0 + cl < K) top = fmaxf(top, sc[j]);
      }
      if (top > mx) {                          // the max moved (always in the first tile): rescale what was summed under the old one
        const float scale = expf(mx - top);   // expf(-inf) = 0 in the first tile, where se = st = 0
        se *= scale, st *= scale, mx = top;
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int cl = cl0 + 8 * j;
        if (k0 + cl < K) {
          const float e = expf(sc[j] - mx);
          se += e;
          if (HV) st += e * (Sp[kRows * kClasses + cl * kRows + rr] + vbk[j]);
        }
      }
      __syncthreads();                         // the next class tile's scores (or the merge) overwrite Sp
    }
    Sp[cl0 * kRows + rr] = mx, Sp[(8 + cl0) * kRows + rr] = se, Sp[(16 + cl0) * kRows + rr] = st;
    __syncthreads();
    if (tid < kRows && row0 + tid < B) {
      float top = Sp[tid];
      for (int q = 1; q < 8; ++q) top = fmaxf(top, Sp[q * kRows + tid]);
      float sum = 0.f, sumt = 0.f;
      for (int q = 0; q < 8; ++q) {
        const float scale = expf(Sp[q * kRows + tid] - top);
        sum += Sp[(8 + q) * kRows + tid] * scale;
        if (HV) sumt += Sp[(16 + q) * kRows + tid] * scale;
      }
      lse[row0 + tid] = top + logf(sum);
      if (HV) a[row0 + tid] = sumt / sum;
    }
    // (the next tile's staging writes Zs only, and a barrier follows it before Sp is written again)
  }
}

// out (+)= the partial sums of walkers 0 .. P-1, in that order.  One thread per (class, column); columns C and C + 1
// of a class are its out_b and out_loss.  ncols: the live columns of a tile (32; a softmax grid pass: 32 / K whole groups),
// so that output k is slot k % ncols of tile k / ncols.
__global__ __launch_bounds__(64) void svm_reduce_kernel(const float *__restrict__ part_W, const float *__restrict__ part_b,
                                                        const float *__restrict__ part_l, int P, int C, int K, int ld_w,
                                                        float *__restrict__ out_W, float *__restrict__ out_b,
                                                        double *__restrict__ out_loss, int accumulate, int ncols) {
  const long long idx = (long long)blockIdx.x * 64 + threadIdx.x;
  if (idx >= (long long)K * (C + 2)) return;
  const int k = (int)(idx / (C + 2)), c = (int)(idx - (long long)k * (C + 2));
  const int ct = k / ncols, i = k - ct * ncols;
  if (c < C) {
    const float sum = ordered_sum<float>(part_W + ((size_t)ct * P * kClasses + i) * C + c, (size_t)kClasses * C, P);
    float *o = out_W + (size_t)k * ld_w + c;
    *o = accumulate ? *o + sum : sum;
  } else if (c == C) {
    const float sum = ordered_sum<float>(part_b + (size_t)ct * P * kClasses + i, kClasses, P);
    out_b[k] = accumulate ? out_b[k] + sum : sum;
  } else if (out_loss) {
    const double sum = ordered_sum<double>(part_l + (size_t)ct * P * kClasses + i, kClasses, P);
    out_loss[k] = accumulate ? out_loss[k] + sum : sum;
  }
}

template <bool HV, int OBJ>
const void *pass_kernel(int C) {
  if (C <= 128) return reinterpret_cast<const void *>(&svm_pass_kernel<HV, 1, OBJ>);
  if (C <= 256) return reinterpret_cast<const void *>(&svm_pass_kernel<HV, 2, OBJ>);
  if (C <= 512) return reinterpret_cast<const void *>(&svm_pass_kernel<HV, 4, OBJ>);
  return reinterpret_cast<const void *>(&svm_pass_kernel<HV, 8, OBJ>);
}

template <int OBJ>
const void *pass_kernel(bool hv, int C) { return hv ? pass_kernel<true, OBJ>(C) : pass_kernel<false, OBJ>(C); }

bool shape_ok(int C, int K) { return cols_ok(C) && K >= 1 && class_tiles(K) <= 65535; }

}  // namespace
}  // namespace lla

using namespace lla;

extern "C" size_t lla_svm_pass_workspace_bytes(int C, int K) {
  if (!shape_ok(C, K)) return 0;
  return (size_t)class_tiles(K) * walkers_max(K) * kClasses * (C + 2) * sizeof(float);
}

namespace {

// The four entry points: the argument checks, (softmax over several class tiles: the row statistics,) the persistent pass
// and the ordered reduction.  obj kHinge: lla_svm_pass; kGrid: `cols`; kSoftmax: `class_weight` (NULL = 1); kSoftGrid: G
// groups of `classes` classes (K = G classes columns), `class_weight` [G][classes], the fold ids and held-out folds in `cols`.
int svm_pass_launch(int obj, const void *z, int z_dtype, int ld_z, const int32_t *y, int B, int C, const float *W,
                    const float *b, const float *V, const float *vb, int K, int ld_w, const GridCols *cols,
                    const float *class_weight, float *out_W, float *out_b, double *out_loss, int accumulate,
                    void *workspace, void *stream, int classes) {
  if (!shape_ok(C, K) || !rows_ok(z, z_dtype, ld_z, B, C) || ld_w < C || (ld_w & 3)) return LLA_EINVAL;
  if (!W || !b || !out_W || !out_b || !workspace || (V && !vb) || (!V && !out_loss) || (B > 0 && !y)) return LLA_EINVAL;
  if (obj == kGrid && (!cols->col_class || !cols->col_held || !cols->col_cpos || !cols->col_cneg)) return LLA_EINVAL;
  if (obj == kSoftGrid && (classes < 1 || classes > kClasses || (cols->fold && !cols->col_held))) return LLA_EINVAL;
  if (((uintptr_t)W & 15) || ((uintptr_t)V & 15) || ((uintptr_t)workspace & 3)) return LLA_EINVAL;
  if (B == 0 && accumulate) return LLA_OK;

  const int ncols = obj == kSoftGrid ? group_tile_cols(classes) : kClasses;      // live columns of a full tile
  const int nct = (K + ncols - 1) / ncols;
  const int ntiles = (B + kRows - 1) / kRows;
  const int pmax = tile_walkers(nct);
  const int P = ntiles < pmax ? ntiles : pmax;
  float *part_W = static_cast<float *>(workspace);
  float *part_b = part_W + (size_t)nct * pmax * kClasses * C;
  float *part_l = part_b + (size_t)nct * pmax * kClasses;
  hipStream_t st = as_stream(stream);
  if (P > 0) {
    const void *kernel = obj == kSoftGrid ? pass_kernel<kSoftGrid>(V != nullptr, C)
                         : obj == kSoftmax ? pass_kernel<kSoftmax>(V != nullptr, C)
                         : obj == kGrid    ? pass_kernel<kGrid>(V != nullptr, C) : pass_kernel<kHinge>(V != nullptr, C);
    const size_t lds_bytes = (size_t)lds_floats(C, obj == kSoftmax || obj == kSoftGrid) * sizeof(float);
    if (lds_bytes > dynamic_lds_limit(kernel)) return LLA_ECAP;
    const int z_f16 = z_dtype == LLA_Z_F16;
    GridCols gc = cols ? *cols : GridCols{nullptr, nullptr, nullptr, nullptr, nullptr};
    SoftmaxRows sm = {class_weight, nullptr, nullptr, classes};
    if (obj == kSoftmax && nct > 1) {          // lse [B], a [B] behind the partial sums
      float *lse = part_l + (size_t)nct * pmax * kClasses, *a = lse + B;
      const void *rows_kernel = V ? reinterpret_cast<const void *>(&softmax_rows_kernel<true>)
                                  : reinterpret_cast<const void *>(&softmax_rows_kernel<false>);
      const size_t rows_lds = (size_t)lds_floats(C) * sizeof(float);
      if (rows_lds > dynamic_lds_limit(rows_kernel)) return LLA_ECAP;
      void *rows_args[] = {(void *)&z, (void *)&z_f16, (void *)&ld_z, (void *)&B, (void *)&C, (void *)&W, (void *)&b,
                           (void *)&V, (void *)&vb, (void *)&K, (void *)&ld_w, (void *)&lse, (void *)&a};
      hipError_t e = hipLaunchKernel(rows_kernel, dim3(ntiles < kResident ? ntiles : kResident), dim3(256), rows_args,
                                     rows_lds, st);
      if (e != hipSuccess) return hip_fail(e);
      sm.lse = lse, sm.a = a;
    }
    void *args[] = {(void *)&z, (void *)&z_f16, (void *)&ld_z, (void *)&y, (void *)&B, (void *)&C, (void *)&W, (void *)&b,
                    (void *)&V, (void *)&vb, (void *)&K, (void *)&ld_w, (void *)&part_W, (void *)&part_b, (void *)&part_l,
                    (void *)&gc, (void *)&sm};
    hipError_t e = hipLaunchKernel(kernel, dim3(P, nct), dim3(256), args, lds_bytes, st);
    if (e != hipSuccess) return hip_fail(e);
  }
  const long long n_out = (long long)K * (C + 2);
  svm_reduce_kernel<<<(unsigned)((n_out + 63) / 64), 64, 0, st>>>(part_W, part_b, part_l, P, C, K, ld_w, out_W, out_b,
                                                                     V ? nullptr : out_loss, accumulate, ncols);
  return check_launch();
}

}  // namespace

extern "C" int lla_svm_pass(const void *z, int z_dtype, int ld_z, const int32_t *y, int B, int C, const float *W,
                            const float *b, const float *V, const float *vb, int K, int ld_w, float *out_W, float *out_b,
                            double *out_loss, int accumulate, void *workspace, void *stream) {
  return svm_pass_launch(kHinge, z, z_dtype, ld_z, y, B, C, W, b, V, vb, K, ld_w, nullptr, nullptr, out_W, out_b, out_loss,
                         accumulate, workspace, stream, 0);
}

// The grid is the one lla_svm_pass launches for K = J: a function of (B, J) alone.
extern "C" size_t lla_svm_grid_pass_workspace_bytes(int C, int J) { return lla_svm_pass_workspace_bytes(C, J); }

extern "C" int lla_svm_grid_pass(const void *z, int z_dtype, int ld_z, const int32_t *y, const int32_t *fold, int B, int C,
                                 const float *W, const float *b, const float *V, const float *vb, int J, int ld_w,
                                 const int32_t *col_class, const int32_t *col_held, const float *col_cpos,
                                 const float *col_cneg, float *out_W, float *out_b, double *out_loss, int accumulate,
                                 void *workspace, void *stream) {
  const GridCols cols = {fold, col_class, col_held, col_cpos, col_cneg};
  return svm_pass_launch(kGrid, z, z_dtype, ld_z, y, B, C, W, b, V, vb, J, ld_w, &cols, nullptr, out_W, out_b, out_loss,
                         accumulate, workspace, stream, 0);
}

// The partial sums of lla_svm_pass, then lse [B] and a [B] when the classes span more than one tile.
extern "C" size_t lla_softmax_pass_workspace_bytes(int C, int K, int B) {
  if (!shape_ok(C, K) || B < 0) return 0;
  return lla_svm_pass_workspace_bytes(C, K) + (class_tiles(K) > 1 ? 2 * (size_t)B * sizeof(float) : 0);
}

extern "C" int lla_softmax_pass(const void *z, int z_dtype, int ld_z, const int32_t *y, int B, int C, const float *W,
                                const float *b, const float *V, const float *vb, int K, int ld_w, const float *class_weight,
                                float *out_W, float *out_b, double *out_loss, int accumulate, void *workspace, void *stream) {
  return svm_pass_launch(kSoftmax, z, z_dtype, ld_z, y, B, C, W, b, V, vb, K, ld_w, nullptr, class_weight, out_W, out_b,
                         out_loss, accumulate, workspace, stream, 0);
}

// The partial sums of ceil(G / (32 / K)) tiles: the grid is a function of (B, K, G) alone.
extern "C" size_t lla_softmax_grid_pass_workspace_bytes(int C, int K, int G) {
  if (K < 1 || K > kClasses || G < 1 || !shape_ok(C, K) || group_tiles(K, G) > 65535) return 0;
  const int nct = (int)group_tiles(K, G);
  return (size_t)nct * tile_walkers(nct) * kClasses * (C + 2) * sizeof(float);
}

extern "C" int lla_softmax_grid_pass(const void *z, int z_dtype, int ld_z, const int32_t *y, const int32_t *fold, int B, int C,
                                     const float *W, const float *b, const float *V, const float *vb, int K, int G, int ld_w,
                                     const int32_t *group_held, const float *group_class_weight, float *out_W, float *out_b,
                                     double *out_loss, int accumulate, void *workspace, void *stream) {
  if (K < 1 || K > kClasses || G < 1 || group_tiles(K, G) > 65535) return LLA_EINVAL;
  const GridCols cols = {fold, nullptr, group_held, nullptr, nullptr};
  return svm_pass_launch(kSoftGrid, z, z_dtype, ld_z, y, B, C, W, b, V, vb, G * K, ld_w, &cols, group_class_weight, out_W,
                         out_b, out_loss, accumulate, workspace, stream, K);
}
