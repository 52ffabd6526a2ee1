// Which GEMM kernel takes which shape, on how many workgroups: the ONE statement of the selection.  Plain host C++ (no HIP, no
// environment): the product's launchers (gemm_pp.hip, gemm_q4.hip, gemm_w8.hip) call it with GemmKnobs{}, the tools/ builds'
// (ablation/gemm_*select.hip) with the A/B switches filled in, tower.hip asks q4_takes() where LayerNorm may ride in a residual
// GEMM, and lla_gemm_plan() shows the answers to tests/test_host.py.
//
// Stands in for the Linear / conv1 layers inside `z = self.clip(X)` (hub/compressor.py:93) and the 1x1 / 3x3 convolutions of
// the RN50-CLIP tower (lossyless/architectures.py:367-371).  With GemmKnobs{}:
//   M >= kBigM rows (batches of ~190+ images):
//     fp16-output layers (QKV, c_fc), N % 256 == 0, K >= 128 ........ gemm_w8_kernel   (eight waves, 16x16x32 MFMA; ragged M too)
//     residual layers (out-proj, c_proj), M % 256 == 0, K >= 256 .... gemm_q4_kernel   (four waves; the tower calls
//                                                                     launch_q4(EPI_RESID_LNX) itself where LayerNorm rides along)
//     everything else 256 columns wide (patch embedding, ragged M) .. gemm_pp_kernel   (two wave rows out of phase)
//     narrower outputs ............................................... gemm_persistent_kernel
//     ReLU / add + ReLU 1x1 convolutions, N % 256 == 0 ............... gemm_persistent_kernel (line-assembling epilogue)
//   kSmallM < M < kBigM, and every implicit 3x3 convolution ......... gemm256_f16_kernel (one 256 x 128 tile per workgroup)
//   M <= kSmallM ...................................................... gemm_f16_kernel    (one 128 x 128 tile per workgroup)
// All of them accumulate K in the same order: an output does not depend on the kernel that computed it.
#pragma once
#include <cstddef>

#include "../../include/lossyless_amd.h"

// compile-time policies of the four-wave kernel that its gate and grid follow (gemm_q4_kernel.h; `make variant DEFS=...`)
#ifndef LLA_Q4_BUFDMA
#define LLA_Q4_BUFDMA 1     // operand panels through buffer descriptors: 32-bit byte offsets from the operands' bases
#endif
#ifndef LLA_LNX_TRIPLES
#define LLA_LNX_TRIPLES 1   // EPI_RESID_LNX walks triples of column tiles laid out for 8 x 32 workgroups
#endif

namespace lla {

constexpr int kWidth = 768, kLayers = 12, kHeadDim = 64, kTokens = 50;  // 12 heads
constexpr int kPatches = 49, kPatchK = 3072, kMlp = 3072, kOut = 512;
constexpr int BM = 128, BN = 128, BK = 64;
constexpr int BM2 = 256, BN2 = 128;   // gemm256_f16_kernel's tile (gemm_kernels.h; lla_conv3x3_relu_f16 checks its shapes against it)

enum { EPI_F16 = 0, EPI_QGELU = 1, EPI_RESID = 2, EPI_PATCH = 3, EPI_RELU = 4, EPI_ADDRELU = 5,
       // (6 .. 8: the algebraic LayerNorm fusion of round 3, retired in round 6: docs/history/DESIGN_rounds_1-5.md 5.4)
       // round 5: EPI_RESID whose epilogue ALSO applies the LayerNorm that follows the residual add (ln_2 after out-proj,
       // ln_1 of the next block after c_proj) to its own 256 x 256 chunk of x and writes it as fp16: the three column
       // tiles of a row tile exchange exact per-row partial sums through memory (GemmParams::lnx_*, gemm_q4.hip)
       EPI_RESID_LNX = 9 };
constexpr int epi_base(int e) { return e == EPI_RESID_LNX ? EPI_RESID : e; }   // the epilogue family of a kernel instantiation
enum { A_PLAIN = 0, A_PATCH_NHWC = 1, A_PATCH_NCHW = 2, A_CONV3 = 3 };

// Small problems (< ~9k rows: batches under ~190 images) do not fill 256 persistent workgroups with 256-wide tiles; measured
// at batch 128: 40.6k img/s persistent vs 48.4k with the one-tile-per-workgroup 256 x 128 kernel.
constexpr int kBigM = 9000;
constexpr int kSmallM = 128;     // up to here a single row of 128 x 128 tiles
constexpr int kWideMinN = 768;   // narrowest output that gets 256-column persistent tiles (three column tiles)
constexpr int kPpMinK = 256;     // the ping-pong kernel's K loop needs something to overlap
constexpr int kXcds = 8;

struct GemmShape { int epi, amode, M, N, K, lda, ldc, n_store, a_chunk_images; };

// The A/B switches that influence the CHOICE (tools/ builds: ablation/gemm_select.hip reads them from the environment).  The
// default member initialisers are the product: GemmKnobs{} IS the product's selection.
struct GemmKnobs {
  int tile = 1;             // LLA_GEMM_TILE: 128 / 256 = that one-tile-per-workgroup kernel instead of the persistent ones
  int pp = 1;               // LLA_GEMM_PP: 0 = lock-step persistent kernel instead of the ping-pong kernel
  int q4 = 1;               // LLA_GEMM_Q4: 0 = no four-wave kernel
  int w8 = 1;               // LLA_GEMM_W8: 0 = no eight-wave kernel (its layers go to the four-wave one), 2 = at every M
  int tall = 1;             // LLA_GEMM_TALL: 0 = 256-row tiles only
  bool balanced = true;     // LLA_GEMM_BALANCED: 0 = the ping-pong kernel on min(tiles, CUs) workgroups
  int persist = 1;          // LLA_GEMM_PERSIST: 0 = the lock-step kernel with one workgroup per tile
  int kb = 64;              // LLA_GEMM_KB: 32 = K-tiles of 32 (256-row tiles only)
  int wide_min_n = kWideMinN;   // LLA_GEMM_WIDE_MIN_N
  int rn_persist = 2;       // LLA_RN_PERSIST: ReLU convolutions 0 = one tile per workgroup, 1 = 128-wide persistent, 3 = ping-pong
};

enum GemmKernel { GK_NONE = 0, GK_TILE128 = 1 /* gemm_f16_kernel */, GK_TILE256 = 2 /* gemm256_f16_kernel */,
                  GK_PERSIST1 = 3, GK_PERSIST2 = 4 /* gemm_persistent_kernel, NJ = 1 / 2 */, GK_PP = 5, GK_Q4 = 6, GK_W8 = 7 };
struct GemmPlan { int status; GemmKernel kernel; int tile_rows, grid; };   // (LLA_OK + GK_NONE: nothing to launch)

inline int ceil_div(int a, int b) { return (a + b - 1) / b; }
// Rounds a persistent grid needs for `tiles` work items (the slowest workgroup's tile count).
inline int rounds_for(int tiles, int cus) { return ceil_div(tiles, cus); }

// Persistent grid.  Balanced: the launch lasts rounds_for(total, cus) tiles per workgroup whatever happens, so only as many
// workgroups as that round count needs are started (rounded up to a multiple of the 8 XCDs): 51 200 rows -> 1440 / 1920 / 480
// tiles = exactly 6 / 8 / 2 rounds on 240 workgroups, against 5.625 / 7.5 / 1.875 (same duration) on 256.
inline int balanced_grid(int total, int cus, bool balanced = true) {
  int grid = total < cus ? total : cus;
  if (balanced && total > cus) {
    const int need = (ceil_div(total, rounds_for(total, cus)) + kXcds - 1) & ~(kXcds - 1);
    if (need < grid) grid = need;
  }
  return grid;
}

// 320-row tiles instead of 256-row ones when that shortens the critical path (cost ~ rounds x rows; on a tie the taller tile
// wins: 10 % fewer operand bytes per flop).
inline bool tall_tiles(int M, int tiles_n, int cus, bool allowed) {
  return allowed && rounds_for(ceil_div(M, 320) * tiles_n, cus) * 320 <= rounds_for(ceil_div(M, 256) * tiles_n, cus) * 256;
}

// columns >= n_store are computed but not stored (GemmParams::n_store; 0: all)
inline int stored_columns(int n_store, int N) { return n_store <= 0 || n_store > N ? N : n_store; }

// 32-bit byte offsets of the four- / eight-wave kernels: inside a tile's operand panel and, `from_bases`, of the panels from the
// operands' bases (the buffer descriptor's scalar offset)
inline bool panel_offsets_fit(const GemmShape &s, bool from_bases) {
  if ((size_t)256 * (size_t)s.lda * 2 >= (1ull << 31) || (size_t)256 * (size_t)s.K * 2 >= (1ull << 31)) return false;
  return !from_bases || ((size_t)s.M * (size_t)s.lda * 2 < (1ull << 32) && (size_t)s.N * (size_t)s.K * 2 < (1ull << 32));
}

// gemm_w8_kernel: A_PLAIN operands, fp16 outputs, every M (a ragged last row tile is stored masked)
inline bool w8_takes(const GemmShape &s) {
  return s.amode == A_PLAIN && (s.epi == EPI_F16 || s.epi == EPI_QGELU) && s.M > 0 && !(s.N & 255) && s.N <= 3072 && !(s.K & 63) &&
         s.K >= 128 && s.lda >= s.K && !(s.lda & 7) && s.ldc >= s.N && !(s.ldc & 7) && panel_offsets_fit(s, true);
}
inline int w8_grid(const GemmShape &s, int cus) { return balanced_grid(ceil_div(s.M, 256) * (s.N / 256), cus); }

// gemm_q4_kernel: A_PLAIN operands, whole 256-row tiles only; EPI_RESID_LNX exchanges a row's sums among its three column tiles
// (and, like every fp32 epilogue, addresses C with 32-bit element offsets: plan_gemm asks the same of EPI_RESID before it
// comes here; a tower slice is far below it, lla_gemm_resid_layernorm768 takes any M)
inline bool q4_takes(const GemmShape &s) {
  const bool epi_ok = s.epi == EPI_F16 || s.epi == EPI_QGELU || s.epi == EPI_RESID ||
                      (s.epi == EPI_RESID_LNX && s.N == kWidth && s.ldc == kWidth && (size_t)s.M * (size_t)kWidth < (1ull << 32));
  return s.amode == A_PLAIN && epi_ok && s.M > 0 && !(s.M & 255) && !(s.N & 255) && s.N <= 3072 && !(s.K & 63) && s.K >= kPpMinK &&
         s.lda >= s.K && !(s.lda & 7) && panel_offsets_fit(s, LLA_Q4_BUFDMA);
}
inline int q4_grid(const GemmShape &s, int cus) {
  const int total = (s.M / 256) * (s.N / 256);
  // (the triple walk of EPI_RESID_LNX is laid out for 8 x 32 workgroups: same number of rounds as the balanced grid --
  // ceil(row tiles / 85) against ceil(3 row tiles / 256) --, no row tile split over two rounds)
  if (LLA_LNX_TRIPLES && s.epi == EPI_RESID_LNX && cus == 256 && total > cus) return 256;
  return balanced_grid(total, cus);
}

inline GemmPlan plan_gemm(GemmShape s, int cus, const GemmKnobs &k = GemmKnobs{}) {
  const GemmPlan refuse{LLA_EINVAL, GK_NONE, 0, 0};
  if (s.M <= 0) return {LLA_OK, GK_NONE, 0, 0};
  if (s.N % BN || s.K % BK) return refuse;
  const bool plain = s.amode == A_PLAIN, patch = s.amode == A_PATCH_NHWC || s.amode == A_PATCH_NCHW, conv3 = s.amode == A_CONV3;
  const bool relu = s.epi == EPI_RELU || s.epi == EPI_ADDRELU, fp16_out = s.epi == EPI_F16 || s.epi == EPI_QGELU;
  if (s.epi == EPI_RESID_LNX) return q4_takes(s) ? GemmPlan{LLA_OK, GK_Q4, 256, q4_grid(s, cus)} : refuse;
  if (!(plain && (fp16_out || relu || s.epi == EPI_RESID)) && !(patch && s.epi == EPI_PATCH) && !(conv3 && s.epi == EPI_RELU)) return refuse;
  const bool big = s.M >= kBigM;
  const bool pp_shape = s.N % 256 == 0 && s.N >= kWideMinN && s.K >= kPpMinK;   // at least three column tiles, K loop worth overlapping
  // (the image batch in pieces: patch embedding of a chip-filling pass, on the ping-pong kernel's 256-row tiles only)
  if (s.a_chunk_images && (!patch || (s.a_chunk_images & 255) || !big || k.tile != 1 || !k.pp || !pp_shape)) return refuse;
  s.n_store = stored_columns(s.n_store, s.N);
  // the fp32 epilogues address C with 32-bit element offsets (registers are scarce there)
  if ((s.epi == EPI_RESID || s.epi == EPI_PATCH) && ((size_t)s.M + (size_t)s.M / kPatches + 2) * (size_t)s.ldc >= (1ull << 32)) return refuse;

  // The 256-column persistent kernels finish fp16 outputs with ONE 16-byte store per lane at C + m ldc + 8 q (gemm_epilogue_staged,
  // gemm_epilogue_swap: gemm_common.h): with ldc % 8 == 4 every other row would sit 8 bytes off that store's alignment.  Nothing
  // here relies on what the memory pipeline does with such a store -- the towers pass multiples of 32 --, so the shape is refused
  // (the one-tile kernels and the 128-column persistent kernel store 8 bytes per lane and keep taking ldc % 4 == 0).
  const bool lines_ok = !(fp16_out || relu) || !(s.ldc & 7);

  auto one_tile = [&](GemmKernel kernel, int rows) { return GemmPlan{LLA_OK, kernel, rows, ceil_div(s.M, rows) * (s.N / 128)}; };
  auto ping_pong = [&] {
    if (!lines_ok) return refuse;
    const int tiles_n = s.N / 256, rows = tall_tiles(s.M, tiles_n, cus, k.tall && !s.a_chunk_images) ? 320 : 256;
    return GemmPlan{LLA_OK, GK_PP, rows, balanced_grid(ceil_div(s.M, rows) * tiles_n, cus, k.balanced)};
  };
  auto lock_step = [&](int nj) {   // (N / (128 nj) column tiles; 320 rows exist for nj = 2, K-tiles of 64)
    if (nj == 2 && !lines_ok) return refuse;
    const int tiles_n = s.N / (128 * nj), rows = tall_tiles(s.M, tiles_n, cus, k.tall && nj == 2 && k.kb == 64) ? 320 : 256;
    const int total = ceil_div(s.M, rows) * tiles_n;
    return GemmPlan{LLA_OK, nj == 2 ? GK_PERSIST2 : GK_PERSIST1, rows, k.persist ? balanced_grid(total, cus, false) : total};
  };

  if (relu) {
    // ResNet-tower GEMMs.  1x1 convolutions whose output is a multiple of 256 channels wide run on
    // the persistent 256-wide kernel with the line-assembling epilogue (whole 128-byte lines instead of 16-byte pieces per
    // row took the add + ReLU convolution of layer1 from 3.2 to 5.3 TB/s); narrow outputs and the implicit 3x3
    // convolutions stay on the one-tile-per-workgroup kernels.
    const bool whole = plain && big && s.N % 256 == 0 && s.n_store == s.N;
    if (k.rn_persist >= 3 && whole && pp_shape) return ping_pong();
    if (k.rn_persist >= 2 && whole) return lock_step(2);
    if (k.rn_persist == 1 && plain && big) return lock_step(1);
    return s.M > kSmallM || conv3 ? one_tile(GK_TILE256, 256) : one_tile(GK_TILE128, 128);
  }
  if (plain && fp16_out && k.w8 && (big || k.w8 == 2) && s.n_store == s.N && w8_takes(s)) return {LLA_OK, GK_W8, 256, w8_grid(s, cus)};
  if (k.tile == 1 && !big && s.M > kSmallM) return one_tile(GK_TILE256, 256);
  // (the four-wave kernel's fp16 epilogues exist only where the eight-wave kernel, which takes every shape they take, is off)
  if (plain && (s.epi == EPI_RESID || (fp16_out && !k.w8)) && k.q4 && big && s.ldc == s.N && q4_takes(s))
    return {LLA_OK, GK_Q4, 256, q4_grid(s, cus)};
  if (k.tile == 1 && s.M > kSmallM) {
    if (k.pp && pp_shape) return ping_pong();
    return lock_step(s.N % 256 == 0 && s.N >= k.wide_min_n ? 2 : 1);
  }
  return k.tile == 256 && s.M > kSmallM ? one_tile(GK_TILE256, 256) : one_tile(GK_TILE128, 128);
}

}  // namespace lla
