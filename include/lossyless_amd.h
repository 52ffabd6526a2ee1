/*
 * lossyless_amd.h -- C ABI of liblossyless_amd.so (MI355X / gfx950).
 *
 * Drop-in boundary for the compress_dataset hot path of YannDubs/lossyless
 * (hub/compressor.py).  The reference reaches native code for this path through
 * three pybind11 entry points of compressai==1.1.5 and through torch/cuDNN for the
 * CLIP tower; each function below names the reference interface it stands in for.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no C++ / torch types.
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream).  Device
 *     entry points only enqueue work; they never synchronise.
 *   - every function returns LLA_OK (0) or a negative LLA_E* code; nothing throws.
 *   - pointers marked [dev] are device pointers, [host] host pointers.
 *   - no global state; re-entrant; caller owns all buffers.  The only state a call may leave behind lives in
 *     handles the caller creates and destroys (lla_tower_*, lla_profiler_*); a handle is used from one host
 *     thread at a time.  (One process-wide cache exists and is guarded: per-device kernel attributes, set once.
 *     The product library reads no environment variable: csrc/switches.h.)
 *
 * Table layout (same as compressai's EntropyModel buffers after update(),
 * hub/compressor.py:56-63):
 *   cdf      int32 [C][W]   row c holds cdf_len[c] valid entries, 0 .. 65536
 *   cdf_len  int32 [C]      = pmf_length + 2
 *   offset   int32 [C]      = -minima
 * Escape symbol of channel c is index cdf_len[c]-2.
 *
 * Domain: |symbol - offset| < 2^30 (the reference's int32 arithmetic is undefined
 * beyond that, rans_interface.cpp encode_with_indexes).
 */
#ifndef LOSSYLESS_AMD_H
#define LOSSYLESS_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LLA_OK 0
#define LLA_EINVAL (-1) /* bad argument (null pointer, size, alignment)        */
#define LLA_ECAP (-2)   /* caller buffer too small                             */
#define LLA_EHIP (-3)   /* HIP runtime reported an error (see lla_last_hip_error) */
#define LLA_EDATA (-4)  /* malformed input (e.g. pmf without a donor frequency) */

/* v4 (round 6): + lla_source_sha(); enum lla_vit_param lost its six LayerNorm-folded weight entries (the blob of
 * lla_vit_b32_weights_bytes() is 99 MB smaller): the algebraic LayerNorm fusion of round 3 they fed was retired. */
#define LLA_ABI_VERSION 4

/* ABI version of the loaded library. */
int lla_abi_version(void);
/* sha256 (first 16 hex digits) over the kernel sources this library was built from (the .hip / .h / .cpp files of csrc + this
 * header; lossyless_amd/csrc/source_sha.py).  The Python host recomputes it from the tree and refuses a stale build. */
const char *lla_source_sha(void);
/* hipError_t of the most recent failing HIP call on this thread (0 if none). */
int lla_last_hip_error(void);

/* ------------------------------------------------------------------------- *
 * Host entry points
 * ------------------------------------------------------------------------- */

/* Replaces compressai._CXX.pmf_to_quantized_cdf(pmf: list[float], precision) ->
 * list[int]  (cpp_exts/ops/ops.cpp), reached from EntropyBottleneck.update(),
 * hub/compressor.py:63; lossyless/rates.py:299.
 * pmf [host] n floats; cdf_out [host] n+1 entries. */
int lla_pmf_to_quantized_cdf(const float *pmf, int n, int precision, uint32_t *cdf_out);

/* Walks the reference's container (hub/compressor.py:233-237: big-endian u32 N, then
 * N x {big-endian u32 len, len bytes}) held in host memory and writes the byte
 * offset of every record, relative to blob + 4, into off[0..N] (off[N] = body size),
 * i.e. exactly the `off` / record_prefix=1 input of lla_rans_decode_batch for the
 * body blob + 4.  *n_out receives N.  off may be NULL to only query N.
 * Returns LLA_EDATA when a record runs past nbytes or when N records cannot fit in nbytes at all
 * (checked even with off == NULL, so a corrupt count never sizes an allocation), LLA_ECAP when
 * off_cap < N+1. */
int lla_container_index(const uint8_t *blob, size_t nbytes, uint64_t *off, size_t off_cap,
                        uint32_t *n_out);

/* Host coder: the batch forms of
 *   ans.RansEncoder().encode_with_indexes(symbols, indexes, cdfs, cdfs_sizes, offsets) -> bytes
 *   ans.RansDecoder().decode_with_indexes(encoded, indexes, cdfs, cdfs_sizes, offsets) -> list[int]
 * (compressai cpp_exts/rans/rans_interface.cpp) with indexes[i] = i, on HOST pointers, threaded
 * over images.  They serve the reference's default decompress_dataset(is_cpu=True)
 * (hub/compressor.py:227-229,236-238: module moved to the CPU, one decode per image) on a box
 * without a GPU, and give CPU-side tools the same bytes as the device kernels.
 *   encode: symbols [host] B*C; out receives the streams back to back (record_prefix = 1: each
 *           preceded by its big-endian u32 length = the container body, hub/compressor.py:192-196);
 *           out_off [host] B+1 byte offsets, out_off[B] = total.  LLA_ECAP if total > cap (out_off
 *           is filled in that case too, so the caller can size `out` and call again).
 *   decode: payload/off/record_prefix/status exactly as lla_rans_decode_batch, host pointers. */
int lla_rans_encode_batch_host(const int32_t *symbols, int B, int C, const int32_t *cdf, int W,
                               const int32_t *cdf_len, const int32_t *offset, int record_prefix,
                               uint8_t *out, size_t cap, uint64_t *out_off);
int lla_rans_decode_batch_host(const uint8_t *payload, const uint64_t *off, int record_prefix, int B,
                               int C, const int32_t *cdf, int W, const int32_t *cdf_len,
                               const int32_t *offset, int32_t *symbols_out, int32_t *status);
/* Host twin of lla_dequantise (same fp32 operations, same values). */
int lla_dequantise_host(const int32_t *symbols, int B, int C, const float *bias,
                        const float *exp_scale, const float *median, float *z_hat);

/* Upper bound on the bytes one image's stream can occupy (C symbols, all
 * escaped with 8 payload digits).  Use it as the per-image scratch stride. */
size_t lla_rans_max_encoded_bytes(int C);

/* ------------------------------------------------------------------------- *
 * Device entry points: entropy stage (A4, A5, A13, A14, A15)
 * ------------------------------------------------------------------------- */

/* z dtype selector for the fused entry points */
#define LLA_Z_F16 1
#define LLA_Z_F32 2

/* process_z_in + quantise (hub/compressor.py:105-109 then EntropyModel.quantize
 * "symbols"): sym = int(rint((float(z) + bias) * exp_scale - median)), every
 * operation rounded to fp32 on its own.
 * z [dev] B*C of z_dtype; bias/exp_scale/median [dev] C floats; symbols [dev] B*C. */
int lla_quantise(const void *z, int z_dtype, int B, int C, const float *bias,
                 const float *exp_scale, const float *median, int32_t *symbols, void *stream);

/* Replaces ans.RansEncoder().encode_with_indexes(symbols, indexes, cdfs,
 * cdfs_sizes, offsets) -> bytes  (cpp_exts/rans/rans_interface.cpp), called once
 * per image by EntropyModel.compress <- hub/compressor.py:98; lossyless/rates.py:559.
 * Here: B images per call, indexes[i] = i.
 * Image b's stream is written END-ALIGNED into scratch + b*stride, i.e. it
 * occupies [b*stride + stride - lengths[b], b*stride + stride).
 * stride must be >= lla_rans_max_encoded_bytes(C) and a multiple of 4. */
int lla_rans_encode_batch(const int32_t *symbols, int B, int C, const int32_t *cdf, int W,
                          const int32_t *cdf_len, const int32_t *offset, uint8_t *scratch,
                          size_t stride, uint32_t *lengths, void *stream);

/* Fused lla_quantise + lla_rans_encode_batch: z never leaves the device as
 * symbols.  symbols_out [dev] may be NULL. */
int lla_quantise_encode(const void *z, int z_dtype, int B, int C, const float *bias,
                        const float *exp_scale, const float *median, const int32_t *cdf, int W,
                        const int32_t *cdf_len, const int32_t *offset, uint8_t *scratch,
                        size_t stride, uint32_t *lengths, int32_t *symbols_out, void *stream);

/* Workspace bytes lla_rans_compact needs for B images. */
size_t lla_rans_compact_workspace_bytes(int B);

/* Packs the end-aligned streams back to back.
 *   record_prefix = 0: out = s_0 s_1 ... ;            out_off[b] = sum_{k<b} len_k
 *   record_prefix = 1: out = be32(len_0) s_0 be32(len_1) s_1 ... which is the body
 *       of the reference's container after its 4-byte count
 *       (hub/compressor.py:192-196);                  out_off[b] = sum_{k<b} (len_k + 4)
 * out_off [dev] B+1 entries, out_off[B] = total bytes.  The caller sizes `out`
 * for the worst case (B*(stride+4)) or reads lengths first; bytes beyond cap are
 * not written and *out_off[B] still reports the needed size. */
int lla_rans_compact(const uint8_t *scratch, size_t stride, const uint32_t *lengths, int B,
                     int record_prefix, uint8_t *out, size_t cap, uint64_t *out_off,
                     void *workspace, size_t workspace_bytes, void *stream);

/* Two sets of end-aligned streams (a = z, b = side information of the scale hyperprior) packed into ONE body of
 * interleaved length-prefixed records:
 *   out = be32(len a_0) a_0 be32(len b_0) b_0 be32(len a_1) a_1 ...
 * i.e. the reference's container body (hub/compressor.py:192-196) with two records per image, which is what a
 * dataset coded by HRateHyperprior.compress (lossyless/rates.py:701-713: [z_strings, side_z_strings]) holds.
 * out_off [dev] 2B+1 entries (record r starts at out_off[r]; out_off[2B] = total bytes).  cap and overrun as in
 * lla_rans_compact: records that would end beyond cap are not written, out_off still reports the needed size.
 * workspace [dev] 8-byte aligned, lla_rans_compact_pairs_workspace_bytes(B) bytes.  LLA_EINVAL for B >= 2^30 (the
 * 2B records are counted in an int). */
size_t lla_rans_compact_pairs_workspace_bytes(int B);
int lla_rans_compact_pairs(const uint8_t *scratch_a, size_t stride_a, const uint32_t *lengths_a,
                           const uint8_t *scratch_b, size_t stride_b, const uint32_t *lengths_b, int B,
                           uint8_t *out, size_t cap, uint64_t *out_off, void *workspace,
                           size_t workspace_bytes, void *stream);

/* Replaces ans.RansDecoder().decode_with_indexes(encoded, indexes, cdfs,
 * cdfs_sizes, offsets) -> list[int], called per image by EntropyModel.decompress
 * <- hub/compressor.py:124,238; lossyless/rates.py:563.
 * payload [dev]; image b's stream is payload[off[b] + skip .. off[b+1]) where
 * skip = 4 when record_prefix (the be32 length is stepped over).  Streams must
 * start 4-byte aligned.  status [dev] B ints: 0 ok, 1 stream overrun. */
int lla_rans_decode_batch(const uint8_t *payload, const uint64_t *off, int record_prefix, int B,
                          int C, const int32_t *cdf, int W, const int32_t *cdf_len,
                          const int32_t *offset, int32_t *symbols_out, int32_t *status,
                          void *stream);

/* lla_rans_decode_batch over every off_step-th record: image b's stream is
 * payload[off[off_first + b*off_step] + skip .. off[off_first + b*off_step + 1]).  off_first = 1, off_step = 2 reads the
 * side-information records of a body written by lla_rans_compact_pairs.  lla_rans_decode_batch is off_first = 0,
 * off_step = 1. */
int lla_rans_decode_batch_strided(const uint8_t *payload, const uint64_t *off, int record_prefix,
                                  int off_first, int off_step, int B, int C, const int32_t *cdf, int W,
                                  const int32_t *cdf_len, const int32_t *offset, int32_t *symbols_out,
                                  int32_t *status, void *stream);

/* Random access into a container body: decode + dequantise the records a caller NAMES, in the order it names them.
 * Extends the reference's decompress_dataset (hub/compressor.py:209-254: read every record of the file in order, one
 * decode per image, stack on the host) to what a downstream trainer draws from a compressed dataset -- a shuffled
 * minibatch, on the device, from a body that stays compressed in device memory.
 * payload / off (N+1 entries) / record_prefix and the tables exactly as in lla_rans_decode_batch; index [dev] B int64.
 * Output row b, at z_hat + b*ld_out ELEMENTS (ld_out >= C), is record index[b] dequantised:
 *   (float(sym) + median) / exp_scale - bias, fp32 per operation  (lla_dequantise; hub/compressor.py:111-115)
 * z_dtype LLA_Z_F32: bit-equal to lla_rans_decode_batch + lla_dequantise; LLA_Z_F16: that value rounded to nearest
 * even.  Columns C .. ld_out-1 of a row are never written.  Symbols never reach global memory.
 * status [dev] B ints: 0 decoded; 1 stream overrun or unopenable (row zeroed); 2 index[b] outside [0, N) (nothing
 * read for it, row zeroed).  Repeated indices are legal.  B == 0: LLA_OK, no launch. */
int lla_rans_decode_gather(const uint8_t *payload, const uint64_t *off, int record_prefix, int N,
                           const int64_t *index, int B, int C, const int32_t *cdf, int W,
                           const int32_t *cdf_len, const int32_t *offset, const float *bias,
                           const float *exp_scale, const float *median, void *z_hat, int z_dtype,
                           size_t ld_out, int32_t *status, void *stream);
/* lla_rans_decode_gather over every off_step-th record of an interleaved body: output row b is record
 * off_first + index[b]*off_step of `off`, N is the number of IMAGES (index[b] in [0, N)), and `off` holds at least
 * off_first + (N-1)*off_step + 2 entries.  The record number is computed in 64 bits and checked before anything is
 * read.  lla_rans_decode_gather is off_first = 0, off_step = 1 of the same kernel.  off_first = 1, off_step = 2 walks
 * the side records of a body written by lla_rans_compact_pairs, i.e. the first half of lossyless/rates.py:715-724
 * (get_indexes_means_hat: EntropyBottleneck.decompress of the side strings) for the images a caller names.
 * With a zero bias, a unit exp_scale and the bottleneck's medians the value written is
 *   (float(sym) + median) / 1 - 0  ==  float(sym) + median      exactly: x / 1 and x - 0 round to x,
 * which is s_hat; with ld_out = the padded K of z_encoder's first layer it lands in the zero-padded fp32 A matrix of
 * that layer's lla_gemm_f32 (columns C .. ld_out-1 are never written and keep their zeros): no int32 symbols, no
 * conversion pass, no padding copy.  HyperpriorLatents (lossyless_amd/latents.py) depends on that equality.
 * LLA_EINVAL for off_first < 0 or off_step < 1. */
int lla_rans_decode_gather_strided(const uint8_t *payload, const uint64_t *off, int record_prefix, int off_first,
                                   int off_step, int N, const int64_t *index, int B, int C, const int32_t *cdf,
                                   int W, const int32_t *cdf_len, const int32_t *offset, const float *bias,
                                   const float *exp_scale, const float *median, void *z_hat, int z_dtype,
                                   size_t ld_out, int32_t *status, void *stream);
/* Host twin (host pointers, threaded over images): same values, same statuses. */
int lla_rans_decode_gather_host(const uint8_t *payload, const uint64_t *off, int record_prefix, int N,
                                const int64_t *index, int B, int C, const int32_t *cdf, int W,
                                const int32_t *cdf_len, const int32_t *offset, const float *bias,
                                const float *exp_scale, const float *median, void *z_hat, int z_dtype,
                                size_t ld_out, int32_t *status);

/* ------------------------------------------------------------------------- *
 * Windowed ("wide") factorized coder: any C, any W <= LLA_WIDE_MAX_W
 * ------------------------------------------------------------------------- *
 * The entry points above keep the whole u16 table [C][W] and the per-channel parameters resident in 64 KiB of LDS
 * and return LLA_EINVAL for a shape that does not fit (C = 512: the encoder from W = 49; C = 1024: from W = 29 or
 * earlier, the shipped width included).  The *_wide entry
 * points code the same streams -- byte for byte, symbol for symbol, bit for bit -- with the table passing through
 * LDS in WINDOWS of channels: one record per lane, all lanes of a workgroup walk the channel index in lock-step, so
 * at any moment the workgroup needs the rows of one window only.  The next window's rows are fetched while the
 * current one is coded (two LDS buffers).  The byte stream does not depend on the window.
 *
 * window_channels: 0 = the library chooses (lla_rans_wide_window reports the choice); otherwise a positive multiple
 *   of 4 (the encoder's group of channels; a multiple of 16 suits the gathered decoder's 16-channel staging best).
 *   A request above 256 or above C rounded up to 4 is clamped to that.  LLA_EINVAL for a value that is no
 *   multiple of 4, or whose two buffers do not fit 64 KiB of LDS.
 * Refusals, before any launch: W > LLA_WIDE_MAX_W (the smallest window, 4 channels, no longer fits the gathered
 *   decoder's LDS: 2 x 4 x W x 2 bytes of rows + 16.3 KiB of staging > 64 KiB; one bound for all three entry points);
 *   null pointers; the argument errors of the resident entry points.  B == 0: LLA_OK, no launch.
 * They take EVERY shape within that bound, the ones the resident entry points take included (slower there:
 * profiles/wide_coder.txt), so a caller chooses with lla_rans_table_fits. */
#define LLA_WIDE_MAX_W 3000
#define LLA_CODER_ENCODE 0 /* lla_rans_encode_batch, lla_quantise_encode                */
#define LLA_CODER_DECODE 1 /* lla_rans_decode_batch, lla_rans_decode_batch_strided      */
#define LLA_CODER_GATHER 2 /* lla_rans_decode_gather, lla_rans_decode_gather_strided    */
/* 1 when the RESIDENT entry points of `kind` take a table of C channels x W entries, 0 when they return LLA_EINVAL
 * for it (or for any C <= 0, W < 3, unknown kind).  Host arithmetic only: no device is touched. */
int lla_rans_table_fits(int C, int W, int kind);
/* The window (channels) the wide entry point of `kind` codes a C x W table with when given `window_channels`, and,
 * if lds_bytes is not NULL, the dynamic LDS of that launch.  LLA_EINVAL exactly where that entry point would refuse
 * the shape or the window.  Host arithmetic only. */
int lla_rans_wide_window(int C, int W, int kind, int window_channels, size_t *lds_bytes);

#define LLA_Z_SYMBOLS 0 /* lla_quantise_encode_wide only: `z` holds int32 symbols */
/* lla_quantise_encode for any table width: same arguments, same end-aligned scratch, lengths and symbols_out.
 * z_dtype LLA_Z_F16 / LLA_Z_F32 as there; LLA_Z_SYMBOLS makes it lla_rans_encode_batch: z [dev] B*C int32 symbols,
 * bias / exp_scale / median are not read (may be NULL) and symbols_out, if given, receives a copy. */
int lla_quantise_encode_wide(const void *z, int z_dtype, int B, int C, const float *bias,
                             const float *exp_scale, const float *median, const int32_t *cdf, int W,
                             const int32_t *cdf_len, const int32_t *offset, uint8_t *scratch,
                             size_t stride, uint32_t *lengths, int32_t *symbols_out, int window_channels,
                             void *stream);
/* lla_rans_decode_batch_strided for any table width: same arguments, values and statuses (an unopenable stream:
 * status 1, row of zeros).  status may be NULL. */
int lla_rans_decode_batch_wide(const uint8_t *payload, const uint64_t *off, int record_prefix, int off_first,
                               int off_step, int B, int C, const int32_t *cdf, int W, const int32_t *cdf_len,
                               const int32_t *offset, int32_t *symbols_out, int32_t *status,
                               int window_channels, void *stream);
/* lla_rans_decode_gather_strided for any table width: gather + decode + dequantise, fp16 or fp32 rows at ld_out,
 * statuses 0 / 1 / 2 and zeroed rows exactly as there; a lane without a record stays with its workgroup to the last
 * window, so its neighbours' rows are complete. */
int lla_rans_decode_gather_wide(const uint8_t *payload, const uint64_t *off, int record_prefix, int off_first,
                                int off_step, int N, const int64_t *index, int B, int C, const int32_t *cdf,
                                int W, const int32_t *cdf_len, const int32_t *offset, const float *bias,
                                const float *exp_scale, const float *median, void *z_hat, int z_dtype,
                                size_t ld_out, int32_t *status, int window_channels, void *stream);

/* The same two coder calls with an arbitrary table row per symbol, i.e. the full
 * ans.RansEncoder().encode_with_indexes(symbols, indexes, cdfs, cdfs_sizes, offsets) /
 * ans.RansDecoder().decode_with_indexes(...) signatures as GaussianConditional.compress /
 * .decompress use them (compressai EntropyModel.compress; lossyless/rates.py:704-729, scale
 * table rows selected by build_indexes) -- SURVEY.md 8(f) rank 4.
 * symbols, indexes [dev] B*n int32 (string b = elements [b*n, (b+1)*n)); cdf [dev] T*W int32,
 * cdf_len/offset [dev] T.  Rows are read from global memory (no size limit on T*W); an index
 * outside [0, T) is clamped.  scratch/stride/lengths and payload/off/record_prefix/status as
 * in lla_rans_encode_batch / lla_rans_decode_batch (stride >= lla_rans_max_encoded_bytes(n)). */
int lla_rans_encode_indexed(const int32_t *symbols, const int32_t *indexes, int B, int n,
                            const int32_t *cdf, int T, int W, const int32_t *cdf_len,
                            const int32_t *offset, uint8_t *scratch, size_t stride,
                            uint32_t *lengths, void *stream);
int lla_rans_decode_indexed(const uint8_t *payload, const uint64_t *off, int record_prefix, int B,
                            int n, const int32_t *indexes, const int32_t *cdf, int T, int W,
                            const int32_t *cdf_len, const int32_t *offset, int32_t *symbols_out,
                            int32_t *status, void *stream);

/* Conditional part of the scale hyperprior in one kernel.  Replaces, per batch, lossyless/rates.py:694-729:
 * process_z_in (:434-435), get_indexes_means_hat's build_indexes(scales_hat) and means_hat = scales_hat (:694-698),
 * and GaussianConditional.compress(z_in, indexes, means=means_hat) (:712: quantize "symbols" + one
 * RansEncoder.encode_with_indexes per image).  Per element, every operation rounded to fp32 on its own:
 *   z_in = (float(z) + bias) * exp_scale
 *   row  = T-1 - #{t < T-1 : max(scale, scale_bound) <= scale_table[t]}     (GaussianConditional.build_indexes)
 *   mean = scale            (the UNBOUNDED prediction: the reference passes the scales as means, rates.py:694-696)
 *   sym  = int(rint(z_in - mean))
 * and sym is coded with table row `row` into the end-aligned scratch exactly as lla_rans_encode_indexed would.
 * z [dev] B*C of z_dtype; bias/exp_scale [dev] C; scales [dev] fp32, element (b, c) at scales[b*ld_scales + c]
 * (ld_scales >= C: the first half of the z_encoder output is read where it lies); scale_table [dev] T floats;
 * cdf [dev] T*W int32, cdf_len/offset [dev] T (rows are read from global memory: a 64-level table is 800 KB).
 * symbols_out / indexes_out [dev] B*C int32, either may be NULL.  scratch/stride/lengths as in lla_rans_encode_batch. */
int lla_gaussian_quantise_encode(const void *z, int z_dtype, int B, int C, const float *bias,
                                 const float *exp_scale, const float *scales, size_t ld_scales,
                                 const float *scale_table, float scale_bound, const int32_t *cdf, int T, int W,
                                 const int32_t *cdf_len, const int32_t *offset, uint8_t *scratch, size_t stride,
                                 uint32_t *lengths, int32_t *symbols_out, int32_t *indexes_out, void *stream);

/* The inverse (lossyless/rates.py:715-724: build_indexes + GaussianConditional.decompress(z_strings, indexes,
 * means=means_hat) -- one RansDecoder.decode_with_indexes per image -- + process_z_out, :437-438): row and mean are
 * derived from `scales` as above, the records decoded, and
 *   z_hat = (float(sym) + mean) / exp_scale - bias          fp32 [dev] B*C.
 * Image b's stream is record off_first + b*off_step of `off` (see lla_rans_decode_batch_strided; off_first = 0,
 * off_step = 2 reads the z records of a body written by lla_rans_compact_pairs).  status [dev] B ints as in
 * lla_rans_decode_batch; every read is bounded by the record and by the table row, whatever the bytes hold. */
int lla_gaussian_decode_dequantise(const uint8_t *payload, const uint64_t *off, int record_prefix, int off_first,
                                   int off_step, int B, int C, const float *bias, const float *exp_scale,
                                   const float *scales, size_t ld_scales, const float *scale_table,
                                   float scale_bound, const int32_t *cdf, int T, int W, const int32_t *cdf_len,
                                   const int32_t *offset, float *z_hat, int32_t *status, void *stream);

/* Random access into the z records of an interleaved body: the second half of lossyless/rates.py:715-724
 * (GaussianConditional.decompress(z_strings, indexes, means=means_hat) + process_z_out) for the images a caller
 * names.  Output row b is record off_first + index[b]*off_step of `off` (N images, `off` as in
 * lla_rans_decode_gather_strided; off_first = 0, off_step = 2 for the z records), decoded exactly as
 * lla_gaussian_decode_dequantise decodes it: row and mean from scales[b*ld_scales + c] -- indexed by the OUTPUT row b,
 * not by the record: the caller's MLP ran on the gathered side information -- and
 *   z_hat = (float(sym) + mean) / exp_scale - bias,
 * written at z_hat + b*ld_out ELEMENTS (ld_out >= C) as fp32 (LLA_Z_F32: bit-equal to lla_gaussian_decode_dequantise
 * on the same record and scales) or as that value rounded to nearest even (LLA_Z_F16).  Columns C .. ld_out-1 are
 * never written.
 * status_in [dev] B ints or NULL: a non-zero entry (the side pass's status of that row) means the row's scales are
 * not to be trusted: nothing is read for it, the row is zeroed and the entry is copied to status[b].
 * status [dev] B ints: 0 decoded; 1 stream overrun or unopenable (row zeroed); 2 index[b] outside [0, N) (nothing
 * read, row zeroed).  Repeated indices are legal.  B == 0: LLA_OK, no launch.  LLA_EINVAL for off_first < 0 or
 * off_step < 1. */
int lla_gaussian_decode_gather(const uint8_t *payload, const uint64_t *off, int record_prefix, int off_first,
                               int off_step, int N, const int64_t *index, int B, int C, const float *bias,
                               const float *exp_scale, const float *scales, size_t ld_scales,
                               const float *scale_table, float scale_bound, const int32_t *cdf, int T, int W,
                               const int32_t *cdf_len, const int32_t *offset, void *z_hat, int z_dtype,
                               size_t ld_out, const int32_t *status_in, int32_t *status, void *stream);

/* What a launch of lla_gaussian_decode_gather on the CURRENT device asks for: returns the dynamic LDS request in
 * bytes (0 for arguments the entry point refuses) and stores in *front (may be NULL) the bytes in front of the
 * packed rows (affine, scale table, vote, staging).  The rows are searched in LDS when
 *   *front + 8*ceil((T+1)/2) + 8*T + 2 * sum_t min(max(cdf_len[t], 3), W)  <=  the value returned,
 * and in global memory otherwise (same results): a caller that depends on the LDS path checks this. */
size_t lla_gaussian_decode_gather_lds_bytes(int C, int T, int W, int z_dtype, size_t *front);

/* The three conditional entry points with the PREDICTED means: opt-in, never what a reference container was coded with.
 * The reference trains the conditional model on a likelihood centred at the predicted means (the second half of the
 * z_encoder output, lossyless/rates.py:647-650) but codes with the scales in their place (rates.py:689-696 overwrite
 * means_hat with scales_hat); the entry points above reproduce the latter.  These depart from rates.py:689-696 on
 * purpose and code with the means the likelihood of rates.py:647-650 belongs to.  Per element, every operation rounded
 * to fp32 on its own:
 *   z_in  = (float(z) + bias) * exp_scale
 *   row   = as above, from scales[b*ld_scales + c] alone: the row never depends on the mean
 *   mean  = means[b*ld_means + c]
 *   sym   = int(rint(z_in - mean))                      (encode)
 *   z_hat = (float(sym) + mean) / exp_scale - bias      (decode, gather)
 * means [dev] fp32, ld_means >= C ELEMENTS; a caller passes means = scales + C, ld_means = ld_scales to read the z_encoder
 * output where it lies.  Rows are fetched with 16-byte loads where the row (the matrix, for the gather) is 16-byte
 * aligned, element by element otherwise, independently of the scales' alignment.  means == NULL or ld_means < C:
 * LLA_EINVAL, no launch.  means == scales with ld_means == ld_scales gives the bytes / values of the entry point
 * without means.  Everything else -- arguments, statuses, bounds on every read -- as documented above.  The container
 * does not record which of the two coded it: records written by one and read by the other decode to wrong values
 * without an error. */

/* lla_gaussian_quantise_encode with means (rates.py:647-650's means, not rates.py:689-696's). */
int lla_gaussian_quantise_encode_means(const void *z, int z_dtype, int B, int C, const float *bias,
                                       const float *exp_scale, const float *scales, size_t ld_scales,
                                       const float *means, size_t ld_means, const float *scale_table,
                                       float scale_bound, const int32_t *cdf, int T, int W, const int32_t *cdf_len,
                                       const int32_t *offset, uint8_t *scratch, size_t stride, uint32_t *lengths,
                                       int32_t *symbols_out, int32_t *indexes_out, void *stream);

/* lla_gaussian_decode_dequantise with means (rates.py:647-650's means, not rates.py:689-696's). */
int lla_gaussian_decode_dequantise_means(const uint8_t *payload, const uint64_t *off, int record_prefix, int off_first,
                                         int off_step, int B, int C, const float *bias, const float *exp_scale,
                                         const float *scales, size_t ld_scales, const float *means, size_t ld_means,
                                         const float *scale_table, float scale_bound, const int32_t *cdf, int T, int W,
                                         const int32_t *cdf_len, const int32_t *offset, float *z_hat, int32_t *status,
                                         void *stream);

/* HOST twins of the two conditional coders (csrc/host.cpp; every pointer a host pointer, threaded over images): the same
 * rows (counted as above), the same three separately rounded fp32 operations and the host coder's rANS primitives -- the
 * same symbols, bytes and values as the device entry points, given the same `scales` (rates.MLP(precision="ordered")
 * gives the host the device's scales bit for bit).  means == NULL: the scales are the means (lla_gaussian_quantise_encode
 * / lla_gaussian_decode_dequantise); else element (b, c) at means[b*ld_means + c] (the _means forms).
 *   encode: image b's stream goes to out + out_off[b] (behind its be32 length if record_prefix), out_off [B+1] as in
 *           lla_rans_encode_batch_host -- LLA_ECAP with out_off filled when cap is too small (out may then be NULL).
 *   decode: image b's stream is record off_first + b*off_step of `off`; status[b] = 1 for a record shorter than 8 bytes,
 *           not a whole number of words, or read past its end (its row is then zeros, as the device leaves it for a record it
 *           cannot open, or whatever the bounded reads gave). */
int lla_gaussian_quantise_encode_host(const void *z, int z_dtype, int B, int C, const float *bias,
                                      const float *exp_scale, const float *scales, size_t ld_scales,
                                      const float *means, size_t ld_means, const float *scale_table,
                                      float scale_bound, const int32_t *cdf, int T, int W, const int32_t *cdf_len,
                                      const int32_t *offset, int record_prefix, uint8_t *out, size_t cap,
                                      uint64_t *out_off, int32_t *symbols_out, int32_t *indexes_out);
int lla_gaussian_decode_dequantise_host(const uint8_t *payload, const uint64_t *off, int record_prefix, int off_first,
                                        int off_step, int B, int C, const float *bias, const float *exp_scale,
                                        const float *scales, size_t ld_scales, const float *means, size_t ld_means,
                                        const float *scale_table, float scale_bound, const int32_t *cdf, int T, int W,
                                        const int32_t *cdf_len, const int32_t *offset, float *z_hat, int32_t *status);

/* lla_gaussian_decode_gather with means (rates.py:647-650's means, not rates.py:689-696's): `means` is indexed by the
 * OUTPUT row b, as `scales` is.  A row whose status_in is non-zero reads neither matrix.  The means are staged in LDS
 * next to the scales (32 KiB more in front of the packed rows): lla_gaussian_decode_gather_means_lds_bytes is this entry
 * point's size query, with the meaning of lla_gaussian_decode_gather_lds_bytes. */
int lla_gaussian_decode_gather_means(const uint8_t *payload, const uint64_t *off, int record_prefix, int off_first,
                                     int off_step, int N, const int64_t *index, int B, int C, const float *bias,
                                     const float *exp_scale, const float *scales, size_t ld_scales, const float *means,
                                     size_t ld_means, const float *scale_table, float scale_bound, const int32_t *cdf,
                                     int T, int W, const int32_t *cdf_len, const int32_t *offset, void *z_hat,
                                     int z_dtype, size_t ld_out, const int32_t *status_in, int32_t *status,
                                     void *stream);
size_t lla_gaussian_decode_gather_means_lds_bytes(int C, int T, int W, int z_dtype, size_t *front);

/* EntropyModel.dequantize + process_z_out (hub/compressor.py:111-115):
 * z_hat = (float(sym) + median) / exp_scale - bias, fp32 per operation. */
int lla_dequantise(const int32_t *symbols, int B, int C, const float *bias,
                   const float *exp_scale, const float *median, float *z_hat, void *stream);

/* compressor(X) without coding: process_z_in -> EntropyBottleneck.forward (eval:
 * round(z_in - median) + median) -> process_z_out, hub/compressor.py:95,100-101. */
int lla_represent(const void *z, int z_dtype, int B, int C, const float *bias,
                  const float *exp_scale, const float *median, float *z_hat, void *stream);

/* ------------------------------------------------------------------------- *
 * Device entry point: CLIP preprocessing
 *   stands in for  compressor.preprocess  = clip._transform (clip==1.0): Resize(224,
 *   BICUBIC) -> CenterCrop(224) -> ToTensor -> Normalize, which the reference applies per
 *   image with PIL in DataLoader workers (hub/compressor.py:155,186;
 *   utils/data/images.py:383-411).  Bit-exact against Pillow's 8-bit resampler.
 * ------------------------------------------------------------------------- */

/* images [dev] uint8 [B][H][W][3] (RGB, all the same size).  The tap tables are built on the
 * host exactly as Pillow's precompute_coeffs / normalize_coeffs_8bpc do (see
 * lossyless_amd/preprocess.py) for the 224 output columns / rows that survive the centre
 * crop: bounds int32 [224][2] = (first tap, tap count), coef int32 [224][ksize] 22-bit fixed
 * point; v_bounds index rows of the RESIZED-width intermediate, i.e. input rows; only input
 * rows [row0, row0+nrows) are touched.  mean3 / std3 [host] floats.  out fp16 [B][224][224][3].
 * workspace [dev] >= lla_preprocess_workspace_bytes(B, nrows). */
size_t lla_preprocess_workspace_bytes(int B, int nrows);
int lla_preprocess_clip(const uint8_t *images, int B, int H, int W, int row0, int nrows,
                        const int32_t *h_bounds, const int32_t *h_coef, int h_ksize,
                        const int32_t *v_bounds, const int32_t *v_coef, int v_ksize,
                        const float *mean3, const float *std3, void *workspace,
                        size_t workspace_bytes, void *out_nhwc_f16, void *stream);

/* Pillow's resampling tap tables on the host -- Resample.c precompute_coeffs (bicubic, a = -0.5, box = the
 * whole axis) followed by normalize_coeffs_8bpc, in the same double arithmetic -- for output positions
 * first .. first+count-1 of a resize in_size -> out_size:
 *   bounds [count][2] = (first tap, number of taps), coef [count][ksize] 22-bit fixed point, rows zero
 *   padded; ksize = lla_pillow_bicubic_ksize(in_size, out_size) = 2 ceil(2 max(in/out, 1)) + 1.
 * A tap TABLE as the ragged entry point below takes it is bounds[224][2] followed by coef[224][ksize]. */
int lla_pillow_bicubic_ksize(int in_size, int out_size);
int lla_pillow_bicubic_taps(int in_size, int out_size, int first, int count, int ksize, int32_t *bounds,
                            int32_t *coef);

/* Ragged batches (every image its own size: ImageNet-style folders, BASELINE configs[2]) -- what the
 * reference's per-image `compressor.preprocess` handles by construction (hub/compressor.py:162-165).
 * One descriptor per image; pointers are DEVICE pointers.  Pixels are RGB, 3 bytes per pixel, rows
 * contiguous; the 3 bytes after an image's last byte must be readable (rows are fetched as aligned
 * dwords).  h_table / v_table: tap tables (see lla_pillow_bicubic_taps) of the 224 cropped output columns /
 * rows; vertical bounds index source rows.  Same bytes out as lla_preprocess_clip on each image alone. */
typedef struct lla_image_desc {
  const uint8_t *pixels;
  const int32_t *h_table;
  const int32_t *v_table;
  int32_t H, W;
  int32_t h_ksize, v_ksize;
} lla_image_desc;
/* LDS bytes one workgroup needs for an image with these (HOST) tables when a band is `band_rows` output rows
 * (a divisor-friendly height such as 28, 14, 7, 4, 2, 1).  The caller passes the maximum over the images of
 * a launch as lds_bytes; LLA_ECAP if that exceeds what the device gives one workgroup (such images go
 * through lla_preprocess_clip one at a time: its two-pass path has no size limit). */
size_t lla_preprocess_ragged_lds_bytes(const int32_t *h_table, int h_ksize, const int32_t *v_table,
                                       int v_ksize, int band_rows);
/* descs [dev] B descriptors; out fp16 [B][224][224][3]. */
int lla_preprocess_clip_ragged(const lla_image_desc *descs, int B, int band_rows, size_t lds_bytes,
                               const float *mean3, const float *std3, void *out_nhwc_f16, void *stream);

/* Synthetic workload (BASELINE.json configs[3]: 1M x 224 x 224 x 3 images sharded across ranks, never
 * materialised): images first_image .. first_image+count-1 of the virtual dataset `seed`, CLIP-normalised fp16
 * NHWC [count][224][224][3].  Element e of the whole virtual tensor is
 *   h = (e ^ (seed * 0x9E3779B97F4A7C15 & (2^63 - 1))) * 0x2545F4914F6CDD1D;  h ^= h >> 29 (int64);
 *   h *= 0x94D049BB133111EB;  u8 = (h >> 40) & 255;  value = fp16((u8 / 255 - mean[c]) / std[c])
 * -- a pure function of (seed, e), so every sharding of the image range generates the same bytes. */
int lla_synthetic_images(uint64_t seed, uint64_t first_image, int count, const float *mean3, const float *std3,
                         void *out_nhwc_f16, void *stream);

/* ------------------------------------------------------------------------- *
 * Device entry points: CLIP ViT-B/32 visual tower (A10)
 *   stands in for  z = self.clip(X)  at hub/compressor.py:93
 *   (clip.model.VisionTransformer.forward, clip==1.0).
 * ------------------------------------------------------------------------- */

#define LLA_LAYOUT_NHWC 0 /* images [B][224][224][3] fp16 */
#define LLA_LAYOUT_NCHW 1 /* images [B][3][224][224] fp16 (what the reference feeds) */

/* Parameter ids of the weight blob.  Matrices are fp16 in torch Linear layout
 * [out][in]; vectors (LayerNorm, biases, embeddings) are fp32. */
enum lla_vit_param {
  LLA_VIT_CONV1_NHWC = 0, /* fp16 [768][32][32][3]   (kh,kw,c) K-order          */
  LLA_VIT_CONV1_NCHW,     /* fp16 [768][3][32][32]   OpenAI order               */
  LLA_VIT_CLASS_EMB,      /* fp32 [768]                                         */
  LLA_VIT_POS_EMB,        /* fp32 [50][768]                                     */
  LLA_VIT_LN_PRE_W,       /* fp32 [768]                                         */
  LLA_VIT_LN_PRE_B,
  LLA_VIT_LN_POST_W,
  LLA_VIT_LN_POST_B,
  LLA_VIT_PROJ_T,         /* fp16 [512][768] = proj.T                           */
  LLA_VIT_GLOBAL_COUNT,
  /* per-layer ids, use with layer = 0..11 */
  LLA_VIT_LN1_W = 16, LLA_VIT_LN1_B,
  LLA_VIT_QKV_W,          /* fp16 [2304][768] attn.in_proj_weight               */
  LLA_VIT_QKV_B,          /* fp32 [2304]                                        */
  LLA_VIT_OUT_W,          /* fp16 [768][768]  attn.out_proj.weight              */
  LLA_VIT_OUT_B,
  LLA_VIT_LN2_W, LLA_VIT_LN2_B,
  LLA_VIT_FC_W,           /* fp16 [3072][768] mlp.c_fc.weight                   */
  LLA_VIT_FC_B,
  LLA_VIT_CPROJ_W,        /* fp16 [768][3072] mlp.c_proj.weight                 */
  LLA_VIT_CPROJ_B,
  LLA_VIT_LAYER_END
};

/* Total bytes of the weight blob. */
size_t lla_vit_b32_weights_bytes(void);
/* Byte offset / byte size of one parameter inside the blob (layer ignored for
 * global ids).  Returns (size_t)-1 for an unknown id. */
size_t lla_vit_b32_param_offset(int param, int layer);
size_t lla_vit_b32_param_bytes(int param);

/* Workspace bytes for a pass that processes `chunk` images at a time (one set of slice buffers: the product library
 * runs the tower on ONE stream; the ablation build doubles it when its two lanes are switched on). */
size_t lla_vit_b32_workspace_bytes(int chunk);

/* images [dev] fp16 in `layout`, CLIP-normalised; weights [dev] blob;
 * z_out [dev] fp16 [B][512].  The batch is walked in slices of at most `chunk` images
 * (chunk <= 0: library default 8704 = 1700 row tiles of 256; capped at 65536; a ragged slice of >= 256 images is cut once more
 * into a multiple of 128 images + the rest: whole 256-row tiles for the residual layers' four-wave GEMM), all on `stream`.  Re-entrant: no
 * state outside the arguments. */
int lla_vit_b32_forward(const void *images, int layout, int B, const void *weights,
                        void *workspace, size_t workspace_bytes, int chunk, void *z_out,
                        void *stream);

/* Tower handle: two HIP streams ("lanes") of the CURRENT device plus the events that fork them from and
 * join them into the caller's stream.  The lanes are the only state the tower entry points keep between
 * calls, and it lives here, in an object the caller owns (one handle per device and driving thread; the
 * entry points taking a handle are not thread-safe with respect to that handle). */
int lla_tower_create(void **tower);
int lla_tower_destroy(void *tower);   /* waits for the lanes to drain */

/* Options of a tower handle (ABI v3).  They select between code paths that give the SAME embeddings bit for bit -- what
 * tests/test_gpu_vit.py asserts with them; nothing here is needed for production use.
 *   LLA_TOWER_OPT_LNX       1 (default): slices of whole 256-row tiles apply the LayerNorm that follows a residual GEMM
 *                           (ln_2 after out-proj, ln_1 of the next block after c_proj: clip VisionTransformer,
 *                           hub/compressor.py:93) in that GEMM's epilogue; 0: layernorm768_kernel after every such GEMM.
 *   LLA_TOWER_OPT_LNX_WAIT  shader cycles a column tile waits there for the two other column tiles of its rows
 *                           (default 24000); < 0: never -- every row tile is normalised by the clean-up kernel. */
#define LLA_TOWER_OPT_LNX 1
#define LLA_TOWER_OPT_LNX_WAIT 2
int lla_tower_set_option(void *tower, int option, int value);

/* The same pass through a tower handle.  PRODUCT LIBRARY (since round 4): everything runs on `stream`, `deferred` only
 * means "the caller joins later", and lla_tower_join is a cheap no-op dependency -- same results, same order.  The
 * two-lane mode described below exists in the tools/ build only (`make ablation`, LLA_VIT_STREAMS=2 there: csrc/switches.h): with two hardware
 * queues active the tower is not bit-reproducible on this stack -- between one embedding in 10^6 and one in 10^8
 * images (box and build dependent) differs by a few fp16 ulps between runs, docs/history/DESIGN_rounds_1-5.md 5.3 -- and bit-identical records
 * for identical inputs are this path's contract.  The entry points stay so that callers written against ABI v2 keep
 * working unchanged.
 *   deferred = 0: batches of >= 640 images (LLA_VIT_SPLIT_MIN) are cut into at least two slices that
 *     alternate between the lanes, forked from and joined back into `stream` with events, when the
 *     workspace holds two slices: one lane's GEMM tails and HBM-bound kernels overlap the other's GEMMs.
 *   deferred = 1: no closing join, for callers that run many batches back to back (RecordStream /
 *     compress_dataset): whole slices alternate between the lanes ACROSS calls, so one batch's last GEMM
 *     rounds overlap the next batch's first kernels.  `z_out` (and the lanes' use of `images`) is complete
 *     on `stream` only after lla_tower_join(tower, stream); a later non-deferred pass on the same handle
 *     joins as well.
 * A workspace of one slice also keeps everything on `stream`. */
int lla_vit_b32_forward_lanes(void *tower, const void *images, int layout, int B, const void *weights,
                              void *workspace, size_t workspace_bytes, int chunk, void *z_out,
                              void *stream, int deferred);
/* `stream` waits for everything queued on the handle's lanes so far. */
int lla_tower_join(void *tower, void *stream);

/* The same pass over a batch that lies in `n_pieces` separate device arrays of `piece_images` images each (the last one
 * may hold fewer): what a caller has who gathers equal batches -- the reference's loop hands over one DataLoader batch
 * at a time, hub/compressor.py:186-197 -- into one chip-filling tower pass, without copying them into one array first
 * (301 KB per image read and written again: 2 % of a pass).  Only the patch-embedding GEMM reads the images; it walks
 * them in 256-row tiles, and 256 images are 49 whole tiles, so with piece_images % 256 == 0 no tile straddles two
 * pieces (a caller whose batches are larger multiples of 256 passes piece_images = 256 and one pointer per 256 images, so
 * that a tower pass may also end in the middle of a batch).  Same embeddings, bit for bit, as lla_vit_b32_forward on the
 * concatenated batch.
 * LLA_EINVAL unless 1 <= n_pieces <= 64, piece_images % 256 == 0, (n_pieces - 1) piece_images < B <= n_pieces piece_images,
 * B % 128 == 0, 256 <= B <= the library's slice size (8704), and the workspace holds one slice of B images: the caller
 * then copies (lla_vit_b32_forward).  Everything runs on `stream`; `pieces` (host array of device pointers) is read
 * before the call returns, the images until the pass has run. */
int lla_vit_b32_forward_gather(void *tower, const void *const *pieces, int n_pieces, int piece_images, int layout, int B,
                               const void *weights, void *workspace, size_t workspace_bytes, void *z_out, void *stream);

/* Optional per-kernel-class timing with HIP events recorded on the launch stream
 * (what bench.py's `roofline` object is computed from).  A profiler owns a pool of
 * event pairs; every kernel launched by lla_vit_b32_forward_profiled is bracketed by
 * one pair.  lla_profiler_collect synchronises the recorded events, accumulates
 * per class  ms[c] += elapsed, work[c] += algorithmic FLOPs (GEMM: 2*M*N*K,
 * attention: 4*50*50*64 per head) or bytes (LayerNorm: bytes read + written),
 * launches[c] += 1, and rewinds the pool. */
#define LLA_PROF_GEMM 0
#define LLA_PROF_LAYERNORM 1
#define LLA_PROF_ATTENTION 2
#define LLA_PROF_CLASSES 3
int lla_profiler_create(void **profiler, int max_launches);
int lla_profiler_destroy(void *profiler);
int lla_profiler_collect(void *profiler, double *ms, double *work, long long *launches);
/* Same as lla_vit_b32_forward (one stream, so that a kernel's duration is its own); profiler may be NULL. */
int lla_vit_b32_forward_profiled(const void *images, int layout, int B, const void *weights,
                                 void *workspace, size_t workspace_bytes, int chunk, void *z_out,
                                 void *stream, void *profiler);

/* Building blocks of the tower, exported for per-kernel parity tests and
 * profiling (same kernels lla_vit_b32_forward launches). */
#define LLA_EPI_F16 0          /* C16 = acc (+bias)                     */
#define LLA_EPI_QUICKGELU_F16 1 /* C16 = quickgelu(acc + bias)           */
#define LLA_EPI_RESID_F32 2    /* C32 += acc + bias                     */
#define LLA_EPI_RELU_F16 4     /* C16 = relu(acc + bias)               */
#define LLA_EPI_ADD_RELU_F16 5 /* C16 = relu(acc + bias + R16)         */
/* C[M][N] (+)= A[M][K] * W[N][K]^T ; A, W fp16 row-major; bias fp32 [N] or NULL.
 * N % 128 == 0, K % 64 == 0. */
int lla_gemm_f16(const void *A, const void *W, const float *bias, void *C, int M, int N, int K,
                 int epilogue, void *stream);
/* The same with explicit row strides (elements; lda % 8 == 0, ldc % 4 == 0 -- ldc % 8 == 0 for an fp16 output that the
 * 256-column persistent kernels take, whose epilogues store 16 bytes per lane: LLA_EINVAL otherwise; with the ReLU epilogues ldc < N,
 * a multiple of 32, stores only the first ldc columns: narrow convolution outputs keep a narrow pitch) and, for
 * LLA_EPI_ADD_RELU_F16, an fp16 matrix R [M][ldr] added before the ReLU (the identity branch of a
 * ResNet bottleneck).  Used by the RN50-CLIP tower below, where 1x1 convolutions are GEMMs over NHWC
 * activations with a channel pitch. */
int lla_gemm_f16_ex(const void *A, int lda, const void *W, const float *bias, void *C, int ldc,
                    const void *resid, int ldr, int M, int N, int K, int epilogue, void *stream);

/* Introspection for tests and tools (no device call): which kernel lla_gemm_f16_ex / the towers would launch for this shape on
 * a device with `cus` compute units.  epi: LLA_EPI_* (3: the patch embedding, amode 1 NHWC / 2 NCHW; 9: residual + LayerNorm),
 * amode 0: plain operands, 3: implicit 3x3 convolution; a_chunk_images: the image batch in pieces (0: contiguous).
 * *kernel: 0 nothing to launch, 1 gemm_f16_kernel, 2 gemm256_f16_kernel, 3 / 4 gemm_persistent_kernel 128 / 256 columns wide,
 * 5 gemm_pp_kernel, 6 gemm_q4_kernel, 7 gemm_w8_kernel; *tile_rows: rows per tile; *grid: workgroups.  LLA_EINVAL: refused. */
int lla_gemm_plan(int epi, int amode, int M, int N, int K, int lda, int ldc, int a_chunk_images, int cus,
                  int *kernel, int *tile_rows, int *grid);

/* fp32 Linear layer on the fp32 matrix cores: C[M][N] = A[M][K] * W[N][K]^T (+ bias) (ReLU if `relu`), all
 * fp32 row-major with row strides lda / ldw / ldc (elements, multiples of 4; K % 8 == 0, N % 4 == 0 -- pad with
 * zeros).  Stands in for the `nn.Linear` layers of the reference's hyperprior networks, which run in fp32 under
 * autocast(False) (lossyless/rates.py:104,631-639,687-699; lossyless/architectures.py:94-168): fp32 operands and
 * accumulation, one rounding per product (v_mfma_f32_32x32x2_f32 = an fma chain), K order fixed by the kernel
 * alone, so the values do not depend on the batch size (encoder and decoder may use different ones). */
int lla_gemm_f32(const float *A, int lda, const float *W, int ldw, const float *bias, float *C, int ldc,
                 int M, int N, int K, int relu, void *stream);

/* The same layer with a DEFINED arithmetic (csrc/gemm_f32_ordered.hip, whose header comment is the contract), on the
 * VALU: the operands, pitches and padding rules of lla_gemm_f32 (A, W, C and bias 16-byte aligned besides), and for every
 * output element, whatever M, the grid or the call's row offset,
 *     acc = +0.0f;  for k = 0 .. K-1 ascending (padding included): acc = fmaf(A[m][k], W[n][k], acc);
 *     y = acc + bias[n] (one rounded add; skipped for bias == NULL);  relu: y = y > 0.f ? y : 0.f;  C[m][n] = y
 * in IEEE-754 binary32, round to nearest even, denormals kept.  lla_gemm_f32_ordered_host (csrc/host.cpp) takes the same
 * arguments as HOST pointers (no alignment asked) and runs the same chain with std::fmaf, threaded over rows: the same
 * bits.  What rates.MLP(precision="ordered") runs on, so that a hyperprior container can be decoded without a GPU. */
int lla_gemm_f32_ordered(const float *A, int lda, const float *W, int ldw, const float *bias, float *C, int ldc,
                         int M, int N, int K, int relu, void *stream);
int lla_gemm_f32_ordered_host(const float *A, int lda, const float *W, int ldw, const float *bias, float *C, int ldc,
                              int M, int N, int K, int relu);

/* One data pass of a linear probe (lossyless_amd/csrc/probe.hip): the sums that the LinearSVC objective -- squared hinge,
 * one-vs-rest, the third step of the reference's workflow (README.md:74-82: LinearSVC(C=7e-3).fit(Z, Y) on the
 * decompressed features) -- needs from B rows, for all K classifiers at once, on the fp32 matrix cores.
 *   z [B][C] (pitch ld_z elements; LLA_Z_F32, or LLA_Z_F16 widened exactly), y[i] a class index: y_ik = +1 iff
 *   y[i] == k, so a label outside [0, K) is negative for every classifier (two classes: K = 1, label 0 = positive).
 *   s_ik = z_i . W_k + b_k,  m_ik = max(0, 1 - y_ik s_ik);  W, V, out_W are [K][C] with pitch ld_w.
 *   V == NULL (gradient):      out_loss[k] = sum_i m_ik^2, out_W[k] = sum_i (-2 y_ik m_ik) z_i, out_b[k] = sum_i (-2 y_ik m_ik)
 *   V != NULL (Hessian-vector): t_ik = [m_ik > 0] (z_i . V_k + vb_k), out_W[k] = sum_i 2 t_ik z_i, out_b[k] = sum_i 2 t_ik;
 *                               out_loss is not touched (may be NULL).
 * The factor C of the objective and its 1/2 |.|^2 terms are the caller's.  accumulate = 1 adds this call's totals to what
 * the outputs hold (a dataset walked in decode groups).  No floating-point atomics: workgroups leave partial sums in
 * `workspace` (lla_svm_pass_workspace_bytes(C, K) bytes; 0 for a refused shape) and a second kernel adds them in a fixed
 * order, the loss in double: the same inputs give the same bits.
 * C % 8 == 0, 8 <= C <= 1024, K >= 1, ld_z >= C, ld_w >= C, pitches multiples of 4, z 16-byte (fp16: 8-byte) and W / V
 * 16-byte aligned; anything else is LLA_EINVAL, decided before any device call.  B == 0: LLA_OK (the outputs are zeroed
 * unless accumulate is set, then nothing is touched). */
size_t lla_svm_pass_workspace_bytes(int C, int K);
int lla_svm_pass(const void *z, int z_dtype, int ld_z, const int32_t *y, int B, int C, const float *W, const float *b,
                 const float *V, const float *vb, int K, int ld_w, float *out_W, float *out_b, double *out_loss,
                 int accumulate, void *workspace, void *stream);

/* The same pass over J independent problems in the place of the K classes: every (candidate, fold, class) of a
 * cross-validated search over C and class_weight (the reference's utils/Z_linear_eval.py:62-93) in the passes of one fit.
 * Problem j has a positive class, a held-out fold and one weight per sign:
 *   y_ij = +1 iff y[i] == col_class[j];  c_ij = 0 if fold != NULL and fold[i] == col_held[j], else col_cpos[j] where
 *   y_ij = +1 and col_cneg[j] where y_ij = -1  (liblinear's class weights: C w[k] for the rows of class k, C for the rest).
 *   V == NULL:  out_loss[j] = sum_i c_ij m_ij^2, out_W[j] = sum_i c_ij (-2 y_ij m_ij) z_i, out_b[j] = sum_i c_ij (-2 y_ij m_ij)
 *   V != NULL:  out_W[j] = sum_i 2 c_ij t_ij z_i, out_b[j] = sum_i 2 c_ij t_ij.
 * W, V, out_W are [J][C], the col_* arrays [J], fold [B] (NULL: no row is held out); all on the device.  The weight is one
 * more fp32 multiply of the residual and of m^2; grid, workspace layout and order of the sums are those of lla_svm_pass
 * for K = J, so fold == NULL, col_class = 0 .. J-1 and unit weights return its bits.  Same shape rules and refusals;
 * a NULL col_* pointer is LLA_EINVAL.  lla_svm_grid_pass_workspace_bytes(C, J) == lla_svm_pass_workspace_bytes(C, J). */
size_t lla_svm_grid_pass_workspace_bytes(int C, int J);
int lla_svm_grid_pass(const void *z, int z_dtype, int ld_z, const int32_t *y, const int32_t *fold, int B, int C,
                      const float *W, const float *b, const float *V, const float *vb, int J, int ld_w,
                      const int32_t *col_class, const int32_t *col_held, const float *col_cpos, const float *col_cneg,
                      float *out_W, float *out_b, double *out_loss, int accumulate, void *workspace, void *stream);

/* One data pass of L2-regularised multinomial logistic regression (softmax regression; CLIP's linear-probe protocol):
 * lla_svm_pass's walk with the softmax residual in the place of the hinge's.
 *   s_ik = z_i . W_k + b_k,  lse_i = log sum_k exp(s_ik) over the K classes,  p_ik = exp(s_ik - lse_i),
 *   w_i = class_weight[y[i]] (class_weight [K] on the device, NULL = 1); a row whose label lies outside [0, K) has
 *   w_i = 0 and contributes exactly nothing.
 *   V == NULL (gradient):  r_ik = w_i (p_ik - [y_i = k]);  out_W[k] = sum_i r_ik z_i, out_b[k] = sum_i r_ik,
 *                          out_loss[k] = sum_{i: y_i = k} w_i (lse_i - s_ik)  (the loss is their sum over k)
 *   V != NULL (Hessian-vector):  t_ik = z_i . V_k + vb_k,  a_i = sum_k p_ik t_ik,  r_ik = w_i p_ik (t_ik - a_i);
 *                          out_W, out_b as above, out_loss is not touched (may be NULL).
 * The row maximum is always subtracted; expf / logf, no fast variants.  K <= 32: the row statistics are taken inside the
 * pass (z is read once).  K > 32: a first kernel leaves lse [B] and a [B] in the workspace, which is why
 * lla_softmax_pass_workspace_bytes takes B (the largest B of the calls that share the workspace; 0 for a refused shape).
 * The factor C of the objective and its 1/2 |.|^2 terms are the caller's.  Shape and alignment rules, refusals
 * (LLA_EINVAL before any device call), B == 0, accumulate, the workgroup-ordered reduction (no floating-point atomics,
 * the loss in double, a grid that depends on (B, K) alone: the same inputs give the same bits): as lla_svm_pass. */
size_t lla_softmax_pass_workspace_bytes(int C, int K, int B);
int lla_softmax_pass(const void *z, int z_dtype, int ld_z, const int32_t *y, int B, int C, const float *W, const float *b,
                     const float *V, const float *vb, int K, int ld_w, const float *class_weight, float *out_W,
                     float *out_b, double *out_loss, int accumulate, void *workspace, void *stream);

/* The same pass over G classifiers ("groups") of K <= 32 classes each that see the same rows: every (candidate, fold) of a
 * cross-validated softmax regression in the passes of one fit.  W, V, out_W are [G K][C] with pitch ld_w, class k of group
 * g in row g K + k; b, vb, out_b, out_loss are [G K]; group_held is [G]; group_class_weight is [G][K] (NULL = 1); fold is
 * [B] (NULL: no row is held out); all on the device.  The quantities are lla_softmax_pass's per group, with the row weight
 *   w_ig = 0 if (fold != NULL and fold[i] == group_held[g]) or y[i] lies outside [0, K), else group_class_weight[g][y[i]]
 * -- selected, not multiplied by a mask: no rounding is added.  A 32-column tile holds 32 / K whole groups (the columns
 * left over are dead), so the pass walks ceil(G / (32 / K)) tiles and its grid is a function of (B, K, G) alone; within a
 * group the maximum and the sums run over its classes in class order, as lla_softmax_pass does, so where the grids agree
 * (one tile) a group's slice of the outputs is bitwise what lla_softmax_pass returns for (W_g, b_g, y with the held-out
 * rows relabelled -1, group_class_weight[g]).  K < 1, K > 32, G < 1 and group_held == NULL with fold != NULL are
 * LLA_EINVAL (the workspace size of a refused shape is 0); everything else as lla_softmax_pass. */
size_t lla_softmax_grid_pass_workspace_bytes(int C, int K, int G);
int lla_softmax_grid_pass(const void *z, int z_dtype, int ld_z, const int32_t *y, const int32_t *fold, int B, int C,
                          const float *W, const float *b, const float *V, const float *vb, int K, int G, int ld_w,
                          const int32_t *group_held, const float *group_class_weight, float *out_W, float *out_b,
                          double *out_loss, int accumulate, void *workspace, void *stream);

/* One data pass of a weighted k-nearest-neighbour classifier (lossyless_amd/csrc/knn.hip) -- the training-free protocol
 * for judging frozen features (Wu et al. 2018, "Unsupervised Feature Learning via Non-Parametric Instance Discrimination",
 * sec. 3.4; DINO, Caron et al. 2021, sec. 4.1: cosine similarity, the k best neighbours, each voting exp(s / T)); the
 * reference has no k-NN.  Every query of the resident block q [Q][C] (fp32, pitch ld_q) keeps a running list of its k best
 * (score, global index) pairs over the train rows seen so far; this call shows it the n rows z [n][C] (pitch ld_z;
 * LLA_Z_F32, or LLA_Z_F16 widened exactly) whose global indexes are row_base .. row_base + n - 1.
 *   metric 0: s_ij = q_i . z_j     metric 1: s_ij = (q_i . z_j) * (1 / sqrt(sum_c z_jc^2))   (0 for a row of zeros)
 * -- exact fp32 products, fp32 accumulation (v_mfma_f32_32x32x2_f32), the reciprocal norm in fp32 in an order fixed by C;
 * the caller normalises the queries.  q_self [Q] (NULL: none) names per query one global index that is never listed
 * (leave-one-out).  accumulate = 0 starts from empty lists, 1 continues what earlier calls with the same (Q, k) and
 * workspace left.  Scores never reach memory: the lists live in `workspace` (lla_knn_pass_workspace_bytes(Q, k) bytes, 0
 * for a refused shape; O(Q k walkers), nothing proportional to Q n), one per walker of the split train range.
 * Order: (score descending, global index ascending), a total order, and a score's bits depend on (q_i, z_j, C, metric)
 * alone, so the lists lla_knn_finish returns are a pure function of the rows shown: the same bits for any split into calls.
 * C % 8 == 0, 8 <= C <= 1024, 1 <= k <= 256, Q >= 1, metric 0 / 1, ld_q, ld_z >= C and multiples of 4, q and z 16-byte
 * (fp16: 8-byte) aligned, row_base >= 0 and row_base + n <= INT32_MAX: anything else is LLA_EINVAL before any device call.
 * n == 0: LLA_OK without a launch, nothing is touched (the first call of a search shows at least one row).  The last
 * 8 bytes of the workspace count the insertions of all calls since the caller zeroed them (a diagnostic: tools/knn_bench.py). */
size_t lla_knn_pass_workspace_bytes(int Q, int k);
int lla_knn_pass(const float *q, int ld_q, int Q, const void *z, int z_dtype, int ld_z, int n, int C, int row_base, int k,
                 int metric, const int32_t *q_self, int accumulate, void *workspace, void *stream);

/* Merges the walkers' lists of lla_knn_pass (same Q, k, workspace) in walker order under the same total order and writes
 * the first k_out <= k entries of every list -- the lists are sorted, so they are the query's top k_out: one search serves
 * every smaller k -- to top_val [Q][k_out] fp32 and top_idx [Q][k_out] int32, best first; slots beyond the rows seen hold
 * (-inf, -1); r below runs over the k_out entries.  With labels [N]
 * (class indexes in [0, K); any other label does not vote), it also writes
 *   votes[i][c] = sum_r exp((s_ir - s_i0) * inv_T) [labels[idx_ir] == c]      (votes [Q][K] fp32)
 * the weights of Wu et al. / DINO scaled by exp(-s_i0 / T) so that nothing overflows (inv_T = 0: every neighbour votes 1);
 * the sum runs serially in rank order, one thread per (query, class): no floating-point atomics.  labels == NULL: votes is
 * not touched (K is ignored).  The workspace is only read, so the call may be repeated with another k_out or inv_T.
 * 1 <= k_out <= k <= 256, Q >= 1, K >= 1 with labels; anything else is LLA_EINVAL before any launch. */
int lla_knn_finish(int Q, int k, int k_out, const int32_t *labels, int K, float inv_T, float *top_val, int32_t *top_idx,
                   float *votes, const void *workspace, void *stream);

/* One Lloyd iteration of k-means (lossyless_amd/csrc/kmeans.hip) -- the unsupervised protocol for judging frozen features:
 * cluster, then score the clusters against the labels (DeepCluster, Caron et al. 2018; SCAN, Van Gansbeke et al. 2020); the
 * reference has no clustering.  lla_svm_pass's walk with an argmax over the centroids in the place of the hinge residual.
 *   z [B][C] (pitch ld_z; LLA_Z_F32, or LLA_Z_F16 widened exactly); W [K][C] (pitch ld_w), b [K]: the centroids' affine scores.
 *   n2_i = sum_c z_ic^2, in fp32 in an order fixed by C.
 *   metric 0 (Euclidean):  s_ik = z_i . W_k + b_k           w_i = 1     dist_i = max(0, n2_i - 2 s_i,a_i)
 *                          -- with W = the centres and b_k = -1/2 |c_k|^2, the squared distance to the nearest centre
 *   metric 1 (spherical):  s_ik = (z_i . W_k) r_i + b_k     w_i = r_i   dist_i = 1 - s_i,a_i
 *                          r_i = 1 / sqrt(n2_i), 0 for a row of zeros
 *   a_i = argmax_k s_ik, the lowest k on ties;  out_assign [B] int32, out_dist [B] fp32: per row, always written.
 *   out_sum[k] = sum_{i: a_i = k} w_i z_i  ([K][C], pitch ld_w),  out_count[k] = the number of such rows (an exact integer
 *   in double),  out_stats[0] = sum_i dist_i,  out_stats[1] = sum_i n2_i  (double [2]).
 * accumulate = 1 adds this call's totals to out_sum, out_count and out_stats (a dataset walked in decode groups).
 * out_sum == NULL (predict only): only out_assign and out_dist are written; out_count and out_stats are not touched and
 * may be NULL.
 * A score's bits depend on (z_i, W_k, b_k, C, metric) alone -- exact fp32 products, fp32 accumulation
 * (v_mfma_f32_32x32x2_f32) in an order fixed by C, one rounding for the scale and one for the add of b -- not on the row's
 * place in a tile, a call or a walker's range, nor on the path: K <= 32 is one kernel (z is read once); K > 32 runs an assign
 * kernel over all centroid tiles, then the sums walk once per centroid tile (the cost of an lla_svm_pass at that K).  The
 * assignment is therefore a pure function of the rows and the centroids.  No floating-point atomics: workgroups leave partial
 * sums in `workspace` (lla_kmeans_pass_workspace_bytes(C, K) bytes; 0 for a refused shape) and a last kernel adds them in
 * workgroup order, counts and statistics in double; the grid depends on (B, K) alone: the same inputs give the same bits.
 * C % 8 == 0, 8 <= C <= 1024, K >= 1, ld_z >= C, ld_w >= C, pitches multiples of 4, metric 0 / 1, z 16-byte (fp16: 8-byte)
 * and W, out_sum, workspace 16-byte aligned; W, b, out_assign, out_dist, workspace not NULL (with out_sum: out_count and
 * out_stats too); anything else is LLA_EINVAL, decided before any device call.  B == 0: LLA_OK, no pass is launched (the
 * accumulated outputs are zeroed unless accumulate is set or out_sum is NULL, then nothing is touched). */
size_t lla_kmeans_pass_workspace_bytes(int C, int K);
int lla_kmeans_pass(const void *z, int z_dtype, int ld_z, int B, int C, const float *W, const float *b, int K, int ld_w,
                    int metric, int32_t *out_assign, float *out_dist, float *out_sum, double *out_count, double *out_stats,
                    int accumulate, void *workspace, void *stream);

/* The second moments of the rows in one pass (lossyless_amd/csrc/gram.hip): the sufficient statistics of a ridge probe on
 * frozen features.  Stands in for `Z.T @ Z`, `Z.sum(0)` and `T.T @ Z` on the decompressed host array that scikit-learn's
 * Ridge / RidgeClassifier would form from the reference's features (the reference itself fits only iterative predictors:
 * LinearSVC in its README, the MLP of lossyless/predictors.py); they do not depend on the penalty and add over rows.
 *   z [B][C] (pitch ld_z; LLA_Z_F32, or LLA_Z_F16 widened exactly); t [B][T] fp32 regression targets (pitch ld_t), or NULL
 *   with T == 0.
 *   out_gram [C][C] = sum_i z_i z_i^T (both triangles written, out_gram[c][d] and out_gram[d][c] from one value),
 *   out_sum [C] = sum_i z_i;  with t: out_cross [T][C] = sum_i t_i z_i^T, out_tsum [T] = sum_i t_i, out_tsq [T] = sum_i t_i^2.
 *   All outputs are double and contiguous.  accumulate = 1 adds this call's totals to them (a dataset walked in groups).
 * Exact fp32 products, fp32 accumulation (v_mfma_f32_32x32x2_f32) along a walker's rows -- a chain is never longer than B --
 * and every sum of chains, the column sums and the target sums in double.  No floating-point atomics: workgroups leave
 * partial tiles in `workspace` (lla_gram_pass_workspace_bytes(C, T) bytes; 0 for a refused shape) and a last kernel adds
 * them in walker order; the grid depends on (B, C, T) alone: the same inputs give the same bits.
 * C % 8 == 0, 8 <= C <= 1024, ld_z >= C and a multiple of 4, z 16-byte (fp16: 8-byte) aligned; t != NULL: 1 <= T <= 4096,
 * ld_t >= T (ANY pitch, not only multiples of 4 as for z: targets are read one by one, so that T == 1 takes a plain [B]
 * vector), t 4-byte aligned.  The cap of 4096 targets bounds the grid and the workspace; the walkers per tile are
 * 512 / (Gram tiles + cross tiles), so once the tiles exceed 512 (C = 1024: T > 1900) every tile has one walker, whose
 * fp32 chain is as long as B and which has no row parallelism: many targets are better passed in several calls; out_gram, out_sum, workspace (with t: out_cross,
 * out_tsum, out_tsq) not NULL and 16-byte aligned; anything else is LLA_EINVAL, decided before any device call.  B == 0:
 * LLA_OK, no kernel is launched (the outputs are zeroed unless accumulate is set). */
size_t lla_gram_pass_workspace_bytes(int C, int T);
int lla_gram_pass(const void *z, int z_dtype, int ld_z, int B, int C, const float *t, int ld_t, int T, double *out_gram,
                  double *out_sum, double *out_cross, double *out_tsum, double *out_tsq, int accumulate, void *workspace,
                  void *stream);

/* Column sums per run of rows (csrc/gram.hip): out [S][C] = sum of z_i over rows seg_offsets[s] <= i < seg_offsets[s + 1], in
 * double.  Stands in for `onehot(Y).T @ Z` of a RidgeClassifier fit on rows sorted by class: the cross-moments of class
 * labels without the one-hot matrix.  seg_offsets is HOST memory: S + 1 ascending offsets, [0] == 0, [S] == B; empty
 * segments are allowed and give zeros.  Eight row lanes per segment add their rows (row = lane mod 8) in row order and are
 * added in lane order: a function of the offsets alone.  z as for lla_gram_pass; S >= 1, out 16-byte aligned; anything else
 * (offsets that descend or do not end at B included) is LLA_EINVAL before any device call.  B == 0: LLA_OK, no kernel
 * (out is zeroed unless accumulate is set). */
int lla_segment_sums(const void *z, int z_dtype, int ld_z, int B, int C, const int32_t *seg_offsets, int S, double *out,
                     int accumulate, void *stream);

/* ---- A training step of the reference's MLP predictor (csrc/mlp.hip): what lla_gemm_f32, the forward half of an fp32
 * Linear layer, lacks.  Everything is fp32, row-major, pitches in elements; v_mfma_f32_32x32x2_f32 (exact fp32 products,
 * fp32 accumulation), no floating-point atomics, the order of every sum fixed by the shape alone (the same inputs give the
 * same bits); refusals are LLA_EINVAL, decided before any device call; a zero-sized call is LLA_OK with no launch. */

/* The input gradient of a Linear layer, with the ReLU backward of the layer below in its epilogue -- what autograd runs for
 * `Linear -> ReLU` of the reference's MLP (lossyless/architectures.py:141-155, trained by lossyless/predictors.py:38-232):
 *   dX[M][K] = dY[M][N] W[N][K],  then dX[i][k] = 0 where H[i][k] > 0 does not hold  (H == NULL: no mask)
 * H [M][K] is the forward OUTPUT of the layer below (relu(a) > 0 iff a > 0; -0.0 and 0.0 mask).  The reduction runs over N:
 * N % 4 == 0 (the caller pads the class dimension with zero columns), K % 4 == 0; ldy >= N, ldw >= K, ldh >= K, ldx >= K;
 * ldy, ldh, ldx multiples of 4 and dY, H, dX 16-byte aligned.  Columns K .. ldx-1 of dX are not written. */
int lla_gemm_f32_nn(const float *dY, int ldy, const float *W, int ldw, const float *H, int ldh, float *dX, int ldx,
                    int M, int N, int K, void *stream);
/* The weight and bias gradients of a Linear layer (the same lines of the reference):
 *   dW[N][K] = dY[M][N]^T X[M][K];   db != NULL: db[n] = sum_i dY[i][n], added in row order.
 * The reduction runs over the batch M, any M >= 1 (the staged operands of a ragged last chunk are zero-filled).  One
 * workgroup owns an output tile over all of M: every element is ONE fma chain in row order, there is no workspace and no
 * second kernel.  N % 4 == 0, K % 4 == 0; ldy >= N, ldx >= K, ldw >= K; ldy, ldx multiples of 4 and dY, X 16-byte aligned.
 * Columns K .. ldw-1 of dW are not written. */
int lla_gemm_f32_tn(const float *dY, int ldy, const float *X, int ldx, float *dW, int ldw, float *db, int M, int N, int K,
                    void *stream);
/* Softmax cross-entropy of a minibatch and its gradient with respect to the logits (F.cross_entropy and its backward:
 * lossyless/predictors.py:172-186; the accuracy of :196-204):
 *   logits [B][ld], the first K columns real;  y [B] int32;  with mx_i = max_k s_ik, se_i = sum_k exp(s_ik - mx_i):
 *   dlogits[i][k] = scale (exp(s_ik - mx_i) / se_i - [y_i = k]) for k < K, and exactly 0 for K <= k < Kpad
 *   *out_loss (double)   = sum_i (mx_i + log se_i - s_{i, y_i})
 *   *out_correct (int32) = the rows whose argmax (the lowest index on ties, as torch.argmax) equals their label.
 * A row whose label lies outside [0, K) gets a zero residual and counts in neither output.  The row maximum is always
 * subtracted; expf / logf, no fast variants; the probability is a quotient, so its error does not grow with |lse| as
 * exp(s - lse) does.  `scale` is the caller's: 1 / (rows of the minibatch with a valid label).  One wave per row; the row
 * losses go through the workspace (lla_softmax_xent_workspace_bytes(B) bytes, 4-byte aligned) and are added in a fixed
 * order in double.  1 <= K <= 1024, K <= Kpad <= ldd, K <= ld.  Columns Kpad .. ldd-1 of dlogits are not written. */
size_t lla_softmax_xent_workspace_bytes(int B);
int lla_softmax_xent(const float *logits, int ld, const int32_t *y, int B, int K, int Kpad, float scale, float *dlogits,
                     int ldd, double *out_loss, int32_t *out_correct, void *workspace, void *stream);
/* One fused update over flat buffers p, g, m, v [n] with the semantics of torch.optim.AdamW (the reference's optimiser:
 * lossyless/predictors.py:206-232, config/optimizer/Adam.yaml / AdamW.yaml):
 *   p <- p (1 - lr wd);  m <- beta1 m + (1 - beta1) g;  v <- beta2 v + (1 - beta2) g^2;
 *   p <- p - (lr / bias_correction1) m / (sqrt(v) / sqrt(bias_correction2) + eps)
 * bias_correction1 = 1 - beta1^t and bias_correction2 = 1 - beta2^t are the host's, in double.  weight_decay = 0 is plain
 * Adam.  m and v are formed in double from the fp32 operands and rounded once; 16-byte loads and stores with a scalar tail
 * for n % 4.  All four pointers 16-byte aligned; lr, eps, weight_decay >= 0, betas in [0, 1), corrections > 0. */
int lla_adamw_step(float *p, const float *g, float *m, float *v, long long n, double lr, double beta1, double beta2,
                   double eps, double weight_decay, double bias_correction1, double bias_correction2, void *stream);

/* ---- BatchNorm1d -> ReLU -> Dropout of the predictor's hidden blocks, training mode (csrc/batchnorm.hip).  The reference's
 * predictor is configured (config/architecture/mlp_probe.yaml) with norm_layer batchnorm and dropout_p 0.2, for which
 * lossyless/architectures.py:137-153 builds each hidden block as Linear(bias=False) -> BatchNorm1d -> ReLU -> Dropout(p).
 * Conventions of the block above: fp32, row-major, pitches in elements, no floating-point atomics, the order of every sum
 * fixed by (B, N) alone, LLA_EINVAL before any device call, a zero-sized call LLA_OK with no launch, no workspace.  Every
 * sum and every element is formed in double and rounded once to fp32.  N % 4 == 0, every pitch >= N and a multiple of 4,
 * every pointer 16-byte aligned; B == 1 is LLA_EINVAL (torch refuses one value per channel in training as well). */

/* Forward of BatchNorm1d (training) -> ReLU -> Dropout (lossyless/architectures.py:143-145,150-152) from the pre-norm
 * activations a [B][lda] (lla_gemm_f32 with bias = NULL).  Per column j:
 *   mean_j = (1/B) sum_i a_ij;  var_j = (1/B) sum_i (a_ij - mean_j)^2  (biased, two-pass);  rstd_j = 1 / sqrt(var_j + eps)
 *   out_ij = keep_ij ? max(gamma_j (a_ij - mean_j) rstd_j + beta_j, 0) s : 0,   s = (float)(1 / (1 - (double)p))
 *   running_mean_j <- (1 - momentum) running_mean_j + momentum mean_j
 *   running_var_j  <- (1 - momentum) running_var_j  + momentum var_j B / (B - 1)        (both NULL: not tracked)
 * mean [N] and rstd [N] are written for lla_bn_bwd; `a` is only read and must differ from `out`.
 * keep_ij: Philox4x32-10 with key (seed & 0xffffffff, seed >> 32) and counter (e & 0xffffffff, e >> 32, step, layer),
 * e = (i N + j) / 4; output word j % 4 gives u = (float)(word >> 8) 2^-24 and keep_ij = (u >= (float)p): a function of
 * (seed, step, layer, i, j) alone.  p == 0 draws nothing and out is the ReLU exactly.  0 <= p < 1, eps >= 0,
 * 0 <= momentum <= 1.  Columns N .. ldo-1 of out are not written. */
int lla_bn_relu_dropout_fwd(const float *a, int lda, const float *gamma, const float *beta, float *out, int ldo,
                            float *mean, float *rstd, float *running_mean, float *running_var, int B, int N, double eps,
                            double momentum, double p, uint64_t seed, uint32_t step, uint32_t layer, void *stream);
/* Backward of the same three modules (what autograd runs for the same lines).  g [B][ldg] is the gradient with respect to
 * `out` already masked by [out > 0] -- lla_gemm_f32_nn with H = out delivers it: out > 0 iff the ReLU passed and the element
 * was kept -- so only the factor s is missing.  With gh = s g and xhat = (a - mean) rstd (a, mean, rstd of the forward):
 *   dbeta_j = sum_i gh_ij;   dgamma_j = sum_i gh_ij xhat_ij;
 *   da_ij = gamma_j rstd_j (gh_ij - dbeta_j / B - xhat_ij dgamma_j / B)
 * da [B][ldda] may be g itself (in place) and must differ from a.  Columns N .. ldda-1 of da are not written. */
int lla_bn_bwd(const float *g, int ldg, const float *a, int lda, const float *gamma, const float *mean, const float *rstd,
               double p, float *dgamma, float *dbeta, float *da, int ldda, int B, int N, void *stream);

/* ---- Training pass of the factorized rate estimator over frozen features (csrc/eb_train.hip): what autograd runs for
 * HRateFactorizedPrior in training mode (lossyless/rates.py:534-554; compressai 1.1.5 EntropyBottleneck with filters (3, 3, 3, 3),
 * uniform noise in place of rounding) and the lossy_Z distortion with p_norm 1 (lossyless/distortions.py:408-449), as
 * lossyless/learnable_compressors.py:241-275 combines them.  Conventions of the blocks above: LLA_EINVAL before any device call,
 * a zero-row call LLA_OK with no launch, no floating-point atomics, the order of every sum a function of (B, C) alone (the same
 * inputs give the same bits).  fp32 arithmetic with expf / logf / log1pf / expm1f / tanhf (no fast variants), products and sums
 * rounded separately; sums over rows in fp32 per walker (at most ceil(B / W) terms), over walkers and channels in double.
 *
 * `params` [58][C] fp32, params[k * C + c] for channel c, k in the order: _matrix0 (3: [j][0]), _matrix1, _matrix2, _matrix3 (9
 * each, row-major [out j][in i]), _matrix4 (3: [0][i]), _bias0 .. _bias3 (3 each), _bias4 (1), _factor0 .. _factor3 (3 each).
 * `scaling`, `biasing` [C].  With s = scaling[c], b = biasing[c], for row i and channel c:
 *   y = (z_ic + b) exp(s);  v = y + u_ic;  L(x): x <- softplus(M_k) x + B_k, then x <- x + tanh(F_k) tanh(x) for k < 4
 *   lower = L(v - .5), upper = L(v + .5), sgn = -sign(lower + upper) (a constant of the backward)
 *   lik = max(|sigmoid(sgn upper) - sigmoid(sgn lower)|, 1e-9), the gradient passing through the bound (compressai's LowerBound
 *   blocks only a gradient that would lower a value at the bound; d(-log lik)/d lik < 0)
 *   rate_i = -sum_c log lik_ic (nats);  dist_i = sum_c |u_ic exp(-s) + 1e-6|  (= nn.PairwiseDistance(p=1) of z_hat = v / exp(s) - b
 *   and z: z_hat - z = u exp(-s) in closed form, so d dist / d b = 0 and d dist / d s = -sign(.) u exp(-s))
 * One formula each: softplus(m) = max(m, 0) + log1p(exp(-|m|)) (derivative sigmoid(m) = 1 / (1 + exp(-m)) evaluated from
 * exp(-|m|)); the sigmoid difference, for a = sgn upper and b = sgn lower (a + b <= 0), is
 * -exp(max(a, b)) expm1(-|a - b|) / ((1 + exp(a)) (1 + exp(b))) signed as a - b when both are <= 0 (two tail values do not cancel)
 * and sigmoid(a) - sigmoid(b) otherwise; sigmoid'(t) = e / (1 + e)^2 with e = exp(-|t|); the rate term is -logf of the BOUNDED
 * likelihood.
 * Noise: Philox4x32-10 as lla_bn_relu_dropout_fwd, key (seed & 0xffffffff, seed >> 32), counter (e & 0xffffffff, e >> 32, step,
 * 0x6e6f6973), e = (i C + c) / 4, output word c % 4: u = (float)(word >> 8) 2^-24 - 0.5f in [-0.5, 0.5): a function of
 * (seed, step, i, c) alone.  C % 4 == 0.
 * z [B][ldz] fp16 or fp32 (LLA_Z_F16 / LLA_Z_F32), ldz >= C in elements, aligned to its element; columns C .. ldz-1 are not read.
 * grads [2][60 C] fp32: grads[0] the gradient of sum_i dist_i, grads[1] of sum_i rate_i, each in the layout of the main
 * optimiser's buffer -- scaling [C], biasing [C], then the 58 C of `params` (so scaling, biasing and params may be three
 * pieces of ONE buffer that lla_adamw_step updates); the caller forms (grads[0] + beta grads[1]) / B.  out_sums [2] doubles:
 * sum_i dist_i, sum_i rate_i.  workspace: lla_eb_train_pass_workspace_bytes(B, C) bytes (0 for a refused shape), contents
 * irrelevant.  params, scaling, biasing, grads, workspace 16-byte aligned, out_sums 8-byte. */
size_t lla_eb_train_pass_workspace_bytes(int B, int C);
int lla_eb_train_pass(const void *z, int z_dtype, size_t ldz, int B, int C, const float *params, const float *scaling,
                      const float *biasing, uint64_t seed, uint32_t step, float *grads, double *out_sums, void *workspace,
                      void *stream);
/* The auxiliary loss of the same module (compressai EntropyBottleneck.loss(); lossyless/learnable_compressors.py:293-295) and
 * its gradient with respect to the quantiles, the network held constant:
 *   aux = sum_c sum_k |L_c(q_c[k]) - target[k]|;   grad_q[c][k] = sign(L_c(q_c[k]) - target[k]) dL_c/dx (q_c[k])
 * with the device functions of the pass (dL/dx is the input derivative the pass needs for scaling and biasing).  params as
 * above; quantiles, grad_q [C][3] fp32 (16-byte aligned), target [3] fp32; *out_loss a double, the channels' losses added in
 * channel order (runs of 8 channels, then the runs).  C % 4 == 0. */
int lla_eb_aux_grad(const float *params, const float *quantiles, const float *target, int C, float *grad_q, double *out_loss,
                    void *stream);

/* ---- Training passes of the scale-hyperprior rate estimator over frozen features (csrc/hyperprior_train.hip): what autograd
 * runs for HRateHyperprior in training mode (lossyless/rates.py:631-678, :428-438; lossyless/learnable_compressors.py:241-303;
 * compressai 1.1.5 EntropyBottleneck and GaussianConditional with uniform noise in place of rounding) around its two MLPs,
 * which run on lla_gemm_f32 / lla_gemm_f32_tn / lla_gemm_f32_nn.  For a minibatch z [B][C], S = side_z_dim:
 *   y = (z + biasing) exp(scaling);  x = side_encoder(y);  s_hat = x + u_s;  lik_s as lla_eb_train_pass's lik (no affine)
 *   gp = z_encoder(s_hat): scales = gp[:, 0..C-1], means = gp[:, C..2C-1];  v = y + u_z;  t = |v - means|;  sc = max(scales, bound)
 *   lik_z = max(Phi((.5 - t) / sc) - Phi((-.5 - t) / sc), 1e-9),  Phi(a) = 0.5 erfc(-a / sqrt 2)
 *   rate_i = -sum log lik_s - sum log lik_z (nats);  dist_i = sum_c |u_z exp(-scaling) + 1e-6|  (the closed form of the block above)
 *   loss = mean_i dist_i + beta_t mean_i rate_i
 * Both LowerBounds follow compressai: a gradient passes where the value is at or above the bound, or where the gradient is
 * negative.  d(-log lik) / d lik < 0 always passes; the scale's bound blocks.  sign(0) = 0 for |.| at v == means.
 * Conventions of the block above: LLA_EINVAL before any device call, a zero-row call LLA_OK with no launch, no floating-point
 * atomics, the order of every sum a function of the shape alone, fp32 arithmetic with expf / logf / erfcf / tanhf / log1pf /
 * expm1f (no fast variants), products and sums rounded separately; sums over rows in fp32 per walker, over walkers and channels in
 * double.  `scale` is the caller's beta_t / B: the passes multiply the rate's gradients by it (per element in fp32 for the
 * activations' gradients; once, in double, on the summed parameter gradients).
 * Noise: element f = i cols + c of a [rows][cols] matrix draws Philox4x32-10 with key (seed & 0xffffffff, seed >> 32) and counter
 * (f / 4 & 0xffffffff, f / 4 >> 32, step, tag), output word f % 4, u = (float)(word >> 8) 2^-24 - 0.5f; tag 0x6e6f6973 for u_z
 * (cols = C: for C % 4 == 0 the stream of lla_eb_train_pass to the bit), 0x73696465 for u_s (cols = S). */

/* The side information's bottleneck, forward and backward, for ANY S >= 1.  x [B][ldx] fp32 (the side encoder's output; columns
 * S .. ldx-1 are not read), params [58][S] in the order of lla_eb_train_pass.  Writes
 *   s_hat [B][lds] = x + u_s (columns S .. lds-1: 0 -- the next GEMM reads them);  dx [B][ldd] = scale d(sum_i rate_s) / dx
 *   (columns S .. ldd-1: 0);  grads [58 S] = scale d(sum_i rate_s) / d params;  *out_sum (double) = sum_i rate_s.
 * workspace: lla_eb_side_pass_workspace_bytes(B, S) bytes (0 for a refused shape).  ldx, lds, ldd >= S; x, s_hat, dx 4-byte,
 * params, grads, workspace 16-byte, out_sum 8-byte aligned. */
size_t lla_eb_side_pass_workspace_bytes(int B, int S);
int lla_eb_side_pass(const float *x, int ldx, int B, int S, const float *params, uint64_t seed, uint32_t step, float scale,
                     float *s_hat, int lds, float *dx, int ldd, float *grads, double *out_sum, void *workspace, void *stream);
/* lla_eb_aux_grad for any S >= 1 (the same kernel: the same bits where both accept the shape). */
int lla_eb_aux_grad_any(const float *params, const float *quantiles, const float *target, int S, float *grad_q,
                        double *out_loss, void *stream);
/* The affine, the Gaussian conditional likelihood and the distortion, forward and backward.  z [B][ldz] fp16 or fp32 as
 * lla_eb_train_pass reads it; gp [B][ldg] fp32, ldg >= 2C; scale_bound > 0 (compressai: 0.11).  Writes
 *   y [B][ldy] fp32 = (z + biasing) exp(scaling), the side encoder's input (columns C .. ldy-1: 0)
 *   dgp [B][ldg] = scale d(sum_i rate_z) / d(scales | means), the scale half through the bound rule (columns 2C .. ldg-1: 0)
 *   dy [B][ldy] = scale d(sum_i rate_z) / dy (columns C .. ldy-1: 0)
 *   g_dist [C] = d(sum_i dist_i) / d scaling, NOT scaled;  out_sums [2] doubles: sum_i dist_i, sum_i rate_z.
 * With a_u = (.5 - t) / sc, a_l = (-.5 - t) / sc and phi(a) = exp(-a^2 / 2) / sqrt(2 pi), evaluated as
 * expf(-0.5f (a a)) 0.39894228f:  d lik / dt = -(phi(a_u) - phi(a_l)) / sc,  d lik / d sc = -(a_u phi(a_u) - a_l phi(a_l)) / sc,
 * dt / dv = -dt / d means = sign(v - means); Phi as 0.5f erfcf(-0.70710678f a); the rate term is -logf of the BOUNDED likelihood
 * and its seed -1 / lik.  gp == NULL is the prologue: y alone is written (its pad columns included) and dgp, dy, g_dist,
 * out_sums, workspace are not touched -- y has to exist before the side encoder runs, gp only after the z encoder has.
 * workspace: lla_gaussian_train_pass_workspace_bytes(B, C) bytes.  z aligned to its element; gp, dgp, y, dy 4-byte; scaling,
 * biasing, g_dist, workspace 16-byte; out_sums 8-byte. */
size_t lla_gaussian_train_pass_workspace_bytes(int B, int C);
int lla_gaussian_train_pass(const void *z, int z_dtype, size_t ldz, int B, int C, const float *scaling, const float *biasing,
                            const float *gp, int ldg, float scale_bound, uint64_t seed, uint32_t step, float scale, float *dgp,
                            float *y, int ldy, float *dy, float *g_dist, double *out_sums, void *workspace, void *stream);
/* The affine's gradient from dy_total [B][ld] = d loss / dy (the Gaussian pass's dy plus the side encoder's input gradient)
 * and y [B][ldy]:
 *   g_scaling[c] = sum_i dy_total_ic y_ic (+ add_scale add_scaling[c] when add_scaling != NULL: the distortion's share,
 *   g_dist / B, added in double before the one rounding);   g_biasing[c] = exp(scaling[c]) sum_i dy_total_ic
 * (dy / d scaling = y, dy / d biasing = exp(scaling)).  Walker partials in fp32, added in double in walker order.
 * workspace: lla_affine_grad_workspace_bytes(B, C) bytes.  dy_total, y 4-byte; the [C] vectors and workspace 16-byte aligned. */
size_t lla_affine_grad_workspace_bytes(int B, int C);
int lla_affine_grad(const float *dy_total, int ld, const float *y, int ldy, const float *scaling, int B, int C,
                    const float *add_scaling, float add_scale, float *g_scaling, float *g_biasing, void *workspace, void *stream);

/* out[n][H][W][ldc] (first cout channels) = relu(conv3x3(in, stride 1, pad 1) + bias) as an IMPLICIT GEMM:
 * `in` is NHWC fp16 [n][H][W][pitch] (first cin channels used; cin % 64 == 0, or cin == 32), weights fp16
 * [cout][K] with K = 9 cin rounded up to a multiple of 64 (zero padded) in the order (kh, kw, c), bias fp32
 * [cout] (BatchNorm folded in), cout % 128 == 0 (weight rows; ldc < cout, a multiple of 32, stores only the
 * first ldc channels).  The A operand is
 * gathered by the GEMM's LDS-DMA loader (out-of-image taps read a zero line): no im2col matrix.  Stands in
 * for `conv2 -> bn2 -> relu` of clip's Bottleneck (clip/model.py as loaded at lossyless/architectures.py:367-371). */
int lla_conv3x3_relu_f16(const void *in, int n, int H, int W, int pitch, int cin, const void *weights,
                         const float *bias, void *out, int ldc, int cout, void *stream);
/* The same convolution for the tower's NARROW layers -- (cin, cout) = (32, 32), (32, 64), (64, 64); H, W multiples of 8 --
 * as a direct convolution (csrc/conv_direct.hip: one 8 x 8 output tile per wave, the 10 x 10 halo in LDS once, weights
 * resident), bit-identical to lla_conv3x3_relu_f16 on the same operands (`weights` as there, rows of `kpad` halfs; ldc >=
 * cout).  pool != 0 (32 -> 64 only): the 2 x 2 average pool that follows the stem's third convolution is applied in the
 * epilogue and `out` is [n][H/2][W/2][ldc] -- the bytes conv + avgpool write as two kernels.  LLA_EINVAL for any other
 * shape (the caller falls back to the implicit GEMM). */
int lla_conv3x3_direct_relu_f16(const void *in, int n, int H, int W, int pitch, int cin, const void *weights, int kpad,
                                const void *bias, void *out, int ldc, int cout, int pool, void *stream);
/* One WHOLE bottleneck of the RN50 tower's layer1 in one kernel (csrc/bottleneck_fused.hip; clip/model.py Bottleneck as loaded at
 * lossyless/architectures.py:367-371, stride 1, no downsample): out = relu(conv3(relu(conv2(relu(conv1(x))))) + x) for x = NHWC
 * fp16 [n][H][W][pitch] (first cin = 256 channels; or 64, below), H and W multiples of 14; conv1 weights fp16 [64][k1pad] (K = cin), conv2
 * [64][k2pad] (K = 9 * 64 in the order (kh, kw, c)), conv3 [256][k3pad] (K = 64), biases fp32 (BatchNorm folded in); out NHWC
 * fp16 [n][H][W][ldo] (first 256 channels), which must not overlap x.  The 64-channel intermediates are rounded to fp16 as the
 * three-kernel path rounds them, but stay in LDS.  cin = 64 is the stage's FIRST block: no identity, and `w3` [256][k3pad] is the
 * one 1x1 convolution over [conv2's output (64) | x (64)] that conv3 and the downsample convolution fold into (K = 128, bias b3 +
 * bds: lla_rn50_fused_desc(0)).  LLA_EINVAL for any other shape (the caller then runs the three kernels). */
int lla_rn50_bottleneck_f16(const void *x, int n, int H, int W, int pitch, int cin, const void *w1, int k1pad, const void *b1,
                            const void *w2, int k2pad, const void *b2, const void *w3, int k3pad, const void *b3, void *out,
                            int ldo, void *stream);
/* The tower's first convolution (clip/model.py ModifiedResNet.conv1 + bn1 + relu): out[n][H/2][W/2][ldc] (first 32
 * channels) = relu(conv3x3(in, stride 2, pad 1) + bias) for in = NHWC fp16 [n][H][W][3] (pitch 3), H, W multiples of 16;
 * weights fp16 [32][kpad] with K = 27 in the order (kh, kw, c), zero padded; bias fp32 [32].  Direct (csrc/conv_direct.hip),
 * bit-identical to the im2col matrix + lla_gemm_f16_ex it replaces. */
int lla_conv3x3_rgb_s2_relu_f16(const void *in, int n, int H, int W, const void *weights, int kpad, const void *bias,
                                void *out, int ldc, void *stream);
/* Patch embedding alone (conv1 of the tower as a GEMM that gathers 32x32 patches in place, plus the
 * positional embedding): x[b*50 + 1 + t][:] = patch(b, t) . conv_w^T + pos[1 + t] for t < 49; class
 * rows (t = -1) are not written.  images fp16 in `layout`; conv_w fp16 [768][3072] with K ordered
 * (kh,kw,c) for NHWC / (c,kh,kw) for NCHW (LLA_VIT_CONV1_*); pos fp32 [50][768]; x fp32 [B*50][768].
 * Same kernel instantiations lla_vit_b32_forward launches first. */
int lla_patch_embed_f16(const void *images, int layout, int B, const void *conv_w, const float *pos,
                        float *x, void *stream);
/* y16[r][:] = LayerNorm(x32[r*row_stride : +768]) * w + b, eps 1e-5. */
int lla_layernorm768(const float *x, size_t row_stride, const float *w, const float *b,
                     void *y16, int rows, void *stream);
/* The tower's residual GEMM with the LayerNorm that follows in its epilogue (out-proj + ln_2, c_proj + ln_1 of the next
 * block: clip ResidualAttentionBlock, hub/compressor.py:93), as the tower's layer loop launches it:
 *   x[M][768] (fp32, in place) += A[M][K] (fp16, row stride lda) * W[768][K]^T (fp16) + bias (fp32 [768] or NULL)
 *   h16[M][768] (fp16) = LayerNorm(x) * gamma + beta, eps 1e-5 -- the bits lla_layernorm768 gives on the updated x
 * on the four-wave kernel, followed by the clean-up kernel (walking the other way) for the row tiles whose three column
 * tiles did not find each other's partial sums in time.  wait_cycles: as LLA_TOWER_OPT_LNX_WAIT (the tower's default is
 * 24000; 0: look once; < 0: every row tile through the clean-up kernel; every wait is bounded).  rev 0 / 1: first / last
 * rows first.  Every combination gives the same bits.
 * M % 256 == 0 (M = 256, one row tile, is valid), 256 <= K, K % 64 == 0, lda >= K, lda % 8 == 0, M * 768 < 2^32 and the
 * operands within 32-bit byte offsets (M * lda < 2^31): exactly the shapes lla_gemm_plan answers LLA_OK to for epi 9,
 * N = ldc = 768.  All pointers 16-byte aligned.  Anything else is LLA_EINVAL, decided before any device call.
 * workspace [dev] lla_gemm_resid_layernorm768_workspace_bytes(M) bytes (0 for a refused M), contents irrelevant: the call
 * zeroes the words it reads before it writes them and tags what it publishes with an epoch of its own. */
size_t lla_gemm_resid_layernorm768_workspace_bytes(int M);
int lla_gemm_resid_layernorm768(const void *A, int lda, const void *W, const float *bias, float *x, const float *gamma,
                                const float *beta, void *h16, int M, int K, int wait_cycles, int rev, void *workspace,
                                void *stream);
/* qkv fp16 [B*50][2304] -> o fp16 [B*50][768]; 12 heads of 64, softmax(QK^T/8)V. */
int lla_attention50(const void *qkv, void *o, int B, void *stream);
/* lla_layernorm768 / lla_attention50 with the walk the tower uses on every second slice: rev 0 = first rows (images)
 * first, 1 = last first; the same bits either way.  Any other rev is LLA_EINVAL. */
int lla_layernorm768_ex(const float *x, size_t row_stride, const float *w, const float *b, void *y16, int rows, int rev,
                        void *stream);
int lla_attention50_ex(const void *qkv, void *o, int B, int rev, void *stream);
/* The tower's token assembly as lla_vit_b32_forward launches it, over x fp32 [rows][768] whose rows r % 50 != 0 hold
 * patch embedding + positional embedding (lla_patch_embed_f16):
 *   x[r] = ln_pre(r % 50 == 0 ? cls + pos[0] : x[r]) (fp32, in place; the class rows of x are not read)
 *   h16[r] (fp16) = ln_1 of block 0 of that x[r]  -- the bits lla_layernorm768 gives on the x written
 * cls fp32 [768], pos fp32 [>= 768] (row 0 of the positional embedding), wpre / bpre / w1 / b1 fp32 [768], eps 1e-5.
 * rows < 0, or a NULL pointer with rows > 0: LLA_EINVAL.  rows == 0: LLA_OK, nothing launched. */
int lla_ln_pre_ln1_768(float *x, const float *cls, const float *pos, const float *wpre, const float *bpre, const float *w1,
                       const float *b1, void *h16, int rows, void *stream);

/* ------------------------------------------------------------------------- *
 * Device entry point: CLIP RN50 visual tower
 *   stands in for  clip.load("RN50")[0].visual  as the reference's pretrained featuriser loads it
 *   (lossyless/architectures.py:367-371; clip==1.0 ModifiedResNet + AttentionPool2d, output 1024).
 * The weight blob holds, per convolution in execution order (stem conv1..3; per bottleneck conv1,
 * conv2, conv3 and, in the first block of a stage, the downsample convolution), the BatchNorm-folded
 * weights fp16 [npad][kpad] with K ordered (kh, kw, c) and zero padding, and the folded bias fp32
 * [npad]; then the attention pool's positional embedding fp32 [50][2048], q_proj fp16 [2048][2048] +
 * bias, (k_proj ; v_proj) fp16 [4096][2048] + bias, c_proj fp16 [1024][2048] + bias.
 * lla_rn50_conv_desc(i, out8) -> {cin, cout, ksize, stride, kpad, npad, weight offset, bias offset};
 * lla_rn50_attnpool_offsets(out7) -> byte offsets of {pos, q_w, q_b, kv_w, kv_b, c_w, c_b}.
 * ------------------------------------------------------------------------- */
size_t lla_rn50_weights_bytes(void);
int lla_rn50_conv_count(void);
int lla_rn50_conv_desc(int i, int64_t *out8);
/* First block of stage `stage` (0..3): conv3 and the downsample convolution run as ONE 1x1 convolution over the
 * concatenated inputs [main path | block input] (no identity tensor): out8 = {cin = planes + inplanes, cout = 4 planes,
 * planes, inplanes, kpad, npad, weight offset, bias offset}; weights fp16 [npad][kpad] = [W3 | Wds] (BatchNorm folded,
 * each rounded to fp16 on its own), bias fp32 [npad] = b3 + bds. */
int lla_rn50_fused_desc(int stage, int64_t *out8);
int lla_rn50_attnpool_offsets(int64_t *out7);
size_t lla_rn50_workspace_bytes(int chunk);
/* images [dev] fp16 NHWC [B][224][224][3], CLIP-normalised; z_out [dev] fp16 [B][1024].  With a tower
 * handle (may be NULL: everything on `stream`), from 32 images on the batch is cut in two slices that
 * alternate between the handle's two lanes (see lla_vit_b32_forward_lanes) when the workspace holds two
 * slices (lla_rn50_workspace_bytes returns that size); joined back into `stream` before returning. */
int lla_rn50_forward(const void *images_nhwc_f16, int B, const void *weights, void *workspace,
                     size_t workspace_bytes, int chunk, void *z_out, void *stream, void *tower);
/* The tower's pooling kernels on their own, as lla_rn50_forward launches them (all fp16, fp32 arithmetic, one rounding):
 * 2x2 average pool (clip/model.py Bottleneck.avgpool and the downsample's AvgPool2d): in NHWC [n][H][W][pitch] (first C
 * channels) -> out [n][H/2][W/2][out_pitch] (first C channels; the others are not written).  H, W even; C, pitch, out_pitch
 * multiples of 8, pitch >= C, out_pitch >= C; in and out 16-byte aligned and not NULL: anything else is LLA_EINVAL. */
int lla_rn50_avgpool2_f16(const void *in, int n, int H, int W, int pitch, int C, void *out, int out_pitch, void *stream);
/* AttentionPool2d's tokens: x [B][49][2048], pos fp32 [50][2048] -> tok [B][50][2048]:
 * tok[b][0] = mean_j x[b][j] + pos[0], tok[b][1 + j] = x[b][j] + pos[1 + j]. */
int lla_rn50_attnpool_tokens_f16(const void *x, const float *pos, void *tok, int B, void *stream);
/* AttentionPool2d's single-query attention, 32 heads of 64: q [B][2048], kv [B * 50][4096] (k | v) -> o [B][2048] =
 * softmax(q k^T / 8) v per head. */
int lla_rn50_attnpool_attend_f16(const void *q, const void *kv, void *o, int B, void *stream);

/* ------------------------------------------------------------------------- *
 * CLIP text tower (csrc/text_tower.hip): the kernels of  clip/model.py CLIP.encode_text  that are not Linear layers
 *   x = token_embedding(text) + positional_embedding;  x = transformer(x)  (pre-LN residual blocks, causal
 *   nn.MultiheadAttention, QuickGELU MLP);  x = ln_final(x);  x[arange, text.argmax(-1)] @ text_projection
 * as the reference calls it on captions (utils/data/images.py:1299-1323).  The Linear layers (in_proj, out_proj, c_fc,
 * c_proj, and text_projection as a bias-free Linear on its transpose) run on lla_gemm_f32.  Everything is fp32, row-major;
 * no floating-point atomics; the order of every sum is fixed by the row's own length, so a prompt's values do not depend
 * on the batch size or on its place in the batch.  Refusals are LLA_EINVAL, decided before any device call; a call with
 * no rows is LLA_OK with no launch.
 * ------------------------------------------------------------------------- */

/* x[p*T + t][:] = tok_emb[tokens[p][t]][:] + pos[t][:]  (one fp32 sum).  tokens int32 [P][T], tok_emb [V][D], pos [T][D]
 * (the first T rows of the positional embedding), x [P*T][D].  The caller checks that the ids lie in [0, V); the kernel
 * clamps the index to that range, so nothing outside tok_emb is ever read.  D % 4 == 0, tok_emb / pos / x 16-byte aligned. */
int lla_text_embed(const int32_t *tokens, int P, int T, const float *tok_emb, int V, const float *pos, int D, float *x,
                   void *stream);
/* Row LayerNorm (clip/model.py LayerNorm on fp32): y[r] = (x[r] - mean) * rstd * w + b with
 *   mean = (1/D) sum_c x[r][c];  var = (1/D) sum_c (x[r][c] - mean)^2  (two-pass);  rstd = 1 / sqrtf(var + eps)
 * x [rows] rows of D at pitch row_stride, y at pitch y_stride (elements, >= D; y may be x).  One wave per row: lane l adds
 * its elements l, l + 64, ... in index order, the 64 lane sums go through one fixed tree.  D % 64 == 0, 64 <= D <= 1024.
 * lla_layernorm768 (fp16 output, the image tower's) is another kernel and is unchanged. */
int lla_layernorm_rows(const float *x, size_t row_stride, const float *w, const float *b, float *y, size_t y_stride, int rows,
                       int D, float eps, void *stream);
/* Causal multi-head attention of the text transformer (nn.MultiheadAttention with attn_mask = triu(-inf, 1)):
 * qkv [P*T][3D] = q | k | v per row as in_proj_weight produces it, D = 64 heads, head dimension 64; o [P*T][D].
 * Per prompt, head and query row i:
 *   s_ij = (q_i . k_j) / 8 for j <= i (an fmaf chain over the 64 dimensions in index order; keys j > i take no part in
 *   row i: the kernel walks j up to its wave's last row, so it reads them from LDS and discards what it computed);  m_i = max_j s_ij;  e_ij = expf(s_ij - m_i);  p_ij = e_ij / sum_{j <= i} e_ij (sum in
 *   increasing j);  o_i = sum_{j <= i} p_ij v_j in increasing j  (row 0 is v_0 exactly).
 * 1 <= T <= 77, heads >= 1, qkv and o 16-byte aligned. */
int lla_attention_causal(const float *qkv, float *o, int P, int T, int heads, void *stream);
/* The two pointwise steps between the GEMMs, over n contiguous floats:
 *   mode 0  x[e] += y[e]                                   (the residual; x and y must not overlap)
 *   mode 1  y[e] = y[e] * sigmoid(1.702f * y[e]),  sigmoid(t) = 1 / (1 + expf(-t))    (QuickGELU, in place; x is not used)
 * x (mode 0) and y 16-byte aligned; any other mode is LLA_EINVAL. */
int lla_text_pointwise(float *x, float *y, long long n, int mode, void *stream);
/* out[r][:] = z[r][:] / |z[r]|_2 for C columns at pitches ld_z / ld_out (elements); a row of zeros gives zeros.  The
 * normalisation of ZeroShotProbe (the image side of CLIP's cosine logits): one wave per row, lane l adds the squares of
 * elements l, l + 64, ... in index order, the lane sums go through one fixed tree; sqrtf, one division per element. */
int lla_unit_rows(const float *z, size_t ld_z, float *out, size_t ld_out, int rows, int C, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* LOSSYLESS_AMD_H */
