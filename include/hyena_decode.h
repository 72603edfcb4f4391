/* hyena_decode.h -- C ABI of the incremental (one position per call) Hyena operator step (same library, libhyena_fftconv.so;
 * kernels in hyena_dna_amd/csrc/decode_kernels.h).
 *
 * Order 2, one head, one block, inner factor 1, short_filter_order 3 (the fused route of HyenaOperator).  One call of each entry point
 * advances ALL B sequences by one position t; t is read from device memory (`pos`, one int) by every kernel and advanced by
 * hyena_decode_post, so a captured graph of the three calls serves every position.  A position outside [0, Lcap) makes the kernels do
 * nothing (and the position stays where it is).
 *
 *   x    : in_proj output of position t WITHOUT its bias, element (c, b) at b ldx + c (ldx >= 3D), `dtype`
 *   bin  : (3D,) fp32 in_proj bias or NULL;  w : (3D, 3) fp32 short-filter taps;  b : (3D,) fp32 short-filter bias
 *   tail : (3D, Bcap, 2) fp32, the raw x of positions t - 2, t - 1 (what the prefill leaves; values before position 0 are not read)
 *   vg   : the history of the convolution's input v * x1, (Bcap, D, lda) `dtype`, row (b, d) at (b D + d) lda, lda >= Lcap, lda % 8 == 0,
 *          16-byte aligned; column t is written by hyena_decode_pre
 *   x0   : (B, D) fp32, the gate of position t (pre writes, post reads)
 *   k    : (D, ldk) fp32 filter (column j = tap j: HyenaFilter.filter_dl(Lcap)), ldk >= Lcap, ldk % 4 == 0, 16-byte aligned
 *   part : hyena_decode_partial_floats(B, D, Lcap) fp32 of scratch, [chunk][B][D] partial sums (no atomics: results are deterministic)
 *   fb   : (D,) fp32 filter bias or NULL;  z : (B, D) `dtype`, the out_proj operand of position t
 * 1 <= B <= Bcap, 1 <= Lcap <= 2^20.  Bad arguments return HYENA_ERR_BAD_ARG before anything is launched.  Asynchronous on `stream`.
 *
 * Per-row positions (hyena_decode_*_rows): the same three calls for a batch whose sequences stand at different positions.  `pos` points
 * at B ints in device memory, row b is advanced from t_b = pos[b]: hyena_decode_pre_rows writes column t_b of row b's history,
 * hyena_decode_conv_rows sums over s <= t_b (one partial per (chunk, b, d) with chunk * 8192 <= t_b; the other slots of `part` are neither
 * written nor read), hyena_decode_post_rows reads those partials and vg[b, d, t_b] and then advances pos[b] by one.  A row whose t_b is
 * outside [0, Lcap) is parked: its z row, history, tail and position stay as they are, the other rows advance.  History columns past t_b
 * of row b must hold finite values (they may be read and are multiplied by a zero tap).  All other arguments, their checks and the
 * stream semantics are those above; with all pos[b] equal the results equal the single-position entry points' bit for bit. */
#ifndef HYENA_DECODE_H
#define HYENA_DECODE_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

size_t hyena_decode_partial_floats(int B, int D, int Lcap);
/* short conv of position t, vg[:, :, t] = x1c * vc, x0 = x0c, tail shifted */
int hyena_decode_pre(const void* x, int ldx, const float* bin, const float* w, const float* b, float* tail, void* vg, float* x0, const int* pos,
                     int B, int Bcap, int D, int Lcap, int lda, int dtype, void* stream);
/* part[chunk][b][d] = sum over the chunk's s <= t of k[d, t - s] vg[b, d, s] */
int hyena_decode_conv(const float* k, int ldk, const void* vg, float* part, const int* pos, int B, int D, int Lcap, int lda, int dtype,
                      void* stream);
/* z = round(round(sum_chunks part + fb vg_t) * x0); then *pos = t + 1 */
int hyena_decode_post(const float* part, const void* vg, const float* fb, const float* x0, void* z, int* pos, int B, int D, int Lcap, int lda,
                      int dtype, void* stream);

/* the three calls above with one position per row: pos points at B ints (see the header comment) */
int hyena_decode_pre_rows(const void* x, int ldx, const float* bin, const float* w, const float* b, float* tail, void* vg, float* x0,
                          const int* pos, int B, int Bcap, int D, int Lcap, int lda, int dtype, void* stream);
int hyena_decode_conv_rows(const float* k, int ldk, const void* vg, float* part, const int* pos, int B, int D, int Lcap, int lda, int dtype,
                           void* stream);
int hyena_decode_post_rows(const float* part, const void* vg, const float* fb, const float* x0, void* z, int* pos, int B, int D, int Lcap,
                           int lda, int dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HYENA_DECODE_H */
