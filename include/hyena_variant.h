/* hyena_variant.h -- C ABI of the edited-window step of the order-2 Hyena operator: M windows of T positions that replace positions
 * [pos[m], pos[m] + T) of a reference sequence whose activations are known (same library, libhyena_fftconv.so; kernels in
 * hyena_dna_amd/csrc/variant_kernels.h).
 *
 * The long convolution is linear in its input vg = v * x1, so below an edit at position p nothing changes and from p on
 *     y_alt[t] = y_ref[t] + sum_{s = p .. t} k[t - s] delta[s] + fb delta[t],        delta[s] = vg_alt[s] - vg_ref[s]
 * Two calls per layer between the in_proj and out_proj GEMMs; no history is read.  1 <= T <= HYENA_VARIANT_TMAX.
 *
 *   x3     : (M, T, ldx) `dtype`, the in_proj output of the window rows WITHOUT its bias, element (m, i, c) at (m T + i) ldx + c, ldx >= 3D
 *   bin    : (3D,) fp32 in_proj bias or NULL;  w : (3D, 3) fp32 short-filter taps;  b : (3D,) fp32 short-filter bias
 *   tail   : (3D, M, 2) fp32, the reference's raw in_proj outputs at pos[m] - 2 and pos[m] - 1 (a value whose position lies before 0 is
 *            never used: it may hold anything)
 *   pos    : (M,) int32 in DEVICE memory, the absolute position of every window's first row.  The short convolution pads with zeros in
 *            front of position 0 -- decode_pre's rule, applied to pos[m] + i
 *   vg_ref : (M, D, T) `dtype`, the reference's convolution input over the window, row (m, d) at (m D + d) T
 *   x0     : (M, T, D) fp32, the gate (pre writes, conv reads), element (m, i, d) at (m T + i) D + d
 *   delta  : (M, D, T) fp32 (pre writes, conv reads) = float(round_dtype(v * x1)) - float(vg_ref): the new convolution input is rounded to
 *            `dtype` first, as the forward stores it
 *   y_ref  : (M, D, T) fp32, the reference's long-convolution output (bias term included) over the window
 *   k      : (D, ldk) fp32 filter, column j = tap j, ldk >= T;  fb : (D,) fp32 filter bias or NULL
 *   z      : (M, T, D) `dtype`, the out_proj operand:
 *            z[m, i, d] = round(round(y_ref[m, d, i] + sum_{j <= i} k[d, i - j] delta[m, d, j] + fb[d] delta[m, d, i]) * x0[m, i, d])
 *            -- fp32 accumulation, the terms of an output in ascending j, then + y_ref, then the fb term as one FMA, then the two roundings
 *            hyena_decode_post makes.  The order depends on T alone: no atomics, no scratch, results are deterministic and a window's result
 *            does not depend on which other windows share the call.
 * Both calls are total: any finite or non-finite input gives a defined output, and a window reads and writes its own rows only.
 * Bad arguments (a null required pointer, M, D < 1, D > 65535, T outside [1, HYENA_VARIANT_TMAX], ldx < 3D, ldk < T, M T D > 2^38, an unknown
 * dtype) return HYENA_ERR_BAD_ARG before anything is launched.  Asynchronous on `stream`. */
#ifndef HYENA_VARIANT_H
#define HYENA_VARIANT_H
#define HYENA_VARIANT_TMAX 1024
#ifdef __cplusplus
extern "C" {
#endif

int hyena_variant_pre(const void* x3, int ldx, const float* bin, const float* w, const float* b, const float* tail, const int* pos,
                      const void* vg_ref, float* x0, float* delta, int M, int D, int T, int dtype, void* stream);
int hyena_variant_conv(const float* y_ref, const float* delta, const float* k, int ldk, const float* fb, const float* x0, void* z, int M, int D,
                       int T, int dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HYENA_VARIANT_H */
