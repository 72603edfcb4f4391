// variant_kernels.h -- edited windows of one reference sequence through the order-2 Hyena operator (variant effect scoring).
//
// A sequence that equals the reference below position p has, in every layer, the reference's own long-convolution output plus a SHORT causal
// convolution of the difference of the convolution inputs (the long convolution is linear in its input vg = v * x1, cm_kernels.h):
//     delta[s] = vg_alt[s] - vg_ref[s]   (0 for s < p)          y_alt[t] = y_ref[t] + sum_{s = p .. t} k[t - s] delta[s] + fb delta[t]
// No history is streamed.  Two kernels per layer between the in_proj and out_proj GEMMs of M windows of T positions, window m starting at the
// absolute position pos[m] (C ABI: include/hyena_variant.h):
//   variant_pre   the three short-conv outputs of every window position with cm_sc's FMA order (dec_sc, decode_kernels.h; the two positions in
//                 front of the window come from `tail`, the reference's raw in_proj outputs), the gate x0 (fp32) and
//                 delta = float(round_io(v * x1)) - float(vg_ref): the new convolution input rounded to the I/O type as the forward stores it
//   variant_conv  z[m, i, d] = round_io(round_io(y_ref[m, d, i] + sum_{j <= i} k[d, i - j] delta[m, d, j] + fb[d] delta[m, d, i]) * x0[m, i, d]):
//                 the T x T lower-triangular Toeplitz product of one (window, channel) in fp32, then decode_post's two roundings
// Both are total: every access is inside the row the thread owns, nothing is multiplied by a mask (values are selected), so any finite or
// non-finite input gives a defined output and no row ever sees another row's data.
//
// variant_conv, one (window, channel): output i is a chain of i + 1 FMAs, so the work is triangular.  A thread takes the PAIR of outputs
// (p, T - 1 - p), p < PP = ceil(T / 2): T + 1 FMAs for every thread, in ONE loop of T + 1 steps with one accumulator --
//     step s <= p : acc = fma(k[p - s], delta[s], acc)                 (output p, its terms j = s in ascending order)
//     step s = p + 1: output p's chain is set aside, acc = 0
//     step s >  p : acc = fma(k[T - s], delta[s - p - 1], acc)          (output T - 1 - p, its terms j = s - p - 1 in ascending order)
// so every lane runs the same trip count and each output keeps one fixed summation order that depends on T alone (never on M, D or the grid).
// k[d, 0 .. T) and delta[m, d, 0 .. T) are staged into LDS once.  In the first phase the lanes of a channel read k at consecutive (descending in s,
// ascending in p) words and ONE word of delta (a broadcast); in the second phase one word of k and consecutive words of delta: a
// dword read whose 32-lane group covers consecutive banks or one address, i.e. no bank conflict in either direction.  A workgroup holds
// cw = min(256 / PP, 32, D) channels of one window so that short windows still fill its lanes; channel rows lie `stride` words apart in LDS
// with stride = PP (mod 32), which keeps the lanes of neighbouring channels on disjoint banks (lane c PP + p reads bank c PP + p - s).  Lanes
// of one wavefront that stand in different phases at the same step may meet on a bank (at most 2-way, around s = p only).
// With PP > 256 (T > 512) a thread takes the pairs tid, tid + 256 one after the other.
#pragma once
#include "decode_kernels.h"   // dec_sc

namespace hyena {

enum { VAR_THREADS = 256, VAR_TMAX = 1024, VAR_CMAX = 32 };

struct VarPreArgs {
    const void* x;        // (M, T, ldx >= 3D) in_proj output of the window rows without bias, I/O type
    const float* bin;     // (3D,) in_proj bias or null
    const float* w;       // (3D, 3) short-filter taps
    const float* b;       // (3D,) short-filter bias
    const float* tail;    // (3D, M, 2) fp32: the reference's raw in_proj outputs at pos[m] - 2, pos[m] - 1
    const int* pos;       // (M,) absolute position of every window's first row (device memory)
    const void* vg_ref;   // (M, D, T) I/O type: the reference's convolution input over the window
    float* x0;            // (M, T, D) fp32 gate
    float* delta;         // (M, D, T) fp32
    int M, D, T, ldx;
};

// one thread per (m, i, d), d fastest: the short convolution is a 3-tap FIR, so every position stands alone.  grid ceil(M T D / VAR_THREADS)
template <int DT>
__global__ void __launch_bounds__(VAR_THREADS) variant_pre_kernel(VarPreArgs a) {
    typedef typename Elem<DT>::type elem_t;
    const size_t idx = (size_t)blockIdx.x * VAR_THREADS + threadIdx.x;
    if (idx >= (size_t)a.M * a.T * a.D) return;
    const int d = (int)(idx % a.D), i = (int)(idx / a.D % a.T), m = (int)(idx / a.D / a.T);
    const int t = a.pos[m] + i;
    const elem_t* x = reinterpret_cast<const elem_t*>(a.x) + (size_t)m * a.T * a.ldx;
    float o[3];
    HY_UNROLL
    for (int g = 0; g < 3; ++g) {
        const int c = g * a.D + d;
        const float* tl = a.tail + ((size_t)c * a.M + m) * 2;
        // positions i - 2, i - 1: inside the window from its own rows, in front of it from the tail (tl[0]: pos - 2, tl[1]: pos - 1)
        const float xm2 = i >= 2 ? Elem<DT>::dec(x[(size_t)(i - 2) * a.ldx + c]) : tl[i];
        const float xm1 = i >= 1 ? Elem<DT>::dec(x[(size_t)(i - 1) * a.ldx + c]) : tl[1];
        const float xn = Elem<DT>::dec(x[(size_t)i * a.ldx + c]);
        o[g] = dec_sc(xm2, xm1, xn, t, a.w[c * 3], a.w[c * 3 + 1], a.w[c * 3 + 2], a.b[c], a.bin != nullptr ? a.bin[c] : 0.f);
    }
    float p = o[1] * o[2];                                               // one fp32 product, then one conversion (decode_pre_kernel)
#if !defined(HIPEMU)
    asm volatile("" : "+v"(p));
#endif
    const size_t r = ((size_t)m * a.D + d) * a.T + i;
    a.delta[r] = Elem<DT>::dec(Elem<DT>::cvt(p)) - Elem<DT>::dec(reinterpret_cast<const elem_t*>(a.vg_ref)[r]);
    a.x0[idx] = o[0];
}

struct VarConvArgs {
    const float* y_ref;   // (M, D, T) fp32: the reference's long-convolution output over the window
    const float* delta;   // (M, D, T) fp32
    const float* k;       // (D, ldk >= T) fp32 filter, column j = tap j
    const float* fb;      // (D,) fp32 filter bias or null
    const float* x0;      // (M, T, D) fp32 gate
    void* z;              // (M, T, D) I/O type
    int M, D, T, ldk;
    int cw, pp, stride;   // channels per workgroup, pairs per channel ceil(T / 2), words between the channels' LDS rows
};

__host__ __device__ inline int var_pairs(int T) { return (T + 1) / 2; }
__host__ __device__ inline int var_cw(int D, int T) {
    int cw = VAR_THREADS / var_pairs(T);
    cw = cw < 1 ? 1 : (cw > VAR_CMAX ? VAR_CMAX : cw);
    return cw < D ? cw : D;
}
__host__ __device__ inline int var_stride(int T) { return T + (((var_pairs(T) - T) % 32 + 32) % 32); }

// grid (M, ceil(D / cw)); dynamic LDS 2 cw stride floats (at most 12 KiB)
template <int DT>
__global__ void __launch_bounds__(VAR_THREADS) variant_conv_kernel(VarConvArgs a) {
    typedef typename Elem<DT>::type elem_t;
    HY_SMEM(smem);
    HY_LDS float* ks = HY_LDS_CAST(float, smem);
    HY_LDS float* dl = ks + a.cw * a.stride;
    const int m = blockIdx.x, d0 = (int)blockIdx.y * a.cw, tid = threadIdx.x, T = a.T;
    const int nc = a.D - d0 < a.cw ? a.D - d0 : a.cw;
    for (int q = tid; q < nc * T; q += VAR_THREADS) {
        const int c = q / T, j = q - c * T;
        ks[c * a.stride + j] = a.k[(size_t)(d0 + c) * a.ldk + j];
        dl[c * a.stride + j] = a.delta[((size_t)m * a.D + d0 + c) * T + j];
    }
    __syncthreads();
    elem_t* z = reinterpret_cast<elem_t*>(a.z);
    for (int q = tid; q < nc * a.pp; q += VAR_THREADS) {
        const int c = q / a.pp, p = q - c * a.pp, d = d0 + c;
        const HY_LDS float* kc = ks + c * a.stride;
        const HY_LDS float* dc = dl + c * a.stride;
        float acc = 0.f, first = 0.f;
        for (int s = 0; s <= T; ++s) {
            const bool lo = s <= p;
            const float kv = kc[lo ? p - s : T - s];
            const float dv = dc[lo ? s : s - p - 1];
            first = s == p + 1 ? acc : first;
            acc = s == p + 1 ? 0.f : acc;
            acc = __builtin_fmaf(kv, dv, acc);
        }
        const float fb = a.fb != nullptr ? a.fb[d] : 0.f;
        const size_t row = ((size_t)m * a.D + d) * T;
        const int i2 = T - 1 - p;
        HY_UNROLL
        for (int h = 0; h < 2; ++h) {
            const int i = h == 0 ? p : i2;
            if (h == 1 && i2 == p) break;                                 // odd T: the middle output is its own partner
            float y = a.y_ref[row + i] + (h == 0 ? first : acc);
            if (a.fb != nullptr) y = __builtin_fmaf(dc[i], fb, y);
            const float yr = Elem<DT>::dec(Elem<DT>::cvt(y));             // the forward's convolution output is stored in the I/O type
            const size_t o = ((size_t)m * T + i) * a.D + d;
            // the fp32 product, then one conversion.  Left to the compiler, the fp16 kernel folds the two into one mixed-precision multiply that
            // rounds the exact product straight to fp16 (variant_pre_kernel, decode_pre_kernel): pinned, so that z is one function of its inputs
            float zp = yr * a.x0[o];
#if !defined(HIPEMU)
            asm volatile("" : "+v"(zp));
#endif
            z[o] = Elem<DT>::cvt(zp);
        }
    }
}

}  // namespace hyena
