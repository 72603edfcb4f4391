// decode_kernels.h -- one decode position of the order-2 Hyena operator for all B sequences (incremental generation).
//
// Every operation of the operator is per-position or causal, and the implicit filter is prefix-consistent (column j of filter_dl(L) does not
// depend on L), so position t of the long convolution is a plain dot product over the history of its input:
//     y_t[b, c] = sum_{s <= t} k[c, t - s] vg[b, c, s] + fb[c] vg[b, c, t]          vg = v * x1, the convolution's input (cm_kernels.h)
// Three kernels per layer and position, between the in_proj and out_proj GEMVs (C ABI: include/hyena_decode.h):
//   decode_pre   xT_t (+ b_in) and the two previous positions (tail state) -> the three short-conv outputs with cm_sc's FMA order, vg_t into
//                column t of the history, the gate x0_t (fp32), the tail shifted by one
//   decode_conv  sum_{s <= t} k[c, t - s] vg[b, c, s] in fp32 over a FIXED grid of (channel, history chunk) workgroups: one partial per
//                (chunk, b, c), no atomics; chunks that start past t leave at once.  The grid depends on Lcap only, never on t.
//   decode_post  the partials summed in chunk order, + fb vg_t, rounded to the I/O type where the forward rounds the convolution's output,
//                times x0_t with cm_post_fwd's arithmetic -> z_t; then the position advances
// The position t lives in device memory and all three kernels read it there: one captured graph serves every position.
// Variants further down: one position per row (_rows), n continuations of one prompt (_fan), T known positions per call (_block), and the
// lookahead carry (_carry, _la): the history's share of the next W outputs taken once per W positions, so that a step reads W + 7 columns.
// At the end of the file: token sampling (plain and constrained) and beam search over the fan-out layout (the beam step, the cache's
// re-parenting, the backtrack).
//
// The two streams of decode_conv run in opposite directions (vg forward in s, k backward), and the k stream is misaligned by t mod 4 words
// relative to the vg stream.  The history is the operand that scales with B, so ITS loads stay aligned 16-byte vectors (8 elements per lane at
// 8-aligned positions of 8-aligned rows); the filter segment a workgroup needs, k[c, t - s0 - CHUNK + 1 .. t - s0], is staged ONCE into LDS with
// aligned 16-byte loads (the segment rounded outwards to 4 words) and read back from LDS at the shifted, reversed index for every one of the B
// rows: k's global bytes do not scale with B and no global load is under-aligned.  (Storing k reversed at cache-build time would put both
// streams in one direction but leave the t mod 4 offset, i.e. under-aligned 16-byte k loads, and k re-read per row or B accumulators per lane.)
#pragma once
#include "block_kernels.h"   // philox4x32_10
#include "cm_kernels.h"

namespace hyena {

enum { DEC_THREADS = 256, DEC_V = 8, DEC_NV = 4, DEC_CHUNK = DEC_THREADS * DEC_V * DEC_NV /* 8192 positions */, DEC_POST_THREADS = 1024,
       DEC_KLDS = DEC_CHUNK + 8 /* floats of staged filter */ };

struct DecArgs {
    const void* x;      // pre: in_proj output of the new position without its bias, element (c, b) at b ldx + c, I/O type
    const float* bin;   // (3D,) in_proj bias or null
    const float* w;     // (3D, 3) short-filter taps
    const float* b;     // (3D,) short-filter bias
    float* tail;        // (3D, Bcap, 2) fp32: raw xT of positions t - 2, t - 1
    void* vg;           // history (Bcap, D, lda) I/O type: row (b, d) at (b D + d) lda
    float* x0;          // (B, D) fp32 gate of position t
    const float* k;     // (D, ldk) fp32 filter, column j = tap j
    float* part;        // [nchunks][B][D] fp32 partial sums
    const float* fb;    // (D,) fp32 filter bias or null
    void* z;            // (B, D) I/O type
    int* pos;           // the position t (device memory); the *_rows kernels: B positions, one per row
    int B, D, Bcap, Lcap, ldx, lda, ldk;
};

__device__ __forceinline__ float dec_sc(float xm2, float xm1, float xn, int t, float w0, float w1, float w2, float bsc, float bin) {
    // cm_sc (cm_kernels.h) at one position: taps before position 0 are zero padding, explicit FMAs in the same order
    const float x0 = t >= 2 ? xm2 + bin : 0.f, x1 = t >= 1 ? xm1 + bin : 0.f, x2 = xn + bin;
    return __builtin_fmaf(w2, x2, __builtin_fmaf(w1, x1, __builtin_fmaf(w0, x0, bsc)));
}

// one thread per (b, d): grid ceil(B D / DEC_THREADS)
template <int DT>
__global__ void __launch_bounds__(DEC_THREADS) decode_pre_kernel(DecArgs a) {
    typedef typename Elem<DT>::type elem_t;
    const int i = (int)(blockIdx.x * DEC_THREADS + threadIdx.x);
    const int t = a.pos[0];
    if (i >= a.B * a.D || t < 0 || t >= a.Lcap) return;
    const int b = i / a.D, d = i % a.D;
    const elem_t* x = reinterpret_cast<const elem_t*>(a.x);
    float o[3];
    HY_UNROLL
    for (int g = 0; g < 3; ++g) {
        const int c = g * a.D + d;
        float* tl = a.tail + ((size_t)c * a.Bcap + b) * 2;
        const float xm2 = tl[0], xm1 = tl[1];
        const float xn = Elem<DT>::dec(x[(size_t)b * a.ldx + c]);
        o[g] = dec_sc(xm2, xm1, xn, t, a.w[c * 3], a.w[c * 3 + 1], a.w[c * 3 + 2], a.b[c], a.bin != nullptr ? a.bin[c] : 0.f);
        tl[0] = xm1;
        tl[1] = xn;
    }
    elem_t* vg = reinterpret_cast<elem_t*>(a.vg);
    // cm_pre_fwd: the fp32 product c1 * cv, then one conversion.  Left to the compiler, the fp16 kernel folds the two into one mixed-precision
    // multiply that rounds the exact product straight to fp16, and ~3e-5 of the elements land on the other neighbour than cm_pre_fwd's
    float p = o[1] * o[2];
#if !defined(HIPEMU)
    asm volatile("" : "+v"(p));
#endif
    vg[((size_t)b * a.D + d) * a.lda + t] = Elem<DT>::cvt(p);
    a.x0[(size_t)b * a.D + d] = o[0];
}

// grid (nchunks, D): workgroup (chunk, c) covers history positions [chunk DEC_CHUNK, (chunk + 1) DEC_CHUNK) of channel c for every b
template <int DT>
__global__ void __launch_bounds__(DEC_THREADS) decode_conv_kernel(DecArgs a) {
    constexpr size_t ES = CmEs<DT>::V;
    HY_SMEM(smem);
    HY_LDS float* ks = HY_LDS_CAST(float, smem);
    HY_LDS float* red = ks + DEC_KLDS;                                   // [2][4]: wavefront sums, alternating by row parity
    const int t = a.pos[0];
    const int chunk = blockIdx.x, c = blockIdx.y, tid = threadIdx.x;
    const int s0 = chunk * DEC_CHUNK;
    if (t < 0 || t >= a.Lcap || s0 > t) return;
    // stage k[c, base .. t - s0] (base = t - s0 - DEC_CHUNK + 1 rounded down to 4 words; negative taps are zeros) with aligned 16-byte loads
    const int jlo = t - s0 - DEC_CHUNK + 1;
    const int base = jlo >= 0 ? (jlo & ~3) : -((3 - jlo) & ~3);
    const int ngroups = (t - s0 - base) / 4 + 1;
    const float* krow = a.k + (size_t)c * a.ldk;
    for (int q = tid; q < ngroups; q += DEC_THREADS) {
        const int j = base + 4 * q;
        float r[4] = {0.f, 0.f, 0.f, 0.f};
        if (j >= 0) __builtin_memcpy(r, krow + j, sizeof(r));
        HY_UNROLL
        for (int e = 0; e < 4; ++e) ks[4 * q + e] = r[e];
    }
    __syncthreads();
    for (int b = 0; b < a.B; ++b) {
        const char* row = cm_row(a.vg, (size_t)b * a.D + c, a.lda, ES);
        float acc = 0.f;
        HY_UNROLL
        for (int v = 0; v < DEC_NV; ++v) {
            const int s = s0 + (v * DEC_THREADS + tid) * DEC_V;
            if (s <= t) {                                                 // (s + DEC_V <= lda: rows are 8-aligned and t < Lcap <= lda)
                // 16-byte aligned (rows start 16-byte aligned, lda and s are multiples of 8): one / two dwordx4 loads, also for fp32
                // (positions past t inside the last vector are read and multiplied by a zero tap: the history holds finite values only --
                // zeros from the cache's allocation or earlier steps' outputs; selecting the tap instead of the product keeps the load whole)
                typename Elem<DT>::type raw[DEC_V];
                __builtin_memcpy(raw, __builtin_assume_aligned(row + (size_t)s * ES, 16), sizeof(raw));
                float x[DEC_V];
                HY_UNROLL
                for (int e = 0; e < DEC_V; ++e) x[e] = Elem<DT>::dec(raw[e]);
                HY_UNROLL
                for (int e = 0; e < DEC_V; ++e) {
                    const bool ok = s + e <= t;
                    const float kv = ks[ok ? t - s - e - base : 0];
                    const float kk = ok ? kv : 0.f;
                    acc = __builtin_fmaf(kk, x[e], acc);
                }
            }
        }
        acc = cm_wave_sum(acc);
        HY_LDS float* rb = red + 4 * (b & 1);
        if ((tid & 63) == 0) rb[tid >> 6] = acc;
        __syncthreads();
        if (tid == 0) a.part[((size_t)chunk * a.B + b) * a.D + c] = (rb[0] + rb[1]) + (rb[2] + rb[3]);
    }
}

// ONE workgroup: every thread reads t before the barrier, one lane advances it after
template <int DT>
__global__ void __launch_bounds__(DEC_POST_THREADS) decode_post_kernel(DecArgs a) {
    typedef typename Elem<DT>::type elem_t;
    const int t = a.pos[0];
    const bool valid = t >= 0 && t < a.Lcap;
    if (valid) {
        const int nc = t / DEC_CHUNK + 1;
        const elem_t* vg = reinterpret_cast<const elem_t*>(a.vg);
        elem_t* z = reinterpret_cast<elem_t*>(a.z);
        for (int i = threadIdx.x; i < a.B * a.D; i += DEC_POST_THREADS) {
            const int b = i / a.D, d = i % a.D;
            float y = 0.f;
            for (int ch = 0; ch < nc; ++ch) y += a.part[((size_t)ch * a.B + b) * a.D + d];
            const float u = Elem<DT>::dec(vg[((size_t)b * a.D + d) * a.lda + t]);
            if (a.fb != nullptr) y = __builtin_fmaf(u, a.fb[d], y);
            const float yr = Elem<DT>::dec(Elem<DT>::cvt(y));                 // the forward's convolution output is stored in the I/O type
            z[i] = Elem<DT>::cvt(yr * a.x0[i]);                                // cm_post_fwd: y * c0, rounded once
        }
    }
    __syncthreads();
    if (threadIdx.x == 0 && valid) a.pos[0] = t + 1;
}

// ---- per-row positions: the same three kernels with t_b = pos[b] from a device int pos[B] (C ABI: hyena_decode_*_rows) --------------------
// Row b of a batch of prompts of different lengths stands at its own position.  A row whose t_b is outside [0, Lcap) is parked: nothing of
// it is read or written and its position stays.  With all t_b equal every kernel computes what its single-position twin above computes,
// bit for bit (same arithmetic, same lanes, same summation order).

// one thread per (b, d): grid ceil(B D / DEC_THREADS)
template <int DT>
__global__ void __launch_bounds__(DEC_THREADS) decode_pre_rows_kernel(DecArgs a) {
    typedef typename Elem<DT>::type elem_t;
    const int i = (int)(blockIdx.x * DEC_THREADS + threadIdx.x);
    if (i >= a.B * a.D) return;
    const int b = i / a.D, d = i % a.D;
    const int t = a.pos[b];
    if (t < 0 || t >= a.Lcap) return;                                    // a parked row: its tail is not shifted
    const elem_t* x = reinterpret_cast<const elem_t*>(a.x);
    float o[3];
    HY_UNROLL
    for (int g = 0; g < 3; ++g) {
        const int c = g * a.D + d;
        float* tl = a.tail + ((size_t)c * a.Bcap + b) * 2;
        const float xm2 = tl[0], xm1 = tl[1];
        const float xn = Elem<DT>::dec(x[(size_t)b * a.ldx + c]);
        o[g] = dec_sc(xm2, xm1, xn, t, a.w[c * 3], a.w[c * 3 + 1], a.w[c * 3 + 2], a.b[c], a.bin != nullptr ? a.bin[c] : 0.f);
        tl[0] = xm1;
        tl[1] = xn;
    }
    elem_t* vg = reinterpret_cast<elem_t*>(a.vg);
    float p = o[1] * o[2];                                               // one fp32 product, then one conversion (decode_pre_kernel)
#if !defined(HIPEMU)
    asm volatile("" : "+v"(p));
#endif
    vg[((size_t)b * a.D + d) * a.lda + t] = Elem<DT>::cvt(p);
    a.x0[(size_t)b * a.D + d] = o[0];
}

// grid (nchunks, D) as decode_conv_kernel.  The staged filter window k[c, t_b - s0 - CHUNK + 1 .. t_b - s0] depends on the row: it is staged
// again only when t_b differs from the position whose window is in LDS.  Every branch around a barrier is taken on pos[b] as all threads
// read it from the same address (nobody writes pos during this kernel), so it is uniform across the workgroup.
template <int DT>
__global__ void __launch_bounds__(DEC_THREADS) decode_conv_rows_kernel(DecArgs a) {
    constexpr size_t ES = CmEs<DT>::V;
    HY_SMEM(smem);
    HY_LDS float* ks = HY_LDS_CAST(float, smem);
    HY_LDS float* red = ks + DEC_KLDS;                                   // [2][4]: wavefront sums, alternating by the parity of the live row
    const int chunk = blockIdx.x, c = blockIdx.y, tid = threadIdx.x;
    const int s0 = chunk * DEC_CHUNK;
    int tmax = -1;
    for (int b = 0; b < a.B; ++b) {
        const int t = a.pos[b];
        if (t >= 0 && t < a.Lcap && t > tmax) tmax = t;
    }
    if (s0 > tmax) return;                                               // the chunk starts past every row: nothing staged, nothing loaded
    const float* krow = a.k + (size_t)c * a.ldk;
    int staged = -1, base = 0, live = 0;                                 // staged: the position whose window ks holds
    for (int b = 0; b < a.B; ++b) {
        const int t = a.pos[b];
        if (t < 0 || t >= a.Lcap || s0 > t) continue;                    // parked, or the chunk starts past this row: no partial is written
        if (t != staged) {
            // (every wavefront's reads of the previous window lie before the barrier that closed the previous live row)
            const int jlo = t - s0 - DEC_CHUNK + 1;
            base = jlo >= 0 ? (jlo & ~3) : -((3 - jlo) & ~3);
            const int ngroups = (t - s0 - base) / 4 + 1;
            for (int q = tid; q < ngroups; q += DEC_THREADS) {
                const int j = base + 4 * q;
                float r[4] = {0.f, 0.f, 0.f, 0.f};
                if (j >= 0) __builtin_memcpy(r, krow + j, sizeof(r));
                HY_UNROLL
                for (int e = 0; e < 4; ++e) ks[4 * q + e] = r[e];
            }
            __syncthreads();
            staged = t;
        }
        const char* row = cm_row(a.vg, (size_t)b * a.D + c, a.lda, ES);
        float acc = 0.f;
        HY_UNROLL
        for (int v = 0; v < DEC_NV; ++v) {
            const int s = s0 + (v * DEC_THREADS + tid) * DEC_V;
            if (s <= t) {                                                 // (s + DEC_V <= lda: rows are 8-aligned and t < Lcap <= lda)
                // aligned 16-byte loads; positions past t inside the last vector meet a zero tap (the history holds finite values only)
                typename Elem<DT>::type raw[DEC_V];
                __builtin_memcpy(raw, __builtin_assume_aligned(row + (size_t)s * ES, 16), sizeof(raw));
                float x[DEC_V];
                HY_UNROLL
                for (int e = 0; e < DEC_V; ++e) x[e] = Elem<DT>::dec(raw[e]);
                HY_UNROLL
                for (int e = 0; e < DEC_V; ++e) {
                    const bool ok = s + e <= t;
                    const float kv = ks[ok ? t - s - e - base : 0];
                    const float kk = ok ? kv : 0.f;
                    acc = __builtin_fmaf(kk, x[e], acc);
                }
            }
        }
        acc = cm_wave_sum(acc);
        HY_LDS float* rb = red + 4 * (live & 1);
        ++live;
        if ((tid & 63) == 0) rb[tid >> 6] = acc;
        __syncthreads();
        if (tid == 0) a.part[((size_t)chunk * a.B + b) * a.D + c] = (rb[0] + rb[1]) + (rb[2] + rb[3]);
    }
}

// ONE workgroup: every thread reads the positions it needs before the barrier; after it, lane b advances pos[b] (the only access to pos[b]
// past the barrier).  Row b sums the t_b / DEC_CHUNK + 1 partials decode_conv_rows wrote for it in this step and no other slot.
template <int DT>
__global__ void __launch_bounds__(DEC_POST_THREADS) decode_post_rows_kernel(DecArgs a) {
    typedef typename Elem<DT>::type elem_t;
    const elem_t* vg = reinterpret_cast<const elem_t*>(a.vg);
    elem_t* z = reinterpret_cast<elem_t*>(a.z);
    for (int i = threadIdx.x; i < a.B * a.D; i += DEC_POST_THREADS) {
        const int b = i / a.D, d = i % a.D;
        const int t = a.pos[b];
        if (t < 0 || t >= a.Lcap) continue;
        const int nc = t / DEC_CHUNK + 1;
        float y = 0.f;
        for (int ch = 0; ch < nc; ++ch) y += a.part[((size_t)ch * a.B + b) * a.D + d];
        const float u = Elem<DT>::dec(vg[((size_t)b * a.D + d) * a.lda + t]);
        if (a.fb != nullptr) y = __builtin_fmaf(u, a.fb[d], y);
        const float yr = Elem<DT>::dec(Elem<DT>::cvt(y));                 // the forward's convolution output is stored in the I/O type
        z[i] = Elem<DT>::cvt(yr * a.x0[i]);                                // cm_post_fwd: y * c0, rounded once
    }
    __syncthreads();
    for (int b = threadIdx.x; b < a.B; b += DEC_POST_THREADS) {
        const int t = a.pos[b];
        if (t >= 0 && t < a.Lcap) a.pos[b] = t + 1;
    }
}

// ---- fan-out: n continuations of one prompt (C ABI: hyena_decode_*_fan) --------------------------------------------------------------------
// G prompts, each fanned out to n = `fan` rows: B = G n, row b belongs to group b / n, one position t for the batch.  Below S (a multiple of
// DEC_CHUNK, at most the prompt length) the n rows of a group hold the same history, so it is stored ONCE:
//   shared   vgs (G, D, lds): columns [0, S) of group g            per row   vg (Bcap, D, lda): columns [S, Lcap) of row b, column s at s - S
// A partial sum of decode_conv depends on one (chunk, row, channel) history segment and on t only, so the partial of a chunk below S is one
// number for the n rows of a group: workgroup (chunk, c) with chunk < S / DEC_CHUNK computes it once per group, into slot [chunk][g n][c] of
// the same `part` layout (the group's other slots of that chunk are neither written nor read), and decode_post_fan reads it from there for
// every row of the group, in the same chunk order.  Same lanes, same FMA order, same wave sums as the single-position kernels: on a batch
// whose rows hold the replicated history those give the same z, x0, tail, history column and position, bit for bit.
// S is a multiple of DEC_CHUNK (so of 8): every 8-element vector of either tensor keeps its 16-byte alignment.  A position outside
// [S, Lcap) makes the kernels do nothing (below S there is no row column to write).
struct DecFanArgs : DecArgs {   // vg / lda: the per-row history and its pitch
    const void* vgs;            // shared history (G, D, lds) I/O type, or null when S == 0
    int fan, S, lds;
};

// one thread per (b, d): decode_pre_kernel's arithmetic, vg_t into column t - S of the row history
template <int DT>
__global__ void __launch_bounds__(DEC_THREADS) decode_pre_fan_kernel(DecFanArgs a) {
    typedef typename Elem<DT>::type elem_t;
    const int i = (int)(blockIdx.x * DEC_THREADS + threadIdx.x);
    const int t = a.pos[0];
    if (i >= a.B * a.D || t < a.S || t >= a.Lcap) return;
    const int b = i / a.D, d = i % a.D;
    const elem_t* x = reinterpret_cast<const elem_t*>(a.x);
    float o[3];
    HY_UNROLL
    for (int g = 0; g < 3; ++g) {
        const int c = g * a.D + d;
        float* tl = a.tail + ((size_t)c * a.Bcap + b) * 2;
        const float xm2 = tl[0], xm1 = tl[1];
        const float xn = Elem<DT>::dec(x[(size_t)b * a.ldx + c]);
        o[g] = dec_sc(xm2, xm1, xn, t, a.w[c * 3], a.w[c * 3 + 1], a.w[c * 3 + 2], a.b[c], a.bin != nullptr ? a.bin[c] : 0.f);
        tl[0] = xm1;
        tl[1] = xn;
    }
    elem_t* vg = reinterpret_cast<elem_t*>(a.vg);
    float p = o[1] * o[2];                                               // one fp32 product, then one conversion (decode_pre_kernel)
#if !defined(HIPEMU)
    asm volatile("" : "+v"(p));
#endif
    vg[((size_t)b * a.D + d) * a.lda + (t - a.S)] = Elem<DT>::cvt(p);
    a.x0[(size_t)b * a.D + d] = o[0];
}

// grid (nchunks, D) as decode_conv_kernel; the filter window is staged once per workgroup (one t for the batch).  Workgroup (chunk, c) with
// chunk < S / DEC_CHUNK loops over the G groups on the shared history, the others over the B rows on the row history.  The early exit and
// the choice between the two are taken on pos[0], S and blockIdx: uniform across the workgroup; both loops have a uniform trip count and
// one barrier per trip, as decode_conv_kernel's.
template <int DT>
__global__ void __launch_bounds__(DEC_THREADS) decode_conv_fan_kernel(DecFanArgs a) {
    constexpr size_t ES = CmEs<DT>::V;
    HY_SMEM(smem);
    HY_LDS float* ks = HY_LDS_CAST(float, smem);
    HY_LDS float* red = ks + DEC_KLDS;                                   // [2][4]: wavefront sums, alternating by the parity of the trip
    const int t = a.pos[0];
    const int chunk = blockIdx.x, c = blockIdx.y, tid = threadIdx.x;
    const int s0 = chunk * DEC_CHUNK;
    if (t < a.S || t >= a.Lcap || s0 > t) return;
    const int jlo = t - s0 - DEC_CHUNK + 1;
    const int base = jlo >= 0 ? (jlo & ~3) : -((3 - jlo) & ~3);
    const int ngroups = (t - s0 - base) / 4 + 1;
    const float* krow = a.k + (size_t)c * a.ldk;
    for (int q = tid; q < ngroups; q += DEC_THREADS) {
        const int j = base + 4 * q;
        float r[4] = {0.f, 0.f, 0.f, 0.f};
        if (j >= 0) __builtin_memcpy(r, krow + j, sizeof(r));
        HY_UNROLL
        for (int e = 0; e < 4; ++e) ks[4 * q + e] = r[e];
    }
    __syncthreads();
    const bool shared = s0 < a.S;                                        // S is a multiple of DEC_CHUNK: the whole chunk lies on one side
    const int nrows = shared ? a.B / a.fan : a.B;
    const void* src = shared ? a.vgs : a.vg;
    const int ld = shared ? a.lds : a.lda;
    const int off = shared ? 0 : a.S;                                    // the tensor's column of history position s: s - off
    for (int r = 0; r < nrows; ++r) {
        const char* row = cm_row(src, (size_t)r * a.D + c, ld, ES);
        float acc = 0.f;
        HY_UNROLL
        for (int v = 0; v < DEC_NV; ++v) {
            const int s = s0 + (v * DEC_THREADS + tid) * DEC_V;
            if (s <= t) {                                                 // (s - off + DEC_V <= ld: 8-aligned rows; s <= t < S <= lds, or t - S < lda)
                // aligned 16-byte loads; positions past t inside the last vector meet a zero tap (the history holds finite values only)
                typename Elem<DT>::type raw[DEC_V];
                __builtin_memcpy(raw, __builtin_assume_aligned(row + (size_t)(s - off) * ES, 16), sizeof(raw));
                float x[DEC_V];
                HY_UNROLL
                for (int e = 0; e < DEC_V; ++e) x[e] = Elem<DT>::dec(raw[e]);
                HY_UNROLL
                for (int e = 0; e < DEC_V; ++e) {
                    const bool ok = s + e <= t;
                    const float kv = ks[ok ? t - s - e - base : 0];
                    const float kk = ok ? kv : 0.f;
                    acc = __builtin_fmaf(kk, x[e], acc);
                }
            }
        }
        acc = cm_wave_sum(acc);
        HY_LDS float* rb = red + 4 * (r & 1);
        if ((tid & 63) == 0) rb[tid >> 6] = acc;
        __syncthreads();
        const int slot = shared ? r * a.fan : r;
        if (tid == 0) a.part[((size_t)chunk * a.B + slot) * a.D + c] = (rb[0] + rb[1]) + (rb[2] + rb[3]);
    }
}

// ONE workgroup, as decode_post_kernel: the partial of chunk ch from the group's slot below S, from the row's own slot from S on
template <int DT>
__global__ void __launch_bounds__(DEC_POST_THREADS) decode_post_fan_kernel(DecFanArgs a) {
    typedef typename Elem<DT>::type elem_t;
    const int t = a.pos[0];
    const bool valid = t >= a.S && t < a.Lcap;
    if (valid) {
        const int nc = t / DEC_CHUNK + 1, ns = a.S / DEC_CHUNK;
        const elem_t* vg = reinterpret_cast<const elem_t*>(a.vg);
        elem_t* z = reinterpret_cast<elem_t*>(a.z);
        for (int i = threadIdx.x; i < a.B * a.D; i += DEC_POST_THREADS) {
            const int b = i / a.D, d = i % a.D;
            const int bs = b / a.fan * a.fan;
            float y = 0.f;
            for (int ch = 0; ch < nc; ++ch) y += a.part[((size_t)ch * a.B + (ch < ns ? bs : b)) * a.D + d];
            const float u = Elem<DT>::dec(vg[((size_t)b * a.D + d) * a.lda + (t - a.S)]);
            if (a.fb != nullptr) y = __builtin_fmaf(u, a.fb[d], y);
            const float yr = Elem<DT>::dec(Elem<DT>::cvt(y));                 // the forward's convolution output is stored in the I/O type
            z[i] = Elem<DT>::cvt(yr * a.x0[i]);                                // cm_post_fwd: y * c0, rounded once
        }
    }
    __syncthreads();
    if (threadIdx.x == 0 && valid) a.pos[0] = t + 1;
}

// ---- block step: T known positions appended in one pass (C ABI: hyena_decode_*_block and *_block_fan) -------------------------------------
// All B rows advance from t0 = *pos to t0 + T, 1 <= T <= DEC_TMAX.  The T outputs of a (row, channel) read the same history and a filter
// window only T - 1 taps longer, so the history is streamed ONCE for the block: a lane keeps its DEC_NV 8-element history vectors in
// registers and runs T accumulators over them, DEC_TT (or DEC_TR for the remainder) at a time.  One set of kernels serves the plain cache
// (S = 0, fan = 1: nothing is shared) and the fan-out layout of DecFanArgs.
//   x (B, T, 3D): element (b, i, c) at (b T + i) ldx + c;   x0, z (B, T, D);   part [chunk][B][T][D] (the slot rule of the fan kernels:
//   a chunk below S writes and reads slot b = g fan only)
// Bit for bit what T single-position steps leave (z, x0, the history columns, tail, pos), because every output keeps its summation:
//   - output i of a lane is its own FMA chain over (vector v, element e) in that order, starting from 0.  The single-position kernel
//     skips a vector that starts past t and selects a zero tap past t inside a vector; here those taps are zeros of the staged window
//     (k has no negative index), and fma(0, x, acc) == acc for finite x and any acc this chain can hold (it never holds -0: it starts at
//     +0, and x + y is -0 only when both are).  Vectors that start past t0 + T - 1 are skipped.  So the history columns a block touches
//     past an output's own position -- the block's later columns and up to 7 columns of over-read -- must be finite, as today.
//   - then cm_wave_sum, (r0 + r1) + (r2 + r3) over the four wavefronts, and the chunks in order in decode_post_block.
// Filter window in LDS: ks[m] = k[c, jlo + m], jlo = t0 - s0 - DEC_CHUNK + 1, m in [0, DEC_CHUNK + DEC_TMAX), zero where jlo + m is negative
// or past t0 + T - 1 - s0.  The tap of (output i, position s = s0 + 8 q + e) is k[t0 + i - s] = ks[(DEC_CHUNK - 8 - 8 q + i0) + (i - i0) - e + 7]:
// a lane's window for a tile of outputs [i0, i0 + TT) is the TT + 7 floats from an index that is a multiple of 4 (i0 is), read as aligned
// 16-byte LDS vectors into registers once per (vector, tile) and slid over the 8 elements -- (TT + 8) / 4 LDS reads for 8 TT FMAs.  The
// staging itself is dword loads (coalesced; jlo has any alignment), once per workgroup for all rows.
enum { DEC_TMAX = 64, DEC_TT = 16, DEC_TR = 4, DEC_PRE_J = 8, DEC_KLDS_BLOCK = DEC_CHUNK + DEC_TMAX, DEC_RED_BLOCK = 2 * DEC_TT * 4 };

struct DecBlockArgs : DecFanArgs {
    int T;
};

__device__ __forceinline__ bool dec_block_valid(const DecBlockArgs& a, int t0) { return t0 >= a.S && t0 <= a.Lcap - a.T; }

// one thread per (b, d), the T positions in order: grid ceil(B D / DEC_THREADS)
template <int DT>
__global__ void __launch_bounds__(DEC_THREADS) decode_pre_block_kernel(DecBlockArgs a) {
    typedef typename Elem<DT>::type elem_t;
    const int i = (int)(blockIdx.x * DEC_THREADS + threadIdx.x);
    const int t0 = a.pos[0];
    if (i >= a.B * a.D || !dec_block_valid(a, t0)) return;
    const int b = i / a.D, d = i % a.D;
    const elem_t* x = reinterpret_cast<const elem_t*>(a.x) + (size_t)b * a.T * a.ldx;
    elem_t* vg = reinterpret_cast<elem_t*>(a.vg) + ((size_t)b * a.D + d) * a.lda + (t0 - a.S);
    float* x0 = a.x0 + (size_t)b * a.T * a.D + d;
    float xm2[3], xm1[3], w[3][3], bsc[3], bin[3];
    HY_UNROLL
    for (int g = 0; g < 3; ++g) {
        const int c = g * a.D + d;
        const float* tl = a.tail + ((size_t)c * a.Bcap + b) * 2;
        xm2[g] = tl[0];
        xm1[g] = tl[1];
        w[g][0] = a.w[c * 3]; w[g][1] = a.w[c * 3 + 1]; w[g][2] = a.w[c * 3 + 2];
        bsc[g] = a.b[c];
        bin[g] = a.bin != nullptr ? a.bin[c] : 0.f;
    }
    for (int j0 = 0; j0 < a.T; j0 += DEC_PRE_J) {
        float xin[DEC_PRE_J][3];                                         // the loads of DEC_PRE_J positions in flight before the first store
        HY_UNROLL
        for (int jj = 0; jj < DEC_PRE_J; ++jj) {
            const int j = j0 + jj < a.T ? j0 + jj : a.T - 1;
            HY_UNROLL
            for (int g = 0; g < 3; ++g) xin[jj][g] = Elem<DT>::dec(x[(size_t)j * a.ldx + g * a.D + d]);
        }
        HY_UNROLL
        for (int jj = 0; jj < DEC_PRE_J; ++jj) {
            const int j = j0 + jj;
            if (j < a.T) {
                float o[3];
                HY_UNROLL
                for (int g = 0; g < 3; ++g) {
                    const float xn = xin[jj][g];
                    o[g] = dec_sc(xm2[g], xm1[g], xn, t0 + j, w[g][0], w[g][1], w[g][2], bsc[g], bin[g]);
                    xm2[g] = xm1[g];
                    xm1[g] = xn;
                }
                float p = o[1] * o[2];                                   // one fp32 product, then one conversion (decode_pre_kernel)
#if !defined(HIPEMU)
                asm volatile("" : "+v"(p));
#endif
                vg[j] = Elem<DT>::cvt(p);
                x0[(size_t)j * a.D] = o[0];
            }
        }
    }
    HY_UNROLL
    for (int g = 0; g < 3; ++g) {
        float* tl = a.tail + ((size_t)(g * a.D + d) * a.Bcap + b) * 2;
        tl[0] = xm2[g];
        tl[1] = xm1[g];
    }
}

// TT outputs [i0, i0 + TT) of one row over the lane's history vectors: acc[ii] is output i0 + ii's FMA chain over (v, e)
template <int TT>
__device__ __forceinline__ void dec_block_tile(const float (&x)[DEC_NV][DEC_V], const bool (&live)[DEC_NV], const HY_LDS float* ks, int tid,
                                               int i0, float (&acc)[TT]) {
    constexpr int NW = (TT + 7 + 3) / 4 * 4;
    HY_UNROLL
    for (int ii = 0; ii < TT; ++ii) acc[ii] = 0.f;
    HY_UNROLL
    for (int v = 0; v < DEC_NV; ++v) {
        if (live[v]) {
            const int m0 = DEC_CHUNK - DEC_V - (v * DEC_THREADS + tid) * DEC_V + i0;   // a multiple of 4: aligned 16-byte LDS reads
            float w[NW];
            HY_UNROLL
            for (int q = 0; q < NW / 4; ++q) {
#if defined(HIPEMU)
                __builtin_memcpy(w + 4 * q, ks + m0 + 4 * q, 16);
#else
                typedef float dec_f4 __attribute__((ext_vector_type(4)));
                const dec_f4 r = *reinterpret_cast<const HY_LDS dec_f4*>(ks + m0 + 4 * q);
                w[4 * q] = r.x; w[4 * q + 1] = r.y; w[4 * q + 2] = r.z; w[4 * q + 3] = r.w;
#endif
            }
            HY_UNROLL
            for (int e = 0; e < DEC_V; ++e) {
                HY_UNROLL
                for (int ii = 0; ii < TT; ++ii) acc[ii] = __builtin_fmaf(w[ii - e + 7], x[v][e], acc[ii]);
            }
        }
    }
}

// wavefront sums of the tile's outputs -> red (one parity) -> part[chunk][slot][i0 + ii][c]; one barrier
template <int TT>
__device__ __forceinline__ void dec_block_reduce(float (&acc)[TT], HY_LDS float* rb, int tid, int i0, int T, float* part, int D) {
    HY_UNROLL
    for (int ii = 0; ii < TT; ++ii) acc[ii] = cm_wave_sum(acc[ii]);
    if ((tid & 63) == 0) {
        HY_UNROLL
        for (int ii = 0; ii < TT; ++ii) rb[ii * 4 + (tid >> 6)] = acc[ii];
    }
    __syncthreads();
    if (tid < TT && i0 + tid < T) part[(size_t)(i0 + tid) * D] = (rb[tid * 4] + rb[tid * 4 + 1]) + (rb[tid * 4 + 2] + rb[tid * 4 + 3]);
}

// grid (nchunks, D) as decode_conv_fan_kernel, the same split between shared and row history.  Every branch around a barrier is taken on
// pos[0], T, S and blockIdx: uniform across the workgroup; one barrier per (row, tile).  A chunk that starts inside the block
// (t0 < s0 <= t0 + T - 1) also writes the (zero) partials of the outputs before s0, which decode_post_block does not read.
template <int DT>
__global__ void __launch_bounds__(DEC_THREADS) decode_conv_block_kernel(DecBlockArgs a) {
    constexpr size_t ES = CmEs<DT>::V;
    HY_SMEM(smem);
    HY_LDS float* ks = HY_LDS_CAST(float, smem);
    HY_LDS float* red = ks + DEC_KLDS_BLOCK;                             // [2][DEC_TT][4]: wavefront sums, alternating by the parity of the trip
    const int t0 = a.pos[0];
    const int chunk = blockIdx.x, c = blockIdx.y, tid = threadIdx.x, T = a.T;
    const int s0 = chunk * DEC_CHUNK;
    if (!dec_block_valid(a, t0) || s0 > t0 + T - 1) return;
    const int tmax = t0 + T - 1;
    const int jlo = t0 - s0 - DEC_CHUNK + 1, jhi = tmax - s0;
    const float* krow = a.k + (size_t)c * a.ldk;
    for (int m = tid; m < DEC_KLDS_BLOCK; m += DEC_THREADS) {
        const int j = jlo + m;
        const bool ok = j >= 0 && j <= jhi;
        const float kv = krow[ok ? j : 0];
        ks[m] = ok ? kv : 0.f;
    }
    __syncthreads();
    const bool shared = s0 < a.S;                                        // S is a multiple of DEC_CHUNK: the whole chunk lies on one side
    const int nrows = shared ? a.B / a.fan : a.B;
    const void* src = shared ? a.vgs : a.vg;
    const int ld = shared ? a.lds : a.lda;
    const int off = shared ? 0 : a.S;                                    // the tensor's column of history position s: s - off
    bool live[DEC_NV];
    HY_UNROLL
    for (int v = 0; v < DEC_NV; ++v) live[v] = s0 + (v * DEC_THREADS + tid) * DEC_V <= tmax;
    int trip = 0;
    for (int r = 0; r < nrows; ++r) {
        const char* row = cm_row(src, (size_t)r * a.D + c, ld, ES);
        float x[DEC_NV][DEC_V];
        HY_UNROLL
        for (int v = 0; v < DEC_NV; ++v) {
            const int s = s0 + (v * DEC_THREADS + tid) * DEC_V;
            HY_UNROLL
            for (int e = 0; e < DEC_V; ++e) x[v][e] = 0.f;
            if (live[v]) {                                                // (s - off + DEC_V <= ld: 8-aligned rows; s <= tmax < Lcap)
                // aligned 16-byte loads, ONCE per block step; positions past an output's own meet a zero tap (finite history)
                typename Elem<DT>::type raw[DEC_V];
                __builtin_memcpy(raw, __builtin_assume_aligned(row + (size_t)(s - off) * ES, 16), sizeof(raw));
                HY_UNROLL
                for (int e = 0; e < DEC_V; ++e) x[v][e] = Elem<DT>::dec(raw[e]);
            }
        }
        const int slot = shared ? r * a.fan : r;
        float* part = a.part + (((size_t)chunk * a.B + slot) * T) * a.D + c;
        int i0 = 0;
        for (; T - i0 > 3 * DEC_TR; i0 += DEC_TT) {                       // whole tiles, and a remainder of more than three small ones
            float acc[DEC_TT];
            dec_block_tile<DEC_TT>(x, live, ks, tid, i0, acc);
            dec_block_reduce<DEC_TT>(acc, red + DEC_TT * 4 * (trip++ & 1), tid, i0, T, part, a.D);
        }
        for (; i0 < T; i0 += DEC_TR) {
            float acc[DEC_TR];
            dec_block_tile<DEC_TR>(x, live, ks, tid, i0, acc);
            dec_block_reduce<DEC_TR>(acc, red + DEC_TT * 4 * (trip++ & 1), tid, i0, T, part, a.D);
        }
    }
}

// one thread per (b, i, d): grid ceil(B T D / DEC_THREADS).  Nothing here writes pos: decode_advance_block_kernel follows on the stream.
template <int DT>
__global__ void __launch_bounds__(DEC_THREADS) decode_post_block_kernel(DecBlockArgs a) {
    typedef typename Elem<DT>::type elem_t;
    const int t0 = a.pos[0];
    const size_t idx = (size_t)blockIdx.x * DEC_THREADS + threadIdx.x;
    if (idx >= (size_t)a.B * a.T * a.D || !dec_block_valid(a, t0)) return;
    const int d = (int)(idx % a.D), i = (int)(idx / a.D % a.T), b = (int)(idx / a.D / a.T);
    const int t = t0 + i;
    const int nc = t / DEC_CHUNK + 1, ns = a.S / DEC_CHUNK, bs = b / a.fan * a.fan;
    float y = 0.f;
    for (int ch = 0; ch < nc; ++ch) y += a.part[(((size_t)ch * a.B + (ch < ns ? bs : b)) * a.T + i) * a.D + d];
    const float u = Elem<DT>::dec(reinterpret_cast<const elem_t*>(a.vg)[((size_t)b * a.D + d) * a.lda + (t - a.S)]);
    if (a.fb != nullptr) y = __builtin_fmaf(u, a.fb[d], y);
    const float yr = Elem<DT>::dec(Elem<DT>::cvt(y));                     // the forward's convolution output is stored in the I/O type
    reinterpret_cast<elem_t*>(a.z)[idx] = Elem<DT>::cvt(yr * a.x0[idx]);  // cm_post_fwd: y * c0, rounded once
}

// one thread, after decode_post_block_kernel on the same stream: the position advances by T
__global__ void __launch_bounds__(64) decode_advance_block_kernel(int* pos, int T, int S, int Lcap) {
    const int t0 = pos[0];
    if (threadIdx.x == 0 && blockIdx.x == 0 && t0 >= S && t0 <= Lcap - T) pos[0] = t0 + T;
}

// ---- lookahead carry: the history's share of the next W outputs, taken ahead (C ABI: hyena_decode_carry, _conv_la, _post_la) --------------
// The convolution is linear in the history, so with t0 the position at a refresh and t0 <= t < t0 + W
//     y_t = carry[b, t - t0, c] + sum_{s = t0 .. t} k[c, t - s] vg[b, c, s] + fb[c] vg[b, c, t],   carry[b, j, c] = sum_{s < t0} k[c, t0 + j - s] vg[b, c, s]
// One refresh streams the history once for W outputs that are not known yet (decode_conv_block_kernel's tiles and staged window: the W
// outputs of a (row, channel) read the same history vectors); a step then reads the at most W + 7 columns from t0 on.
//   decode_carry_kernel         grid (nchunks, D): part[chunk][b][j][d] for the chunks that start below t0, outputs j < min(W, Lcap - t0).  The
//                               bound s < t0 is taken on the HISTORY VALUE (a column at or past t0 enters as an exact 0, whatever it
//                               holds), not on the tap: tap t0 + j - s is live for the outputs j > s - t0 and dead for the others.
//   decode_carry_reduce_kernel  one thread per (b, j, d): the ceil(t0 / DEC_CHUNK) partials in chunk order -> carry (B, W, D); t0 = 0 gives
//                               exact zeros and no history is read
//   decode_set_base_kernel      one thread, behind them on the stream: *base = t0
//   decode_conv_la_kernel       grid (2, D): decode_conv_kernel with the lower bound lo = *base.  [lo, t] spans at most two chunks (W <=
//                               DEC_TMAX), so workgroup (x, c) takes chunk lo / DEC_CHUNK + x into part[x][b][c]; vectors that end at or
//                               below lo are skipped, columns below lo inside a vector meet a zero tap (they are real, finite history).
//                               The same lanes, FMA order and wave sums as decode_conv_kernel: with lo = 0 the same partial, bit for bit.
//   decode_post_la_kernel       ONE workgroup: carry[b, t - lo, d], then the live partials in chunk order, then decode_post_kernel's tail
// A step parks (nothing is written, the position stays) when t is outside [0, Lcap) or t - lo outside [0, W), or lo is negative.  Every
// branch around a barrier is taken on pos[0] / base[0], W and blockIdx: uniform across the workgroup.
struct DecLaArgs : DecArgs {
    float* carry;       // (B, W, D) fp32
    int* base;          // the position of the last refresh (device memory)
    int W;
};

enum { DEC_KLDS_LA = DEC_TMAX + 8 /* floats: a step's window is the taps 0 .. t - lo < W, rounded outwards to 4 words */ };

__device__ __forceinline__ bool dec_la_valid(const DecLaArgs& a, int t, int lo) {
    return t >= 0 && t < a.Lcap && lo >= 0 && lo <= t && t - lo < a.W;
}

template <int DT>
__global__ void __launch_bounds__(DEC_THREADS) decode_carry_kernel(DecLaArgs a) {
    constexpr size_t ES = CmEs<DT>::V;
    HY_SMEM(smem);
    HY_LDS float* ks = HY_LDS_CAST(float, smem);
    HY_LDS float* red = ks + DEC_KLDS_BLOCK;                             // [2][DEC_TT][4]: wavefront sums, alternating by the parity of the trip
    const int t0 = a.pos[0];
    const int chunk = blockIdx.x, c = blockIdx.y, tid = threadIdx.x;
    const int s0 = chunk * DEC_CHUNK;
    if (t0 < 0 || t0 >= a.Lcap || s0 >= t0) return;                      // (t0 = 0: no workgroup stays)
    const int T = a.W < a.Lcap - t0 ? a.W : a.Lcap - t0;                 // the outputs that lie inside the cache
    // ks[m] = k[c, jlo + m] as in decode_conv_block_kernel; zero past the last output's first tap (k has Lcap columns)
    const int jlo = t0 - s0 - DEC_CHUNK + 1, jhi = t0 + T - 1 - s0;
    const float* krow = a.k + (size_t)c * a.ldk;
    for (int m = tid; m < DEC_KLDS_BLOCK; m += DEC_THREADS) {
        const int j = jlo + m;
        const bool ok = j >= 0 && j <= jhi;
        const float kv = krow[ok ? j : 0];
        ks[m] = ok ? kv : 0.f;
    }
    __syncthreads();
    bool live[DEC_NV];
    HY_UNROLL
    for (int v = 0; v < DEC_NV; ++v) live[v] = s0 + (v * DEC_THREADS + tid) * DEC_V < t0;
    int trip = 0;
    for (int b = 0; b < a.B; ++b) {
        const char* row = cm_row(a.vg, (size_t)b * a.D + c, a.lda, ES);
        float x[DEC_NV][DEC_V];
        HY_UNROLL
        for (int v = 0; v < DEC_NV; ++v) {
            const int s = s0 + (v * DEC_THREADS + tid) * DEC_V;
            HY_UNROLL
            for (int e = 0; e < DEC_V; ++e) x[v][e] = 0.f;
            if (live[v]) {                                                // (s + DEC_V <= lda: 8-aligned rows; s < t0 < Lcap)
                typename Elem<DT>::type raw[DEC_V];
                __builtin_memcpy(raw, __builtin_assume_aligned(row + (size_t)s * ES, 16), sizeof(raw));
                HY_UNROLL
                for (int e = 0; e < DEC_V; ++e) {
                    const float xv = Elem<DT>::dec(raw[e]);
                    x[v][e] = s + e < t0 ? xv : 0.f;                      // the value is selected, not multiplied: s < t0 holds exactly
                }
            }
        }
        float* part = a.part + (((size_t)chunk * a.B + b) * a.W) * a.D + c;
        int i0 = 0;
        for (; T - i0 > 3 * DEC_TR; i0 += DEC_TT) {                       // decode_conv_block_kernel's tiling
            float acc[DEC_TT];
            dec_block_tile<DEC_TT>(x, live, ks, tid, i0, acc);
            dec_block_reduce<DEC_TT>(acc, red + DEC_TT * 4 * (trip++ & 1), tid, i0, T, part, a.D);
        }
        for (; i0 < T; i0 += DEC_TR) {
            float acc[DEC_TR];
            dec_block_tile<DEC_TR>(x, live, ks, tid, i0, acc);
            dec_block_reduce<DEC_TR>(acc, red + DEC_TT * 4 * (trip++ & 1), tid, i0, T, part, a.D);
        }
    }
}

// one thread per (b, j, d): grid ceil(B W D / DEC_THREADS).  Slots j >= Lcap - t0 are not written.
__global__ void __launch_bounds__(DEC_THREADS) decode_carry_reduce_kernel(DecLaArgs a) {
    const int t0 = a.pos[0];
    const size_t idx = (size_t)blockIdx.x * DEC_THREADS + threadIdx.x;
    if (idx >= (size_t)a.B * a.W * a.D || t0 < 0 || t0 >= a.Lcap) return;
    const int d = (int)(idx % a.D), j = (int)(idx / a.D % a.W), b = (int)(idx / a.D / a.W);
    if (j >= a.Lcap - t0) return;
    const int nc = (t0 + DEC_CHUNK - 1) / DEC_CHUNK;
    float y = 0.f;
    for (int ch = 0; ch < nc; ++ch) y += a.part[(((size_t)ch * a.B + b) * a.W + j) * a.D + d];
    a.carry[idx] = y;
}

// one thread, after decode_carry_reduce_kernel on the same stream
__global__ void __launch_bounds__(64) decode_set_base_kernel(const int* pos, int* base, int Lcap) {
    const int t0 = pos[0];
    if (threadIdx.x == 0 && blockIdx.x == 0 && t0 >= 0 && t0 < Lcap) base[0] = t0;
}

// grid (2, D): workgroup (x, c) covers chunk lo / DEC_CHUNK + x of channel c for every b
template <int DT>
__global__ void __launch_bounds__(DEC_THREADS) decode_conv_la_kernel(DecLaArgs a) {
    constexpr size_t ES = CmEs<DT>::V;
    HY_SMEM(smem);
    HY_LDS float* ks = HY_LDS_CAST(float, smem);
    HY_LDS float* red = ks + DEC_KLDS_LA;                                // [2][4]: wavefront sums, alternating by row parity
    const int t = a.pos[0], lo = a.base[0];
    const int c = blockIdx.y, tid = threadIdx.x;
    if (!dec_la_valid(a, t, lo)) return;
    const int s0 = (lo / DEC_CHUNK + (int)blockIdx.x) * DEC_CHUNK;
    if (s0 > t) return;
    // stage the taps jmin .. t - max(s0, lo) (at most W of them), rounded outwards to 4 words, with aligned 16-byte loads
    const int shi = s0 > lo ? s0 : lo;
    const int jmin = t - s0 - DEC_CHUNK + 1 > 0 ? t - s0 - DEC_CHUNK + 1 : 0;
    const int kb = jmin & ~3;
    const int ngroups = (t - shi - kb) / 4 + 1;
    const float* krow = a.k + (size_t)c * a.ldk;
    for (int q = tid; q < ngroups; q += DEC_THREADS) {
        float r[4];
        __builtin_memcpy(r, krow + kb + 4 * q, sizeof(r));
        HY_UNROLL
        for (int e = 0; e < 4; ++e) ks[4 * q + e] = r[e];
    }
    __syncthreads();
    for (int b = 0; b < a.B; ++b) {
        const char* row = cm_row(a.vg, (size_t)b * a.D + c, a.lda, ES);
        float acc = 0.f;
        HY_UNROLL
        for (int v = 0; v < DEC_NV; ++v) {
            const int s = s0 + (v * DEC_THREADS + tid) * DEC_V;
            if (s <= t && s + DEC_V > lo) {                               // (s + DEC_V <= lda: rows are 8-aligned and t < Lcap <= lda)
                // aligned 16-byte loads; positions below lo and past t inside a vector meet a zero tap (the history holds finite values only)
                typename Elem<DT>::type raw[DEC_V];
                __builtin_memcpy(raw, __builtin_assume_aligned(row + (size_t)s * ES, 16), sizeof(raw));
                float x[DEC_V];
                HY_UNROLL
                for (int e = 0; e < DEC_V; ++e) x[e] = Elem<DT>::dec(raw[e]);
                HY_UNROLL
                for (int e = 0; e < DEC_V; ++e) {
                    const bool ok = s + e <= t && s + e >= lo;
                    const float kv = ks[ok ? t - s - e - kb : 0];
                    const float kk = ok ? kv : 0.f;
                    acc = __builtin_fmaf(kk, x[e], acc);
                }
            }
        }
        acc = cm_wave_sum(acc);
        HY_LDS float* rb = red + 4 * (b & 1);
        if ((tid & 63) == 0) rb[tid >> 6] = acc;
        __syncthreads();
        if (tid == 0) a.part[((size_t)blockIdx.x * a.B + b) * a.D + c] = (rb[0] + rb[1]) + (rb[2] + rb[3]);
    }
}

// ONE workgroup: every thread reads t and lo before the barrier, one lane advances the position after
template <int DT>
__global__ void __launch_bounds__(DEC_POST_THREADS) decode_post_la_kernel(DecLaArgs a) {
    typedef typename Elem<DT>::type elem_t;
    const int t = a.pos[0], lo = a.base[0];
    const bool valid = dec_la_valid(a, t, lo);
    if (valid) {
        const int nl = t / DEC_CHUNK - lo / DEC_CHUNK + 1;                    // live chunks: 1 or 2
        const elem_t* vg = reinterpret_cast<const elem_t*>(a.vg);
        elem_t* z = reinterpret_cast<elem_t*>(a.z);
        for (int i = threadIdx.x; i < a.B * a.D; i += DEC_POST_THREADS) {
            const int b = i / a.D, d = i % a.D;
            float y = a.carry[((size_t)b * a.W + (t - lo)) * a.D + d];
            for (int x = 0; x < nl; ++x) y += a.part[((size_t)x * a.B + b) * a.D + d];
            const float u = Elem<DT>::dec(vg[((size_t)b * a.D + d) * a.lda + t]);
            if (a.fb != nullptr) y = __builtin_fmaf(u, a.fb[d], y);
            const float yr = Elem<DT>::dec(Elem<DT>::cvt(y));                 // the forward's convolution output is stored in the I/O type
            z[i] = Elem<DT>::cvt(yr * a.x0[i]);                                // cm_post_fwd: y * c0, rounded once
        }
    }
    __syncthreads();
    if (threadIdx.x == 0 && valid) a.pos[0] = t + 1;
}

// ---- token sampling: the last node of the per-token graph (C ABI: hyena_decode_sample) ---------------------------------------------------
// One wavefront per logit row (V <= 64: lane i holds logit i); workgroup = one wavefront, rows beyond the grid by a grid-stride loop.  The
// row's column c = col[b] and its done flag live in device memory, like the decode positions: one captured graph serves every token, and
// the token goes straight into the graph's static id buffer (`next`) and into column c of the preallocated sequence tensor.
//   rank     r_i = #{ j < Vlive : j comes before i }: a NaN before every number, among NaNs the lower index first; among numbers l_j > l_i, or
//            l_j == l_i and j < i (torch.sort(l, descending=True, stable=True): a permutation of 0 .. Vlive - 1 for EVERY input; equal values,
//            -inf among them, rank by index)
//   greedy   top_k <= 1: the token of rank 0 (torch.argmax); nothing random is drawn
//   total    a row whose rank-0 logit is not finite (a NaN, a +inf, or -inf: every live logit is -inf) emits its rank-0 token whatever top_k,
//            top_p and T are (its masses would be NaN); u is drawn and reported as for any other row
//   top-k    keep r_i < min(top_k, Vlive); p_i = exp((l_i - max l) / T) in fp32, summed IN RANK ORDER (every lane runs the same serial scan
//            over LDS: the sums do not depend on lane count or reduction shape)
//   top-p    the kept tokens whose preceding kept mass is < top_p Z: a prefix in rank order (the masses are >= 0), never empty
//   draw     u = (word 0 of Philox4x32-10(counter (c, b), key seed) >> 8) 2^-24: a pure function of (seed, row, column); the first kept
//            token whose inclusive cumulative mass exceeds u Z', else the last kept one
// A parked row (c outside [0, ncols)) is neither read nor written; a done row writes next = pad and nothing else.  No atomics: lane 0 is the
// only writer of the row's state, after every lane has read it.
enum { SMP_VMAX = 64, SMP_MAX_GRID = 1 << 16, SMP_LDS_BYTES = 4 * SMP_VMAX * 4 };

struct SampleArgs {
    const void* logits;               // (B, V) I/O type, row b at b ldl
    float* scores;                    // (B, ncols, V) fp32 or null: scores[b, c] = l / T
    float* u_out;                     // (B,) fp32 or null: the uniform the row drew
    const unsigned long long* seed;   // device pointer to the 64-bit seed
    int* col;                         // (B,) the column row b writes next
    int* done;                        // (B,) set once row b has emitted eos
    long long* seq;                   // (B, ncols) token ids, row b at b lds
    long long* next;                  // (B,) the model's next input ids, element b at b ldn
    long ldl, lds, ldn;
    int B, V, Vlive, ncols, top_k, eos, pad;
    float T, top_p;
};

template <int DT>
__global__ void __launch_bounds__(SMP_VMAX) decode_sample_kernel(SampleArgs a) {
    typedef typename Elem<DT>::type elem_t;
    HY_SMEM(smem);
    HY_LDS float* sl = HY_LDS_CAST(float, smem);                 // [64] live logits by index
    HY_LDS float* ss = sl + SMP_VMAX;                            // [64] logits by rank
    HY_LDS float* sp = ss + SMP_VMAX;                            // [64] masses by rank
    HY_LDS int* si = HY_LDS_CAST(int, smem) + 3 * SMP_VMAX;      // [64] token by rank
    const int i = threadIdx.x;
    const float ninf = -__builtin_inff();
    // (every branch around a barrier is taken on col[b] / done[b] / top_k: uniform across the wavefront)
    for (long b = blockIdx.x; b < a.B; b += gridDim.x) {
        const int c = a.col[b];
        if (c < 0 || c >= a.ncols) continue;                     // parked
        if (a.done[b] != 0) {
            if (i == 0) a.next[(size_t)b * a.ldn] = a.pad;
            continue;
        }
        float l = ninf;
        if (i < a.V) {
            l = Elem<DT>::dec(reinterpret_cast<const elem_t*>(a.logits)[(size_t)b * a.ldl + i]);
            if (a.scores != nullptr) a.scores[((size_t)b * a.ncols + c) * a.V + i] = l / a.T;
        }
        const bool live = i < a.Vlive;
        sl[i] = live ? l : ninf;
        __syncthreads();                                         // (also orders the previous row's scan before this row's ss / sp / si)
        int r = 0;
        for (int j = 0; j < a.Vlive; ++j) {
            const float lj = sl[j];
            const bool first = lj != lj ? (l == l || j < i) : (lj > l || (lj == l && j < i));   // (a NaN l: both comparisons are false)
            r += first ? 1 : 0;
        }
        if (live) {
            ss[r] = l;
            si[r] = i;
        }
        __syncthreads();
        int tok;
        if (a.top_k <= 1) {
            tok = si[0];
        } else {
            const int k = a.top_k < a.Vlive ? a.top_k : a.Vlive;
            if (live) sp[r] = r < k ? expf((l - ss[0]) / a.T) : 0.f;
            __syncthreads();
            float Z = 0.f;
            for (int q = 0; q < k; ++q) Z += sp[q];
            const float lim = a.top_p * Z;
            int nk = 0;
            float kept = 0.f;                                    // Z': the mass of the nucleus
            while (nk < k && kept < lim) kept += sp[nk++];
            const unsigned long long seed = a.seed[0];
            unsigned rnd[4];
            philox4x32_10((unsigned)c, (unsigned)b, (unsigned)seed, (unsigned)(seed >> 32), rnd);
            const float u = (float)(rnd[0] >> 8) * 5.9604644775390625e-8f;          // 2^-24: exact
            const float target = u * kept;
            const float top = ss[0];
            if (!(top - top == 0.f)) {                           // rank 0 is NaN or +-inf: sp, Z and nk mean nothing
                tok = si[0];
            } else {
                tok = si[nk - 1];
                float acc = 0.f;
                for (int q = 0; q < nk; ++q) {
                    acc += sp[q];
                    if (acc > target) {
                        tok = si[q];
                        break;
                    }
                }
            }
            if (i == 0 && a.u_out != nullptr) a.u_out[b] = u;
        }
        if (i == 0) {
            a.seq[(size_t)b * a.lds + c] = tok;
            a.next[(size_t)b * a.ldn] = tok;
            a.col[b] = c + 1;
            if (tok == a.eos) a.done[b] = 1;
        }
    }
}

// ---- constrained token sampling with token log-probs (C ABI: hyena_decode_sample_constrained) -------------------------------------------------
// decode_sample_kernel with an allowed set per row and new-token number, and the emitted token's log-probability.  With n = c - start[b] the
// number of the row's new token, its mask is allow[b lda + n] (lda = 0: one row of masks for the batch) and
//   A        = { v < Vlive : bit v of the mask }; the whole live vocabulary where allow is null, n lies outside [0, nallow) or no bit below
//            Vlive is set (the kernel ends a captured graph and cannot raise: it stays total)
// Every rule above then reads "A" for "the live tokens": ranks are taken among A (a NaN first, then by value, then by index), greedy takes
// rank 0 of A, k = min(top_k, |A|), the masses are exp((l_i - max_A l) / T) summed in rank order, a row whose rank-0 logit within A is not
// finite emits that token, and u is the same Philox word of (seed, row, column).  eos ends the row when it is emitted, so only where A holds
// it.  With A the live vocabulary every value below is the one decode_sample_kernel computes, operation for operation.
//   logprob  logprobs[b ldp + n] = (l_tok - m) - log(sum_{j < Vlive} exp(l_j - m)), m = max_{j < Vlive} l_j (NaNs skipped by fmaxf): the
//            model's own distribution at T = 1 over ALL live tokens, in fp32, the sum taken serially in index order by every lane from LDS
//            (a pure function of the row's logits; lane j computes the term exp(l_j - m), m being taken in the rank loop).  m or the sum
//            not finite (a live NaN or +inf, or every live logit -inf): NaN.  Written for n in [0, ldp) only.  The terms cross the
//            second barrier with the ranks and l_tok is read back by rank (ss): the row's path has decode_sample_kernel's barriers and
//            no more.
// The mask, start[b] and col[b] are loaded by every lane from one address: every branch around a barrier stays uniform.
enum { SMP_CON_LDS_BYTES = 5 * SMP_VMAX * 4 };
// "these values are needed HERE": their loads are issued, together, before this point.  (The empty statement takes its operands in vector
// registers; the uniform ones go back to scalar registers, so that the branches on them stay scalar branches.)
#if !defined(HIPEMU)
#define SMP_UNIFORM_ISSUED3(x, y, z)                                                                                   \
    do {                                                                                                               \
        asm volatile("" : "+v"(x), "+v"(y), "+v"(z));                                                                \
        x = __builtin_amdgcn_readfirstlane(x); y = __builtin_amdgcn_readfirstlane(y); z = __builtin_amdgcn_readfirstlane(z); \
    } while (0)
#define SMP_ISSUED2_UNIFORM64(x, m)                                                                                    \
    do {                                                                                                               \
        asm volatile("" : "+v"(x), "+v"(m));                                                                         \
        m = ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(m >> 32)) << 32) |                     \
            (unsigned)__builtin_amdgcn_readfirstlane((int)m);                                                          \
    } while (0)
#define SMP_UNIFORM_ISSUED4(x, y, z, w)                                                                                \
    do {                                                                                                               \
        asm volatile("" : "+v"(x), "+v"(y), "+v"(z), "+v"(w));                                                       \
        x = __builtin_amdgcn_readfirstlane(x); y = __builtin_amdgcn_readfirstlane(y); z = __builtin_amdgcn_readfirstlane(z); \
        w = __builtin_amdgcn_readfirstlane(w);                                                                         \
    } while (0)
#else
#define SMP_UNIFORM_ISSUED3(x, y, z) ((void)0)
#define SMP_ISSUED2_UNIFORM64(x, m) ((void)0)
#define SMP_UNIFORM_ISSUED4(x, y, z, w) ((void)0)
#endif

struct SampleConArgs : SampleArgs {
    const unsigned long long* allow;  // (B or 1, nallow) bit masks, row b at b lda, or null
    const int* start;                 // (B,) the column of row b's first new token
    float* logprobs;                  // (B, ldp) fp32 or null
    long lda, ldp;
    int nallow;
};

// The automaton tables of hyena_decode_sample_automaton / hyena_decode_beam_automaton (the semantics stand below decode_sample_con_kernel)
struct AutoTabs {
    int* dstate;                      // (B,) the automaton state of row b
    const unsigned long long* M;      // (Nt, S) allowed sets by (new-token number, state); Nt == 1: one row for every number
    const int* delta;                 // (S, V) the state after token v in state s; -1: forbidden
    int S, Nt;
};

struct SampleAutoArgs : SampleConArgs {   // hyena_decode_sample_automaton (the semantics stand below the kernel)
    AutoTabs t;
};

// AUTO = false, Args = SampleConArgs: the kernel of hyena_decode_sample_constrained, as it has always been (every `if constexpr (AUTO)` is
// discarded); AUTO = true, Args = SampleAutoArgs: the same body with the mask from the automaton's tables
template <int DT, bool AUTO = false, class Args = SampleConArgs>
__global__ void __launch_bounds__(SMP_VMAX) decode_sample_con_kernel(Args a) {
    typedef typename Elem<DT>::type elem_t;
    HY_SMEM(smem);
    HY_LDS float* sl = HY_LDS_CAST(float, smem);                 // [64] live logits by index
    HY_LDS float* ss = sl + SMP_VMAX;                            // [64] allowed logits by rank
    HY_LDS float* sp = ss + SMP_VMAX;                            // [64] masses by rank
    HY_LDS int* si = HY_LDS_CAST(int, smem) + 3 * SMP_VMAX;      // [64] token by rank
    HY_LDS float* se = sl + 4 * SMP_VMAX;                        // [64] exp(l - max l) of the live tokens by index (log-prob)
    const int i = threadIdx.x;
    const float ninf = -__builtin_inff();
    const unsigned long long all = a.Vlive >= 64 ? ~0ull : (1ull << a.Vlive) - 1ull;
    // (every branch around a barrier is taken on col[b] / done[b] / top_k: uniform across the wavefront)
    // The loads are dependent round trips to memory, and they are what this kernel's time is made of.  Left alone the compiler sinks every
    // load behind the branch that guards its use -- five trips in a row.  Here col, done and start (of every row, parked or not) go out
    // together, then the row's logits and its mask together, each group from straight-line code and pinned by SMP_*ISSUED*: two trips.
    // (Lanes from V on read logit 0 and drop it; a row without a mask reads the seed's word and drops it: valid addresses, no branch.)
    const unsigned long long seed = a.top_k > 1 ? a.seed[0] : 0ull;
    const int* first_col = a.start != nullptr ? a.start : a.col;            // (no start: n = 0 -- no mask and no log-prob, the launcher sees to it)
    for (long b = blockIdx.x; b < a.B; b += gridDim.x) {
        int c = a.col[b];
        int fin = a.done[b];
        int c0 = first_col[b];
        int st = 0;                                              // AUTO: the row's state, out with col, done and start -- still two trips
        if constexpr (AUTO) {
            st = a.t.dstate[b];
            SMP_UNIFORM_ISSUED4(c, fin, c0, st);
        } else {
            SMP_UNIFORM_ISSUED3(c, fin, c0);
        }
        if (c < 0 || c >= a.ncols) continue;                     // parked
        if (fin != 0) {
            if (i == 0) a.next[(size_t)b * a.ldn] = a.pad;
            continue;
        }
        const long n = (long)c - c0;
        bool masked;
        const unsigned long long* mp;
        if constexpr (AUTO) {                                    // (a state outside the table: the row samples unmasked and keeps it)
            masked = st >= 0 && st < a.t.S && (a.t.Nt == 1 || (n >= 0 && n < a.t.Nt));
            mp = masked ? a.t.M + ((size_t)(a.t.Nt == 1 ? 0 : n) * a.t.S + st) : a.seed;
        } else {
            masked = a.allow != nullptr && n >= 0 && n < a.nallow;
            mp = masked ? a.allow + ((size_t)b * a.lda + n) : a.seed;
        }
        float l = Elem<DT>::dec(reinterpret_cast<const elem_t*>(a.logits)[(size_t)b * a.ldl + (i < a.V ? i : 0)]);
        unsigned long long m = mp[0];
        SMP_ISSUED2_UNIFORM64(l, m);
        if (!masked) m = 0ull;
        if (i < a.V) {
            if (a.scores != nullptr) a.scores[((size_t)b * a.ncols + c) * a.V + i] = l / a.T;
        } else {
            l = ninf;
        }
        const unsigned long long A = (m & all) != 0ull ? m & all : all;
        const int nA = __builtin_popcountll(A);
        const bool live = i < a.Vlive;
        const bool mine = ((A >> i) & 1ull) != 0ull;             // (A has no bit from Vlive on)
        sl[i] = live ? l : ninf;
        __syncthreads();                                         // (also orders the previous row's scan before this row's ss / sp / si)
        int r = 0;
        float lmax = ninf;
        for (int j = 0; j < a.Vlive; ++j) {
            const float lj = sl[j];
            // decode_sample_kernel's "j comes before i" without a branch (lj is uniform, and a branch on it costs the loop its unrolling):
            // a NaN lj fails both of its comparisons, a NaN l both of its own
            const bool first = ((lj != lj) & ((l == l) | (j < i))) | (lj > l) | ((lj == l) & (j < i));
            r += (first ? 1 : 0) & (int)((A >> j) & 1ull);
            lmax = fmaxf(lmax, lj);                              // over ALL live tokens, NaNs skipped
        }
        if (mine) {
            ss[r] = l;
            si[r] = i;
        }
        const bool want_lp = a.logprobs != nullptr && n >= 0 && n < a.ldp;
        if (want_lp) se[i] = live ? expf(l - lmax) : 0.f;        // by index; read after the barrier below, rewritten after the next row's first
        __syncthreads();
        float lsum = 0.f;
        if (want_lp)
            for (int j = 0; j < a.Vlive; ++j) lsum += se[j];     // serially in index order, the same sum in every lane
        int tok;
        float ltok = ss[0];
        if (a.top_k <= 1) {
            tok = si[0];
        } else {
            const int k = a.top_k < nA ? a.top_k : nA;
            if (mine) sp[r] = r < k ? expf((l - ss[0]) / a.T) : 0.f;
            __syncthreads();
            float Z = 0.f;
            for (int q = 0; q < k; ++q) Z += sp[q];
            const float lim = a.top_p * Z;
            int nk = 0;
            float kept = 0.f;                                    // Z': the mass of the nucleus
            while (nk < k && kept < lim) kept += sp[nk++];
            unsigned rnd[4];
            philox4x32_10((unsigned)c, (unsigned)b, (unsigned)seed, (unsigned)(seed >> 32), rnd);
            const float u = (float)(rnd[0] >> 8) * 5.9604644775390625e-8f;          // 2^-24: exact
            const float target = u * kept;
            const float top = ss[0];
            if (!(top - top == 0.f)) {                           // rank 0 is NaN or +-inf: sp, Z and nk mean nothing
                tok = si[0];
            } else {
                tok = si[nk - 1];
                ltok = ss[nk - 1];
                float acc = 0.f;
                for (int q = 0; q < nk; ++q) {
                    acc += sp[q];
                    if (acc > target) {
                        tok = si[q];
                        ltok = ss[q];
                        break;
                    }
                }
            }
            if (i == 0 && a.u_out != nullptr) a.u_out[b] = u;
        }
        if (i == 0) {
            int ns = -1;                                         // AUTO: the one load of delta, at the tail, in front of the stores
            if constexpr (AUTO)
                if (st >= 0 && st < a.t.S) ns = a.t.delta[(size_t)st * a.V + tok];
            a.seq[(size_t)b * a.lds + c] = tok;
            a.next[(size_t)b * a.ldn] = tok;
            a.col[b] = c + 1;
            if (tok == a.eos) a.done[b] = 1;
            if (want_lp) {
                const bool ok = lmax - lmax == 0.f && lsum - lsum == 0.f;
                a.logprobs[(size_t)b * a.ldp + n] = ok ? (ltok - lmax) - logf(lsum) : __builtin_nanf("");
            }
            if constexpr (AUTO)
                if (ns >= 0 && tok != a.eos) a.t.dstate[b] = ns;   // (eos, or a forbidden token out of the total fall-back: the state stays)
        }
    }
}

// ---- automaton-constrained sampling (C ABI: hyena_decode_sample_automaton) -----------------------------------------------------------------
// decode_sample_con_kernel with the row's mask looked up by the state of a deterministic automaton that the row carries in device memory:
// with s = dstate[b] and n = c - start[b], the mask is M[(Nt == 1 ? 0 : n) S + s] -- M (Nt, S) holds, for every new-token number and state,
// the tokens after which an accepted word can still be completed (the host computes it backwards; Nt == 1: the same row for every n).
// Everything from the mask on is decode_sample_con_kernel operation for operation (one body, a template parameter apart): A, ranks, greedy,
// top-k, top-p, the Philox word of (seed, row, column), the log-prob over all live tokens, and the rule that a mask without a bit below
// Vlive means the whole live vocabulary.  After the token is chosen lane 0 writes dstate[b] = delta[s V + tok].  The state stays as it is
// for a finished row, for a row that has just emitted eos, for a -1 transition (reachable through the total fall-back only) and for an s
// outside [0, S) -- such a row, and one with Nt > 1 and n outside [0, Nt), also samples unmasked.  Parked rows touch nothing.
// Loads: dstate[b] goes out with col, done and start, the mask with the row's logits -- two dependent trips as before; delta is read by
// lane 0 at the tail, in front of the stores.  s, like c, is one address for the wavefront: the branches around barriers stay uniform.

// ---- beam search: the beam step, the cache reorder, the backtrack (C ABI: hyena_decode_beam, _reorder_fan, _beam_backtrack) ------------------
// The k beams of a prompt are the k = `fan` rows of a fan group (row g k + r: rank r of prompt g, best first).  The beam step takes the
// sampler's place as the last compute node of a step: one wavefront per group, grid-stride over the groups, all of its state in device
// memory.  With c = col[g k] (one column per group; outside [0, ncols): parked, nothing of the group is read or written):
//   log-prob    of a live row j: lp[j][i] = (l_i - m) - log(sum_{v < Vlive} exp(l_v - m)), decode_sample_con_kernel's value operation for
//               operation (m by fmaxf in index order, NaNs skipped; the terms expf(l_v - m) summed serially in index order; NaN where m or
//               the sum is not finite).  Lane j walks row j's 64 LDS slots alone -- the k rows' serial scans run side by side.
//   candidates  a live row: every token i of its allowed set A (decode_sample_con_kernel's, the empty-mask rule included) with score
//               beam_score[j] + lp[j][i]; a finished row: ONE candidate, token `pad`, its score unchanged, in slot i = 0.
//   selection   the first k candidates in the order: numbers by score descending (-inf is a number), then NaNs; ties -- equal scores, or
//               two NaNs -- by the flat index j V + i ascending.  A total order for every input.  k rounds: every lane offers the best
//               candidate left in its column i (its k slots are its own), a butterfly of six exchanges over the wavefront leaves the
//               first of the 64 offers in every lane (the order is total: one winner whatever the reduction's shape), its lane
//               strikes it out.  No barrier inside a round.  (A serial scan of the 64 offers from LDS by every lane, the first
//               version, made the kernel 54 us at k = 8 by kernel trace, twelve times the sampler's.)
//   writes      rank r goes to row g k + r: parent (the absolute row of the candidate), beam_score, done (the parent's, or 1 on eos), next
//               (the token; pad for a finished row), col = c + 1, and the records tok_hist / parent_hist / lp_hist [b, n], n = c - start[b],
//               for n inside [0, nrec) (lp of a finished row's pad: 0, so that a beam's records sum to its score).  Lane 0 writes, after
//               the barriers, i.e. after every lane has read the group's state: the sampler's single-writer rule.  No atomics.
// Every row yields a candidate, so k exist; should none be left all the same (it cannot happen), the round yields the row itself with
// `pad` and a NaN score: the kernel stays total.  Every branch around a barrier is taken on col[g k], fan or the loop counters: uniform.
enum { BEAM_MAX = 16, BEAM_LD = SMP_VMAX + 1 /* row pitch in LDS: lane j walks row j, one bank apart */,
       BEAM_LDS_BYTES = (2 * BEAM_MAX * BEAM_LD + 11 * BEAM_MAX) * 4 };

struct BeamArgs {
    const void* logits;               // (B, V) I/O type, row b at b ldl
    float* score;                     // (B,) fp32 cumulative log-probability of the beam in row b
    int* col;                         // (B,) the column row b writes next (one value per group)
    int* done;                        // (B,) set once the beam in row b has emitted eos
    const int* start;                 // (B,) the column of row b's first new token
    int* parent;                      // (B,) out: the row this step's row b continues
    long long* next;                  // (B,) the model's next input ids, element b at b ldn
    const unsigned long long* allow;  // (B or 1, nallow) bit masks, row b at b lda, or null
    int* tok_hist;                    // (B, nrec) records, row b at b ldh, or null
    int* parent_hist;
    float* lp_hist;
    long ldl, ldn, lda, ldh;
    int B, fan, V, Vlive, ncols, eos, pad, nallow, nrec;
};

// "a comes before b" in the selection order; ia, ib: flat indices
__device__ __forceinline__ bool beam_before(float sa, int ia, float sb, int ib) {
    const bool an = sa != sa, bn = sb != sb;
    if (an || bn) return an == bn ? ia < ib : bn;
    return sa > sb || (sa == sb && ia < ib);
}

__device__ __forceinline__ uint32_t beam_f32_bits(float v) { uint32_t u; __builtin_memcpy(&u, &v, 4); return u; }
__device__ __forceinline__ float beam_bits_f32(uint32_t u) { float v; __builtin_memcpy(&v, &u, 4); return v; }

struct BeamAutoArgs : BeamArgs {           // hyena_decode_beam_automaton (the semantics stand below the kernel)
    AutoTabs t;
};

// AUTO = false, Args = BeamArgs: the kernel of hyena_decode_beam, as it has always been (every `if constexpr (AUTO)` is discarded);
// AUTO = true, Args = BeamAutoArgs: the same body with the rows' allowed sets from the automaton's tables
template <int DT, bool AUTO = false, class Args = BeamArgs>
__global__ void __launch_bounds__(SMP_VMAX) decode_beam_kernel(Args a) {
    typedef typename Elem<DT>::type elem_t;
    HY_SMEM(smem);
    HY_LDS float* sl = HY_LDS_CAST(float, smem);                 // [k][BEAM_LD] live logits by (row, index); then the candidates' scores
    HY_LDS float* se = sl + BEAM_MAX * BEAM_LD;                  // [k][BEAM_LD] exp(l - max l); then the candidates' log-probs
    HY_LDS float* smax = se + BEAM_MAX * BEAM_LD;                // [k] max of the live logits of row j
    HY_LDS float* ssum = smax + BEAM_MAX;                        // [k] sum of the terms of row j
    HY_LDS float* rs = ssum + BEAM_MAX;                          // [k] result: score of rank r
    HY_LDS float* rl = rs + BEAM_MAX;                            // [k] result: log-prob of rank r's token
    HY_LDS int* sfin = HY_LDS_CAST(int, rl + BEAM_MAX);          // [k] done flag of row j
    HY_LDS int* rp = sfin + BEAM_MAX;                            // [k] result: row of rank r within the group
    HY_LDS int* rt = rp + BEAM_MAX;                              // [k] result: token of rank r
    HY_LDS int* rd = rt + BEAM_MAX;                              // [k] result: done flag of rank r
    HY_LDS float* ssc = HY_LDS_CAST(float, rd + BEAM_MAX);       // [k] beam_score of row j
    HY_LDS int* sAlo = rd + 2 * BEAM_MAX;                        // [k] allowed set of row j, low and high word
    HY_LDS int* sAhi = sAlo + BEAM_MAX;
    [[maybe_unused]] HY_LDS int* sst = sAhi + BEAM_MAX;          // [k] AUTO: automaton state of row j
    [[maybe_unused]] HY_LDS int* rst = sst + BEAM_MAX;           // [k] AUTO: result: state of rank r
    const int i = threadIdx.x, k = a.fan;
    const float ninf = -__builtin_inff();
    const unsigned long long all = a.Vlive >= 64 ? ~0ull : (1ull << a.Vlive) - 1ull;
    const bool live = i < a.Vlive;
    const int G = a.B / k;
    for (long g = blockIdx.x; g < G; g += gridDim.x) {
        const long b0 = g * k;
        const int c = a.col[b0];
        if (c < 0 || c >= a.ncols) continue;                     // parked (uniform: one address for the wavefront)
        __syncthreads();                                         // the previous group's results have been read by lane 0
        // the rows' logits by (row, index); lane j keeps row j's state
        for (int j = 0; j < k; ++j) {
            const float l = Elem<DT>::dec(reinterpret_cast<const elem_t*>(a.logits)[(size_t)(b0 + j) * a.ldl + (i < a.V ? i : 0)]);
            sl[j * BEAM_LD + i] = live ? l : ninf;
        }
        float sc_row = 0.f;                                      // lane j < k: beam_score, done, mask of row j
        int fin_row = 0;
        unsigned long long A_row = all;
        if (i < k) {
            sc_row = a.score[b0 + i];
            fin_row = a.done[b0 + i];
            const long n = (long)c - a.start[b0 + i];
            if constexpr (AUTO) {
                const int st = a.t.dstate[b0 + i];
                if (st >= 0 && st < a.t.S && (a.t.Nt == 1 || (n >= 0 && n < a.t.Nt))) {
                    const unsigned long long m = a.t.M[(size_t)(a.t.Nt == 1 ? 0 : n) * a.t.S + st] & all;
                    if (m != 0ull) A_row = m;
                }
                sst[i] = st;
            } else {
                if (a.allow != nullptr && n >= 0 && n < a.nallow) {
                    const unsigned long long m = a.allow[(size_t)(b0 + i) * a.lda + n] & all;
                    if (m != 0ull) A_row = m;
                }
            }
            sfin[i] = fin_row;
            ssc[i] = sc_row;
            sAlo[i] = (int)A_row;
            sAhi[i] = (int)(A_row >> 32);
        }
        __syncthreads();
        if (i < k) {
            float lmax = ninf;
            for (int v = 0; v < a.Vlive; ++v) lmax = fmaxf(lmax, sl[i * BEAM_LD + v]);      // over ALL live tokens, NaNs skipped
            smax[i] = lmax;
        }
        __syncthreads();
        for (int j = 0; j < k; ++j) se[j * BEAM_LD + i] = live ? expf(sl[j * BEAM_LD + i] - smax[j]) : 0.f;
        __syncthreads();
        if (i < k) {
            float lsum = 0.f;
            for (int v = 0; v < a.Vlive; ++v) lsum += se[i * BEAM_LD + v];                   // serially in index order
            ssum[i] = lsum;
        }
        __syncthreads();
        // the candidates of column i: slot (j, i) of sl receives the score, of se the log-prob; `mine`: bit j -- candidate (j, i) is in the race
        unsigned mine = 0u;
        for (int j = 0; j < k; ++j) {
            const float sj = ssc[j];
            const unsigned long long Aj = ((unsigned long long)(unsigned)sAhi[j] << 32) | (unsigned)sAlo[j];
            const float lmax = smax[j], lsum = ssum[j];
            const bool ok = lmax - lmax == 0.f && lsum - lsum == 0.f;
            const float lp = ok ? (sl[j * BEAM_LD + i] - lmax) - logf(lsum) : __builtin_nanf("");
            const bool fin = sfin[j] != 0;
            const bool in = fin ? i == 0 : (((Aj >> i) & 1ull) != 0ull);
            sl[j * BEAM_LD + i] = fin ? sj : sj + lp;
            se[j * BEAM_LD + i] = fin ? 0.f : lp;
            mine |= in ? 1u << j : 0u;
        }
        __syncthreads();                                         // (lane 0 reads the winners' log-probs out of other lanes' slots)
        for (int r = 0; r < k; ++r) {
            float best = 0.f;
            int bestj = -1;
            for (int j = 0; j < k; ++j) {
                const float s = sl[j * BEAM_LD + i];
                if (((mine >> j) & 1u) != 0u && (bestj < 0 || beam_before(s, j, best, bestj))) {      // (one column: the flat index orders as j)
                    best = s;
                    bestj = j;
                }
            }
            // the first of the 64 offers in the selection order, by a butterfly over the wavefront: the order is total and the flat indices
            // differ, so the minimum is one candidate whatever the shape of the reduction, and after six exchanges every lane holds it
            float win = best;
            int wflat = bestj < 0 ? -1 : bestj * a.V + i;
            HY_UNROLL
            for (int m = SMP_VMAX / 2; m >= 1; m >>= 1) {
                const float so = beam_bits_f32(HY_SHFL_U32(beam_f32_bits(win), i ^ m));
                const int fo = (int)HY_SHFL_U32((uint32_t)wflat, i ^ m);
                if (fo >= 0 && (wflat < 0 || beam_before(so, fo, win, wflat))) {
                    win = so;
                    wflat = fo;
                }
            }
            const int winj = wflat < 0 ? -1 : wflat / a.V, wini = wflat < 0 ? 0 : wflat % a.V;
            if (winj >= 0 && i == wini) mine &= ~(1u << winj);
            if (i == 0) {
                const bool none = winj < 0;                      // (cannot happen: every row yields a candidate)
                const int pj = none ? r : winj;
                const bool fin = none || sfin[pj] != 0;
                const int tok = fin ? a.pad : wini;
                rp[r] = pj;
                rt[r] = tok;
                rs[r] = none ? __builtin_nanf("") : win;
                rl[r] = none ? 0.f : se[pj * BEAM_LD + wini];
                rd[r] = (sfin[pj] != 0 || (!fin && tok == a.eos)) ? 1 : 0;
            }
        }
        if constexpr (AUTO) {                                    // lane r: the state of rank r, out of its parent's (read before any write)
            __syncthreads();
            if (i < k) {
                const int pj = rp[i], tok = rt[i], ps = sst[pj];
                int ns = ps;                                     // a finished beam's pad, an eos, a state outside the table: the parent's state
                if (sfin[pj] == 0 && tok != a.eos && ps >= 0 && ps < a.t.S) {
                    const int d = a.t.delta[(size_t)ps * a.V + tok];
                    if (d >= 0) ns = d;                          // (-1: through the total fall-back only)
                }
                rst[i] = ns;
            }
            __syncthreads();
        }
        // (lane 0 wrote the results itself; every lane's reads of score / done / start / col lie before the barriers above)
        if (i == 0) {
            for (int r = 0; r < k; ++r) {
                const long b = b0 + r;
                const long n = (long)c - a.start[b];
                if constexpr (AUTO) a.t.dstate[b] = rst[r];
                a.parent[b] = (int)(b0 + rp[r]);
                a.score[b] = rs[r];
                a.done[b] = rd[r];
                a.next[(size_t)b * a.ldn] = rt[r];
                a.col[b] = c + 1;
                if (n >= 0 && n < a.nrec) {
                    if (a.tok_hist != nullptr) a.tok_hist[(size_t)b * a.ldh + n] = rt[r];
                    if (a.parent_hist != nullptr) a.parent_hist[(size_t)b * a.ldh + n] = (int)(b0 + rp[r]);
                    if (a.lp_hist != nullptr) a.lp_hist[(size_t)b * a.ldh + n] = rl[r];
                }
            }
        }
    }
}

// ---- automaton-constrained beam step (C ABI: hyena_decode_beam_automaton) -------------------------------------------------------------------
// decode_beam_kernel with row j's allowed set looked up as the automaton sampler looks it up: lane j < k loads dstate[b0 + j] and
// M[(Nt == 1 ? 0 : n) S + state] with the row's score and done flag, and keeps the state in LDS with the other per-row state -- all k are
// read before any row of the group is written.  The order, the selection rounds and the records are decode_beam_kernel's (one body).  After
// the rounds lane r takes rank r's state out of its parent's: delta[state[parent] V + tok]; the parent's own state for a finished beam's
// pad candidate, for eos, for a -1 transition and for a state outside [0, S) (whose row had the whole live vocabulary).  Lane 0 writes it
// with the rest: the state travels inside the beam kernel, decode_reorder_fan_kernel never sees it.
enum { BEAM_AUTO_LDS_BYTES = BEAM_LDS_BYTES + 2 * BEAM_MAX * 4 };

// Re-parenting the rows of one layer's fan-out cache in place: with t1 = *pos (the position decode_post_fan left) and c0 the first column
// that can differ between the rows of a group (the prompt length),
//     vgr[b, d, s - S] = old vgr[parent[b], d, s - S]  for c0 <= s < t1,      tail[c, b, :] = old tail[c, parent[b], :]  for c < 3 D
// for every row b; a parent outside b's own group counts as b.  t1 outside [S, Lcap]: nothing is written.  The shared tensor, the columns
// below c0 and those from t1 on are never touched.  In place without scratch or a second launch: ONE thread owns one (group, channel,
// column) -- or one (group, tail element) -- for all k rows: it loads the k values through parent[] into registers (the loop is fully
// unrolled to BEAM_MAX with a predicate on j < fan: the address is dynamic, the register index is not), and only then stores them.  No
// other thread reads or writes those addresses.  Consecutive threads take consecutive columns of one row: the accesses coalesce; c0 - S
// has no alignment, so the loads and stores are single elements of the I/O type.  The grid comes from Lcap - c0 on the host with a
// grid-stride loop, the live range from *pos: one captured launch serves every token.
// Bytes per layer and step: 2 B D (t1 - c0) sizeof(io) (+ 2 * 6 B D * 4 for the tails) -- linear in the number of new tokens, independent
// of the prompt.
struct ReorderArgs {
    void* vg;                         // per-row history (Bcap, D, lda) I/O type, column s at s - S
    float* tail;                      // (3D, Bcap, 2) fp32
    const int* parent;                // (B,)
    const int* pos;                   // t1
    int B, Bcap, fan, D, Lcap, S, c0, lda;
};

template <int DT>
__global__ void __launch_bounds__(DEC_THREADS) decode_reorder_fan_kernel(ReorderArgs a) {
    typedef typename Elem<DT>::type elem_t;
    const int t1 = a.pos[0];
    if (t1 < a.S || t1 > a.Lcap) return;
    const int k = a.fan;
    const size_t W = (size_t)(a.Lcap - a.c0);                    // columns a thread index can stand for
    const size_t nh = (size_t)(a.B / k) * a.D * W, nt = (size_t)(a.B / k) * a.D * 6;
    elem_t* vg = reinterpret_cast<elem_t*>(a.vg);
    for (size_t idx = (size_t)blockIdx.x * DEC_THREADS + threadIdx.x; idx < nh + nt; idx += (size_t)gridDim.x * DEC_THREADS) {
        if (idx < nh) {
            const int s = a.c0 + (int)(idx % W);
            if (s >= t1) continue;
            const size_t gd = idx / W;
            const int g = (int)(gd / a.D), d = (int)(gd % a.D);
            const int b0 = g * k;
            const size_t off = (size_t)d * a.lda + (size_t)(s - a.S);
            elem_t v[BEAM_MAX];
            HY_UNROLL
            for (int j = 0; j < BEAM_MAX; ++j) {
                if (j < k) {
                    int p = a.parent[b0 + j];
                    if (p < b0 || p >= b0 + k) p = b0 + j;
                    v[j] = vg[(size_t)p * a.D * a.lda + off];
                }
            }
            HY_UNROLL
            for (int j = 0; j < BEAM_MAX; ++j)
                if (j < k) vg[(size_t)(b0 + j) * a.D * a.lda + off] = v[j];
        } else {
            const size_t q = idx - nh;                            // (g, c, e): consecutive threads, consecutive floats of one tail row
            const int e = (int)(q % 2);
            const size_t gc = q / 2;
            const int c = (int)(gc % (3 * (size_t)a.D)), g = (int)(gc / (3 * (size_t)a.D));
            const int b0 = g * k;
            float* row = a.tail + (size_t)c * a.Bcap * 2 + e;
            float v[BEAM_MAX];
            HY_UNROLL
            for (int j = 0; j < BEAM_MAX; ++j) {
                if (j < k) {
                    int p = a.parent[b0 + j];
                    if (p < b0 || p >= b0 + k) p = b0 + j;
                    v[j] = row[(size_t)p * 2];
                }
            }
            HY_UNROLL
            for (int j = 0; j < BEAM_MAX; ++j)
                if (j < k) row[(size_t)(b0 + j) * 2] = v[j];
        }
    }
}

// After the last step: one thread per returned row q = g n_ret + r walks the records from step n_done - 1 back to step 0, starting at row
// g k + r (rank r of group g): token and log-prob of step i from the row it stands in, then on to that row's parent of step i (a parent
// outside [0, B) counts as the row itself).  seq[q, P + i] and, where asked for, logprobs[q, i] for i < n_done.
struct BacktrackArgs {
    const int* tok_hist;              // (B, >= n_done) records, row b at b ldh
    const int* parent_hist;
    const float* lp_hist;             // or null
    long long* seq;                   // (G n_ret, >= P + n_done), row q at q lds
    float* logprobs;                  // (G n_ret, >= n_done), row q at q ldp, or null
    long ldh, lds, ldp;
    int B, fan, n_done, n_ret, P;
};

__global__ void __launch_bounds__(DEC_THREADS) decode_beam_backtrack_kernel(BacktrackArgs a) {
    const long q = (long)blockIdx.x * DEC_THREADS + threadIdx.x;
    if (q >= (long)(a.B / a.fan) * a.n_ret) return;
    long b = q / a.n_ret * a.fan + q % a.n_ret;
    for (int i = a.n_done - 1; i >= 0; --i) {
        a.seq[(size_t)q * a.lds + a.P + i] = a.tok_hist[(size_t)b * a.ldh + i];
        if (a.logprobs != nullptr) a.logprobs[(size_t)q * a.ldp + i] = a.lp_hist[(size_t)b * a.ldh + i];
        const int p = a.parent_hist[(size_t)b * a.ldh + i];
        if (p >= 0 && p < a.B) b = p;
    }
}

}  // namespace hyena
