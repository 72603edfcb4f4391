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

// ---- token sampling: the last node of the per-token graph (C ABI: hyena_decode_sample) ---------------------------------------------------
// One wavefront per logit row (V <= 64: lane i holds logit i); workgroup = one wavefront, rows beyond the grid by a grid-stride loop.  The
// row's column c = col[b] and its done flag live in device memory, like the decode positions: one captured graph serves every token, and
// the token goes straight into the graph's static id buffer (`next`) and into column c of the preallocated sequence tensor.
//   rank     r_i = #{ j < Vlive : l_j > l_i, or l_j == l_i and j < i }       (a permutation of 0 .. Vlive - 1; -inf logits rank by index)
//   greedy   top_k <= 1: the token of rank 0; nothing random is drawn
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
            r += (lj > l || (lj == l && j < i)) ? 1 : 0;
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
            tok = si[nk - 1];
            float acc = 0.f;
            for (int q = 0; q < nk; ++q) {
                acc += sp[q];
                if (acc > target) {
                    tok = si[q];
                    break;
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

}  // namespace hyena
