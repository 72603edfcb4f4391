// block_kernels.h -- the residual glue of a HyenaDNA block around the mixer: (dropout ->) add -> LayerNorm, fused.
//
// Reference (prenorm block, src/models/sequence/simple_lm.py:267-271 / 280-284, long_conv_lm.py:381-396; the fused path
// the reference takes when flash_attn is installed is flash_attn.ops.layer_norm.dropout_add_layer_norm):
//     residual' = dropout(x0) + residual            (fp32 when residual_in_fp32)
//     out       = LayerNorm(residual'; weight, bias, eps)
// returning (out, residual') for prenorm blocks, out alone for the final norm.  HyenaDNA trains with residual dropout 0 and an
// embedding dropout of 0.1, which the reference applies as the FIRST block's dropout (long_conv_lm.py: resid_dropout1 = embed_dropout
// for layer 0).  Dropout (round 4) is part of the pass: the keep / drop decision of element i is a pure function of (seed, i) -- Philox
// 4x32-10, four consecutive elements per call -- so the backward regenerates it and no mask tensor exists (PyTorch's unfused dropout
// reads and writes the activation once more in each direction and keeps a byte per element: 0.86 ms per step at 2^20 x 256 fp32).
//
// One pass forward (read x0, residual; write out, residual'; + mean / rstd per row), one pass backward (read dout,
// residual', d residual'; write dx0 = d residual; per-workgroup partial weight / bias gradients, summed in a fixed
// order by filter_reduce_kernel).  A wavefront owns one row: lane l holds the E = D / 64 consecutive channels l E ..
// l E + E - 1 (one 16-byte access per tensor at D = 256), row statistics by a 6-step butterfly over the wavefront.
// Unfused, PyTorch spends an add, a cast, a LayerNorm and (under autocast) another cast on this: ~2.5x the traffic.
#pragma once
#include "fftconv_kernels.h"

namespace hyena {

enum { BLK_WAVES = 4, BLK_THREADS = BLK_WAVES * 64, BLK_MAX_GRID = 2048, BLK_VMAX = 16 /* token classes of the EMB kernels (the DNA vocabulary: 12 -> 16) */ };

struct AddNormArgs {
    const void* x;          // (rows, D) elements of XDT        fwd: x0          bwd: dout
    const float* res_in;    // (rows, D) fp32 or null           fwd: residual    bwd: gradient w.r.t. residual' (or null)
    const float* weight;    // (D,)
    const float* bias;      // (D,)  fwd only
    void* out;              // (rows, D) elements of ODT        fwd: out         bwd: dx0
    float* res_out;         // (rows, D) fp32                   fwd: residual'   bwd: gradient w.r.t. residual (or null)
    const float* saved;     // bwd: residual' as written by the forward
    float* mean;            // (rows,)  fwd: out, bwd: in
    float* rstd;            // (rows,)
    float* part;            // bwd: [gridDim.x][np][D] partial (dweight | dbias [| column sums of the dx0 values as stored])
    int np = 2;             // bwd: 2, or 3: also the column sums of dx0 -- the bias gradient of the linear layer that produced x0 (out_proj, fc2:
                            // round 6; their own streaming pass over dx0 cost 94 us each at 2^20 x 256)
    long rows;
    int D;
    float eps;
    const long long* ids;   // EMB kernels: (rows,) token ids; x0[row] = table[ids[row]] with table = `x` (V_MAX rows at most, fp32) -- the embedding
                            // is never materialised; the backward returns per-token-class sums of d x0 instead of d x0 (part_e)
    float* part_e;          // EMB bwd: [gridDim.x][BLK_VMAX][D] partial sums of the embedding gradient
    const unsigned long long* seed;   // device pointer to the 64-bit dropout seed, or null: no dropout
    unsigned drop_below;              // an element is dropped when its 32 random bits are < drop_below (= p * 2^32)
    float keep_scale;                 // 1 / (1 - p)
    int V;                            // EMB kernels: rows of the embedding table.  An id outside [0, V) reads NO memory: the forward poisons that
                                      // row of out / residual' with NaN (F.embedding, which this pass replaces, device-asserts there), the
                                      // backward leaves it out of every sum
};

// Philox 4x32-10 (Salmon et al., SC'11): counter (c0, c1, 0, 0), key (k0, k1) -> four 32-bit words
__device__ __forceinline__ void philox4x32_10(unsigned c0, unsigned c1, unsigned k0, unsigned k1, unsigned (&out)[4]) {
    unsigned x0 = c0, x1 = c1, x2 = 0u, x3 = 0u;
    HY_UNROLL
    for (int r = 0; r < 10; ++r) {
        const unsigned long long p0 = (unsigned long long)0xD2511F53u * x0, p1 = (unsigned long long)0xCD9E8D57u * x2;
        const unsigned n0 = (unsigned)(p1 >> 32) ^ x1 ^ k0, n1 = (unsigned)p1, n2 = (unsigned)(p0 >> 32) ^ x3 ^ k1, n3 = (unsigned)p0;
        x0 = n0; x1 = n1; x2 = n2; x3 = n3;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    out[0] = x0; out[1] = x1; out[2] = x2; out[3] = x3;
}
// v[e] -> dropout(v[e]) for the E consecutive elements starting at linear index `off` (a multiple of E; E a multiple of 4 or E < 4)
template <int E>
__device__ __forceinline__ void blk_dropout(float (&v)[E], size_t off, unsigned long long seed, unsigned drop_below, float keep_scale) {
    HY_UNROLL
    for (int q = 0; q < (E + 3) / 4; ++q) {
        const size_t idx = (off + 4 * q) >> 2;                  // one Philox call per aligned group of four elements
        unsigned rnd[4];
        philox4x32_10((unsigned)idx, (unsigned)(idx >> 32), (unsigned)seed, (unsigned)(seed >> 32), rnd);
        HY_UNROLL
        for (int i = 0; i < 4 && 4 * q + i < E; ++i) {
            const unsigned word = rnd[(off + 4 * q + i) & 3];   // E < 4: the lane's elements are a part of an aligned group
            v[4 * q + i] = word < drop_below ? 0.f : v[4 * q + i] * keep_scale;
        }
    }
}

__device__ __forceinline__ float wave_sum(float v) {
    HY_UNROLL
    for (int m = 32; m >= 1; m >>= 1) v += u2f(HY_SHFL_U32(f2u(v), (int)((threadIdx.x & 63) ^ m)));
    return v;
}

// E consecutive elements of a row as ONE access (rows start at multiples of D elements and c0 = lane * E, so the
// address is a multiple of E elements: 16 bytes for fp32 at D = 256, 8 bytes for 16-bit types)
template <int DT, int E>
__device__ __forceinline__ void blk_load(const void* base, size_t off, float (&v)[E]) {
    typedef typename Elem<DT>::type elem_t;
    struct __attribute__((aligned(sizeof(elem_t) * (E > 4 ? 4 : E)))) Raw { elem_t e[E]; } raw;
    raw = *reinterpret_cast<const Raw*>(reinterpret_cast<const elem_t*>(base) + off);
    HY_UNROLL
    for (int e = 0; e < E; ++e) v[e] = Elem<DT>::dec(raw.e[e]);
}
template <int DT, int E>
__device__ __forceinline__ void blk_store(void* base, size_t off, const float (&v)[E]) {
    typedef typename Elem<DT>::type elem_t;
    struct __attribute__((aligned(sizeof(elem_t) * (E > 4 ? 4 : E)))) Raw { elem_t e[E]; } raw;
    HY_UNROLL
    for (int e = 0; e < E; ++e) raw.e[e] = Elem<DT>::cvt(v[e]);
    *reinterpret_cast<Raw*>(reinterpret_cast<elem_t*>(base) + off) = raw;
}

template <int XDT, int ODT, int E, bool EMB = false>
__global__ void __launch_bounds__(BLK_THREADS) add_norm_fwd_kernel(AddNormArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c0 = lane * E;
    float w[E], b[E];
    HY_UNROLL
    for (int e = 0; e < E; ++e) { w[e] = a.weight[c0 + e]; b[e] = a.bias[c0 + e]; }
    const float inv_d = 1.f / (float)a.D;
    const unsigned long long seed = a.seed != nullptr ? *a.seed : 0ull;
    for (long row = (long)blockIdx.x * BLK_WAVES + wave; row < a.rows; row += (long)gridDim.x * BLK_WAVES) {
        const size_t off = (size_t)row * a.D + c0;
        float r[E];
        const long long id = EMB ? a.ids[row] : 0;
        const bool bad_id = EMB && (unsigned long long)id >= (unsigned long long)a.V;   // never index the table with it
        blk_load<XDT, E>(a.x, EMB ? (size_t)(bad_id ? 0 : id) * a.D + c0 : off, r);          // EMB: the row of the embedding table
        if (a.seed != nullptr) blk_dropout<E>(r, off, seed, a.drop_below, a.keep_scale);
        if (bad_id) {                                        // (after the dropout: the whole row, not only its kept elements)
            HY_UNROLL
            for (int e = 0; e < E; ++e) r[e] = __builtin_nanf("");
        }
        if (a.res_in != nullptr) {
            float q[E];
            blk_load<DT_F32, E>(a.res_in, off, q);
            HY_UNROLL
            for (int e = 0; e < E; ++e) r[e] += q[e];
        }
        float s = 0.f;
        HY_UNROLL
        for (int e = 0; e < E; ++e) s += r[e];
        const float mean = wave_sum(s) * inv_d;
        float v = 0.f;
        HY_UNROLL
        for (int e = 0; e < E; ++e) v += (r[e] - mean) * (r[e] - mean);
        const float rstd = 1.f / sqrtf(wave_sum(v) * inv_d + a.eps);
        float o[E];
        HY_UNROLL
        for (int e = 0; e < E; ++e) o[e] = (r[e] - mean) * rstd * w[e] + b[e];
        blk_store<ODT, E>(a.out, off, o);
        blk_store<DT_F32, E>(a.res_out, off, r);
        if (lane == 0) { a.mean[row] = mean; a.rstd[row] = rstd; }
    }
}

template <int GDT, int ODT, int E, bool EMB = false>
__global__ void __launch_bounds__(BLK_THREADS) add_norm_bwd_kernel(AddNormArgs a) {
    HY_SMEM(smem);
    HY_LDS float* red = HY_LDS_CAST(float, smem);            // [BLK_WAVES][np][64 * E]  (EMB: also [BLK_VMAX][64 * E], whichever is larger)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c0 = lane * E;
    float w[E], dw[E], db[E], dxs[E];
    HY_UNROLL
    for (int e = 0; e < E; ++e) { w[e] = a.weight[c0 + e]; dw[e] = 0.f; db[e] = 0.f; dxs[e] = 0.f; }
    const int np = EMB ? 2 : a.np;
    float eacc[EMB ? BLK_VMAX : 1][E];                       // EMB: this wavefront's sums of d x0 per token class (its rows, in order)
    HY_UNROLL
    for (int q = 0; q < (EMB ? BLK_VMAX : 1); ++q) {
        HY_UNROLL
        for (int e = 0; e < E; ++e) eacc[q][e] = 0.f;
    }
    const float inv_d = 1.f / (float)a.D;
    const unsigned long long seed = a.seed != nullptr ? *a.seed : 0ull;
    for (long row = (long)blockIdx.x * BLK_WAVES + wave; row < a.rows; row += (long)gridDim.x * BLK_WAVES) {
        const size_t off = (size_t)row * a.D + c0;
        float g[E], r[E];
        blk_load<GDT, E>(a.x, off, g);
        blk_load<DT_F32, E>(a.saved, off, r);
        const float mean = a.mean[row], rstd = a.rstd[row];
        // EMB: the row's token class, wave-uniform; -1: no class -- the forward left NaN in `saved`, the row joins no sum
        const int v = EMB ? HY_SGPR((unsigned long long)a.ids[row] < (unsigned long long)a.V ? (int)a.ids[row] : -1) : 0;
        float s1 = 0.f, s2 = 0.f, xh[E];
        HY_UNROLL
        for (int e = 0; e < E; ++e) {
            xh[e] = (r[e] - mean) * rstd;
            const float dxh = g[e] * w[e];
            s1 += dxh;
            s2 += dxh * xh[e];
            if (EMB) {                                       // the same operations on a copy, kept only for a row with a class (a select, no branch)
                const float dwn = dw[e] + g[e] * xh[e], dbn = db[e] + g[e];
                dw[e] = v >= 0 ? dwn : dw[e];
                db[e] = v >= 0 ? dbn : db[e];
            } else {
                dw[e] += g[e] * xh[e];
                db[e] += g[e];
            }
        }
        s1 = wave_sum(s1) * inv_d;
        s2 = wave_sum(s2) * inv_d;
        float dr[E];
        HY_UNROLL
        for (int e = 0; e < E; ++e) dr[e] = rstd * (g[e] * w[e] - s1 - xh[e] * s2);
        if (a.res_in != nullptr) {
            float h[E];
            blk_load<DT_F32, E>(a.res_in, off, h);
            HY_UNROLL
            for (int e = 0; e < E; ++e) dr[e] += h[e];
        }
        if (a.res_out != nullptr) blk_store<DT_F32, E>(a.res_out, off, dr);
        if (a.seed != nullptr) blk_dropout<E>(dr, off, seed, a.drop_below, a.keep_scale);      // d x0 = d residual' through the same mask
        if (EMB) {
            HY_UNROLL
            for (int q = 0; q < BLK_VMAX; ++q) {
                if (v == q) {
                    HY_UNROLL
                    for (int e = 0; e < E; ++e) eacc[EMB ? q : 0][e] += dr[e];
                }
            }
        } else {
            blk_store<ODT, E>(a.out, off, dr);
            if (np == 3) {                                   // (the values as stored: what a column sum over the dx0 tensor would read)
                HY_UNROLL
                for (int e = 0; e < E; ++e) dxs[e] += Elem<ODT>::dec(Elem<ODT>::cvt(dr[e]));
            }
        }
    }
    const int D = 64 * E;
    if (EMB) {
        // embedding-gradient partials of this workgroup: the 4 wavefronts add their sums into the LDS image one after the other
        HY_UNROLL
        for (int wv = 0; wv < BLK_WAVES; ++wv) {
            if (wave == wv) {
                HY_UNROLL
                for (int q = 0; q < BLK_VMAX; ++q) {
                    HY_UNROLL
                    for (int e = 0; e < E; ++e) {
                        HY_LDS float* slot = red + q * D + c0 + e;
                        *slot = wv == 0 ? eacc[EMB ? q : 0][e] : *slot + eacc[EMB ? q : 0][e];
                    }
                }
            }
            __syncthreads();
        }
        for (int i = threadIdx.x; i < BLK_VMAX * D; i += BLK_THREADS) a.part_e[(size_t)blockIdx.x * BLK_VMAX * D + i] = red[i];
        __syncthreads();
    }
    // weight / bias gradient partials of this workgroup: the 4 wavefronts are added in order
    HY_UNROLL
    for (int e = 0; e < E; ++e) {
        red[(wave * np + 0) * D + c0 + e] = dw[e];
        red[(wave * np + 1) * D + c0 + e] = db[e];
        if (np == 3) red[(wave * np + 2) * D + c0 + e] = dxs[e];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < np * D; i += BLK_THREADS) {
        float s = 0.f;
        HY_UNROLL
        for (int q = 0; q < BLK_WAVES; ++q) s += red[q * np * D + i];
        a.part[(size_t)blockIdx.x * np * D + i] = s;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// The FIRST block's norm with a soft prompt in front of the tokens (evals/soft_prompting_genomics.py LitModel.forward:
// torch.cat([repeat(soft_tokens_drop(soft_tokens), 'n d -> b n d'), embeddings(x)], 1) -> layers[0]):
//     x0[b, t]  = softdrop(soft)[t]             t < n         (n learnable rows of D fp32, shared by the batch)
//               = table[ids[b, t - n]]          t >= n
//     residual' = dropout(x0),   out = LayerNorm(residual')   over the B (n + L) rows, arithmetic of add_norm_fwd_kernel
// Neither the embedding nor the concatenation is stored.  Two dropouts: the block's, per element of the (B, n + L, D) output from
// (seed, linear index) as in the plain kernel; the soft tokens', per element of (n, D) from (soft_seed, t D + c) -- the same for
// every batch row (the reference drops before `repeat`).  The backbone is frozen on this route, so the backward returns d soft
// alone and reads only the B n soft rows: a wavefront owns a soft position t and adds the rows b = 0 .. B - 1 in order -- no
// atomics, no partial buffer, one launch, every element of d_soft written.
// ---------------------------------------------------------------------------------------------------------------
// no multiply of an earlier statement is fused into the additions of the compound statement this opens (hipcc contracts across statements)
#ifdef HIPEMU
#define HY_NO_CONTRACT
#else
#define HY_NO_CONTRACT _Pragma("clang fp contract(off)")
#endif
enum { SOFT_BATCH_UNROLL = 4 /* batch rows of a soft position whose loads are in flight together (bwd) */ };

struct SoftNormArgs {
    const long long* ids;   // (B, L) token ids                 fwd
    const float* table;     // (V, D) fp32                      fwd
    const float* soft;      // (n, D) fp32                      fwd
    const void* dout;       // (B (n + L), D) elements of GDT   bwd
    const float* dres;      // (B (n + L), D) fp32 or null      bwd: gradient w.r.t. residual'
    const float* saved;     // bwd: residual' as written by the forward
    const float* weight;    // (D,)
    const float* bias;      // (D,)  fwd only
    void* out;              // fwd: (B (n + L), D) elements of ODT
    float* res_out;         // fwd: residual' fp32
    float* mean;            // (B (n + L),)  fwd: out, bwd: in
    float* rstd;
    float* d_soft;          // bwd: (n, D) fp32
    int B;
    long n, L;
    int D, V;
    float eps;
    const unsigned long long* seed;        // the block's dropout (null: none), as AddNormArgs
    unsigned drop_below;
    float keep_scale;
    const unsigned long long* soft_seed;   // the soft tokens' dropout (null: none)
    unsigned soft_drop_below;
    float soft_keep_scale;
};

template <int ODT, int E>
__global__ void __launch_bounds__(BLK_THREADS) soft_embed_add_norm_fwd_kernel(SoftNormArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c0 = lane * E;
    float w[E], b[E];
    HY_UNROLL
    for (int e = 0; e < E; ++e) { w[e] = a.weight[c0 + e]; b[e] = a.bias[c0 + e]; }
    const float inv_d = 1.f / (float)a.D;
    const unsigned long long seed = a.seed != nullptr ? *a.seed : 0ull;
    const unsigned long long sseed = a.soft_seed != nullptr ? *a.soft_seed : 0ull;
    const long T = a.n + a.L, rows = (long)a.B * T;
    // (batch row, position) of a row without a division per row: one for the first row, one for the stride
    const long row0 = (long)blockIdx.x * BLK_WAVES + wave, stride = (long)gridDim.x * BLK_WAVES;
    const long stride_b = stride / T, stride_t = stride - stride_b * T;
    long bi = row0 / T, t = row0 - bi * T;                   // wave-uniform
    for (long row = row0; row < rows; row += stride, bi += stride_b, t += stride_t) {
        if (t >= T) { t -= T; ++bi; }
        const size_t off = (size_t)row * a.D + c0;
        float r[E];
        bool bad_id = false;
        if (t < a.n) {
            const size_t soff = (size_t)t * a.D + c0;
            blk_load<DT_F32, E>(a.soft, soff, r);
            if (a.soft_seed != nullptr) blk_dropout<E>(r, soff, sseed, a.soft_drop_below, a.soft_keep_scale);
        } else {
            const long long id = a.ids[bi * a.L + (t - a.n)];
            bad_id = (unsigned long long)id >= (unsigned long long)a.V;                        // never index the table with it
            blk_load<DT_F32, E>(a.table, (size_t)(bad_id ? 0 : id) * a.D + c0, r);
        }
        if (a.seed != nullptr) blk_dropout<E>(r, off, seed, a.drop_below, a.keep_scale);
        if (bad_id) {
            HY_UNROLL
            for (int e = 0; e < E; ++e) r[e] = __builtin_nanf("");
        }
        float s = 0.f;
        HY_UNROLL
        for (int e = 0; e < E; ++e) s += r[e];
        const float mean = wave_sum(s) * inv_d;
        float v = 0.f;
        HY_UNROLL
        for (int e = 0; e < E; ++e) v += (r[e] - mean) * (r[e] - mean);
        const float rstd = 1.f / sqrtf(wave_sum(v) * inv_d + a.eps);
        float o[E];
        HY_UNROLL
        for (int e = 0; e < E; ++e) o[e] = (r[e] - mean) * rstd * w[e] + b[e];
        blk_store<ODT, E>(a.out, off, o);
        blk_store<DT_F32, E>(a.res_out, off, r);
        if (lane == 0) { a.mean[row] = mean; a.rstd[row] = rstd; }
    }
}

template <int GDT, int E>
__global__ void __launch_bounds__(BLK_THREADS) soft_embed_add_norm_bwd_kernel(SoftNormArgs a) {
    enum { U = SOFT_BATCH_UNROLL };
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c0 = lane * E;
    float w[E];
    HY_UNROLL
    for (int e = 0; e < E; ++e) w[e] = a.weight[c0 + e];
    const float inv_d = 1.f / (float)a.D;
    const unsigned long long seed = a.seed != nullptr ? *a.seed : 0ull;
    const unsigned long long sseed = a.soft_seed != nullptr ? *a.soft_seed : 0ull;
    const long T = a.n + a.L;
    for (long t = (long)blockIdx.x * BLK_WAVES + wave; t < a.n; t += (long)gridDim.x * BLK_WAVES) {
        float acc[E];
        HY_UNROLL
        for (int e = 0; e < E; ++e) acc[e] = 0.f;
        for (int b0 = 0; b0 < a.B; b0 += U) {
            // the loads of up to U consecutive batch rows first (independent: all in flight), then their arithmetic in the order of b; a
            // slot past the batch (wave-uniform) issues no load and no arithmetic
            float g[U][E], r[U][E], h[U][E], mean[U], rstd[U];
            size_t off[U];
            HY_UNROLL
            for (int u = 0; u < U; ++u) {
                if (b0 + u >= a.B) break;
                const long row = (long)(b0 + u) * T + t;
                off[u] = (size_t)row * a.D + c0;
                blk_load<GDT, E>(a.dout, off[u], g[u]);
                blk_load<DT_F32, E>(a.saved, off[u], r[u]);
                mean[u] = a.mean[row];
                rstd[u] = a.rstd[row];
                if (a.dres != nullptr) blk_load<DT_F32, E>(a.dres, off[u], h[u]);
            }
            HY_UNROLL
            for (int u = 0; u < U; ++u) {
                if (b0 + u >= a.B) break;
                float s1 = 0.f, s2 = 0.f, xh[E];
                HY_UNROLL
                for (int e = 0; e < E; ++e) {
                    xh[e] = (r[u][e] - mean[u]) * rstd[u];
                    const float dxh = g[u][e] * w[e];
                    s1 += dxh;
                    s2 += dxh * xh[e];
                }
                s1 = wave_sum(s1) * inv_d;
                s2 = wave_sum(s2) * inv_d;
                float dr[E];
                HY_UNROLL
                for (int e = 0; e < E; ++e) dr[e] = rstd[u] * (g[u][e] * w[e] - s1 - xh[e] * s2);
                if (a.dres != nullptr) {
                    // (dr is rounded before this add, as in add_norm_bwd_kernel: the sum over b is held to that kernel's dx0 bit for bit)
                    HY_NO_CONTRACT
                    HY_UNROLL
                    for (int e = 0; e < E; ++e) dr[e] += h[u][e];
                }
                if (a.seed != nullptr) blk_dropout<E>(dr, off[u], seed, a.drop_below, a.keep_scale);
                {
                    HY_NO_CONTRACT                           // (the scaled dx0 of a row is rounded before it joins the sum)
                    HY_UNROLL
                    for (int e = 0; e < E; ++e) acc[e] = b0 + u == 0 ? dr[e] : acc[e] + dr[e];
                }
            }
        }
        const size_t soff = (size_t)t * a.D + c0;
        if (a.soft_seed != nullptr) blk_dropout<E>(acc, soff, sseed, a.soft_drop_below, a.soft_keep_scale);
        blk_store<DT_F32, E>(a.d_soft, soff, acc);
    }
}

#undef HY_NO_CONTRACT

// ---------------------------------------------------------------------------------------------------------------
// A row-wise language-model head for the few rows a soft-prompt readout keeps: out[row, v] = sum_c x[row, c] W[v, c], V <= BLK_VMAX token
// classes.  A library GEMM picks its kernel -- and the order of its additions -- from the row count, so the logits of B n_pos gathered rows
// are not the bits of the same rows among B L; here a wavefront owns a row (lane l the E channels from l E on, W in registers), every
// product is accumulated in one fixed order (the lane's E channels, then the 6-step butterfly), and a row's logits do not depend on which
// other rows the call holds.  x, W and out share one type (fp32, or the 16-bit autocast type: nn.Linear's semantics), sums in fp32.
// The backward returns dx alone (the head is frozen on this route): dx[row, c] = sum_v dy[row, v] W[v, c], v in order, lane-local.
// ---------------------------------------------------------------------------------------------------------------
struct RowHeadArgs {
    const void* x;          // fwd: (rows, D) elements of DT    bwd: dy (rows, V)
    const void* w;          // (V, D) elements of DT
    void* out;              // fwd: (rows, V)                   bwd: dx (rows, D)
    long rows;
    int V, D;
};

template <int DT, int E, bool BWD>
__global__ void __launch_bounds__(BLK_THREADS) row_head_kernel(RowHeadArgs a) {
    typedef typename Elem<DT>::type elem_t;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c0 = lane * E;
    float w[BLK_VMAX][E];
    HY_UNROLL
    for (int v = 0; v < BLK_VMAX; ++v) {
        if (v < a.V) {
            blk_load<DT, E>(a.w, (size_t)v * a.D + c0, w[v]);
        } else {
            HY_UNROLL
            for (int e = 0; e < E; ++e) w[v][e] = 0.f;
        }
    }
    for (long row = (long)blockIdx.x * BLK_WAVES + wave; row < a.rows; row += (long)gridDim.x * BLK_WAVES) {
        if (!BWD) {
            float x[E];
            blk_load<DT, E>(a.x, (size_t)row * a.D + c0, x);
            float mine = 0.f;                                // lane v keeps logit v
            HY_UNROLL
            for (int v = 0; v < BLK_VMAX; ++v) {
                if (v < a.V) {                               // wave-uniform
                    float s = 0.f;
                    HY_UNROLL
                    for (int e = 0; e < E; ++e) s += x[e] * w[v][e];
                    s = wave_sum(s);
                    mine = lane == v ? s : mine;
                }
            }
            if (lane < a.V) reinterpret_cast<elem_t*>(a.out)[(size_t)row * a.V + lane] = Elem<DT>::cvt(mine);
        } else {
            float dx[E];
            HY_UNROLL
            for (int e = 0; e < E; ++e) dx[e] = 0.f;
            HY_UNROLL
            for (int v = 0; v < BLK_VMAX; ++v) {
                if (v < a.V) {
                    const float g = Elem<DT>::dec(reinterpret_cast<const elem_t*>(a.x)[(size_t)row * a.V + v]);
                    HY_UNROLL
                    for (int e = 0; e < E; ++e) dx[e] += g * w[v][e];
                }
            }
            blk_store<DT, E>(a.out, (size_t)row * a.D + c0, dx);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// The pooled readout of a sequence classifier (src/tasks/decoders.py SequenceDecoder, mode pool / sum, on top of the backbone's
// final norm, long_conv_lm.py:381-396):
//     pooled[b, :] = scale_b * sum_{t < n_b} LayerNorm(dropout(x0[b, t]) + residual[b, t])        scale_b = 1 / n_b (mean) or 1 (sum)
// inside the add + LayerNorm pass: neither the normalised (B, L, D) tensor nor residual' is written, and the backward needs no
// (B, L, D) dout -- every row's dout is the one vector scale_b * g[b], held in registers.  Same arithmetic and layout as
// add_norm_fwd_kernel (a wavefront owns a row, lane l the E channels from l E on).  The grid is (row chunks, B) and depends on
// (B, L) only: n_b is read from device memory (`lengths`, int32, clamped to [0, L]; null: L), so one captured graph serves every
// batch.  Sums are taken in a fixed order -- a wavefront over its rows, the 4 wavefronts through LDS, the chunks by
// add_norm_pool_finish_kernel -- no atomics: bit-reproducible.
// ---------------------------------------------------------------------------------------------------------------
enum { POOL_MEAN = 0, POOL_SUM = 1 };

struct AddNormPoolArgs {
    const void* x;          // (B, L, D) elements of XDT: x0
    const float* res_in;    // (B, L, D) fp32 or null: residual
    const float* weight;    // (D,)
    const float* bias;      // (D,)  fwd only
    const int* lengths;     // (B,) device int32 or null
    const float* g;         // bwd: (B, D) gradient of pooled
    float* pooled;          // fwd: (B, D)
    void* dx;               // bwd: (B, L, D) elements of XDT
    float* dres;            // bwd: (B, L, D) fp32 or null
    float* mean;            // (B L,)  fwd: out (rows t < n_b), bwd: in
    float* rstd;            // (B L,)
    float* part;            // fwd: [B][chunks][D]; bwd: [B * chunks][np][D] (dweight | dbias [| column sums of dx0 as stored])
    int np;
    int mode;               // POOL_MEAN / POOL_SUM
    long L;
    int D;
    int chunk_rows;         // rows of a chunk: a multiple of BLK_WAVES
    float eps;
    const unsigned long long* seed;
    unsigned drop_below;
    float keep_scale;
};

__device__ __forceinline__ long pool_len(const AddNormPoolArgs& a, int b) {
    if (a.lengths == nullptr) return a.L;
    const long n = a.lengths[b];
    return n < 0 ? 0 : (n > a.L ? a.L : n);
}

// residual' of one row in registers: dropout(x0) + residual, as add_norm_fwd_kernel forms it
template <int XDT, int E>
__device__ __forceinline__ void pool_row(const AddNormPoolArgs& a, size_t off, unsigned long long seed, float (&r)[E]) {
    blk_load<XDT, E>(a.x, off, r);
    if (a.seed != nullptr) blk_dropout<E>(r, off, seed, a.drop_below, a.keep_scale);
    if (a.res_in != nullptr) {
        float q[E];
        blk_load<DT_F32, E>(a.res_in, off, q);
        HY_UNROLL
        for (int e = 0; e < E; ++e) r[e] += q[e];
    }
}

template <int XDT, int E>
__global__ void __launch_bounds__(BLK_THREADS) add_norm_pool_fwd_kernel(AddNormPoolArgs a) {
    HY_SMEM(smem);
    HY_LDS float* red = HY_LDS_CAST(float, smem);            // [BLK_WAVES][64 * E]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c0 = lane * E, D = 64 * E;
    const int b = blockIdx.y;
    const long n = pool_len(a, b);
    const long t0 = (long)blockIdx.x * a.chunk_rows;
    if (t0 >= n) return;                                     // a chunk of pad rows only: nothing is read, the finish kernel does not look at its slot
    const long t1 = t0 + a.chunk_rows < n ? t0 + a.chunk_rows : n;
    float w[E], bs[E], acc[E];
    HY_UNROLL
    for (int e = 0; e < E; ++e) { w[e] = a.weight[c0 + e]; bs[e] = a.bias[c0 + e]; acc[e] = 0.f; }
    const float inv_d = 1.f / (float)D;
    const unsigned long long seed = a.seed != nullptr ? *a.seed : 0ull;
    for (long t = t0 + wave; t < t1; t += BLK_WAVES) {
        const long row = (long)b * a.L + t;
        float r[E];
        pool_row<XDT, E>(a, (size_t)row * D + c0, seed, r);
        float s = 0.f;
        HY_UNROLL
        for (int e = 0; e < E; ++e) s += r[e];
        const float mean = wave_sum(s) * inv_d;
        float v = 0.f;
        HY_UNROLL
        for (int e = 0; e < E; ++e) v += (r[e] - mean) * (r[e] - mean);
        const float rstd = 1.f / sqrtf(wave_sum(v) * inv_d + a.eps);
        HY_UNROLL
        for (int e = 0; e < E; ++e) acc[e] += (r[e] - mean) * rstd * w[e] + bs[e];     // fp32, never rounded to the I/O type
        if (lane == 0) { a.mean[row] = mean; a.rstd[row] = rstd; }
    }
    HY_UNROLL
    for (int e = 0; e < E; ++e) red[wave * D + c0 + e] = acc[e];
    __syncthreads();
    for (int i = threadIdx.x; i < D; i += BLK_THREADS) {
        float s = 0.f;
        HY_UNROLL
        for (int q = 0; q < BLK_WAVES; ++q) s += red[q * D + i];                       // the 4 wavefronts, in order
        a.part[((size_t)b * gridDim.x + blockIdx.x) * D + i] = s;
    }
}

// pooled[b][j] = scale_b * sum over the chunks that hold rows < n_b, in index order: a workgroup owns 16 channels of one sequence, its 16
// thread rows sum interleaved slices of the chunks (independent loads in flight), thread row 0 adds the slices in order.  (A template only
// because this header is part of several translation units.)
template <int S = 16>
__global__ void __launch_bounds__(256) add_norm_pool_finish_kernel(AddNormPoolArgs a, int chunks) {
    HY_SMEM(smem);
    HY_LDS float* sm = HY_LDS_CAST(float, smem);             // [16][16]
    const int jj = threadIdx.x & 15, cs = threadIdx.x >> 4;
    const int b = blockIdx.y, D = a.D;
    const int j = blockIdx.x * 16 + jj;
    const int jc = j < D ? j : D - 1;
    const long n = pool_len(a, b);
    const int active = (int)((n + a.chunk_rows - 1) / a.chunk_rows);                   // <= chunks
    const float* part = a.part + (size_t)b * chunks * D;
    float s = 0.f;
    int c = cs;
    for (; c + 7 * 16 < active; c += 8 * 16) {
        float v[8];
        HY_UNROLL
        for (int u = 0; u < 8; ++u) v[u] = part[(size_t)(c + u * 16) * D + jc];
        HY_UNROLL
        for (int u = 0; u < 8; ++u) s += v[u];
    }
    for (; c < active; c += 16) s += part[(size_t)c * D + jc];
    sm[cs * 16 + jj] = s;
    __syncthreads();
    if (cs == 0 && j < D) {
        float r = 0.f;
        for (int q = 0; q < 16; ++q) r += sm[q * 16 + jj];
        if (a.mode == POOL_MEAN) r = n > 0 ? r / (float)n : 0.f;                       // n_b = 0: zeros, never NaN
        a.pooled[(size_t)b * D + j] = r;
    }
}

// The backward.  dout of every row t < n_b is gv = scale_b g[b]: with it s1 = mean(gv w) is one number per sequence, dweight = gv * (sum of
// the rows' xhat) and dbias = gv * (number of rows), so a row costs one butterfly (s2) instead of two.  residual' is rebuilt from x0 and
// residual (dropout regenerated from the seed); rows t >= n_b get zeros without a load.
template <int XDT, int E>
__global__ void __launch_bounds__(BLK_THREADS) add_norm_pool_bwd_kernel(AddNormPoolArgs a) {
    HY_SMEM(smem);
    HY_LDS float* red = HY_LDS_CAST(float, smem);            // [BLK_WAVES][np][64 * E]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c0 = lane * E, D = 64 * E, np = a.np;
    const int b = blockIdx.y;
    const long n = pool_len(a, b);
    const long t0 = (long)blockIdx.x * a.chunk_rows;
    const long t1 = t0 + a.chunk_rows < a.L ? t0 + a.chunk_rows : a.L;
    const float scale = a.mode == POOL_MEAN ? (n > 0 ? 1.f / (float)n : 0.f) : 1.f;
    const float inv_d = 1.f / (float)D;
    float gv[E], gw[E], sxh[E], dxs[E], zero[E];
    float s1 = 0.f, cnt = 0.f;
    HY_UNROLL
    for (int e = 0; e < E; ++e) {
        gv[e] = scale * a.g[(size_t)b * D + c0 + e];
        gw[e] = gv[e] * a.weight[c0 + e];
        s1 += gw[e];
        sxh[e] = 0.f; dxs[e] = 0.f; zero[e] = 0.f;
    }
    s1 = wave_sum(s1) * inv_d;
    const unsigned long long seed = a.seed != nullptr ? *a.seed : 0ull;
    for (long t = t0 + wave; t < t1; t += BLK_WAVES) {
        const long row = (long)b * a.L + t;
        const size_t off = (size_t)row * D + c0;
        if (t >= n) {                                        // a pad row (wave-uniform): its gradients are zero
            blk_store<XDT, E>(a.dx, off, zero);
            if (a.dres != nullptr) blk_store<DT_F32, E>(a.dres, off, zero);
            continue;
        }
        float r[E];
        pool_row<XDT, E>(a, off, seed, r);
        const float mean = a.mean[row], rstd = a.rstd[row];
        float s2 = 0.f, xh[E];
        HY_UNROLL
        for (int e = 0; e < E; ++e) {
            xh[e] = (r[e] - mean) * rstd;
            s2 += gw[e] * xh[e];
            sxh[e] += xh[e];
        }
        cnt += 1.f;
        s2 = wave_sum(s2) * inv_d;
        float dr[E];
        HY_UNROLL
        for (int e = 0; e < E; ++e) dr[e] = rstd * (gw[e] - s1 - xh[e] * s2);
        if (a.dres != nullptr) blk_store<DT_F32, E>(a.dres, off, dr);
        if (a.seed != nullptr) blk_dropout<E>(dr, off, seed, a.drop_below, a.keep_scale);      // d x0 = d residual' through the same mask
        blk_store<XDT, E>(a.dx, off, dr);
        if (np == 3) {
            HY_UNROLL
            for (int e = 0; e < E; ++e) dxs[e] += Elem<XDT>::dec(Elem<XDT>::cvt(dr[e]));
        }
    }
    HY_UNROLL
    for (int e = 0; e < E; ++e) {
        red[(wave * np + 0) * D + c0 + e] = gv[e] * sxh[e];
        red[(wave * np + 1) * D + c0 + e] = gv[e] * cnt;
        if (np == 3) red[(wave * np + 2) * D + c0 + e] = dxs[e];
    }
    __syncthreads();
    const size_t slot = (size_t)b * gridDim.x + blockIdx.x;
    for (int i = threadIdx.x; i < np * D; i += BLK_THREADS) {
        float s = 0.f;
        HY_UNROLL
        for (int q = 0; q < BLK_WAVES; ++q) s += red[q * np * D + i];
        a.part[slot * np * D + i] = s;
    }
}

}  // namespace hyena
