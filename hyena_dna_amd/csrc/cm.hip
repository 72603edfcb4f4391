// cm.hip -- host side of the channel-major operator shell (cm_kernels.h; C ABI in include/hyena_mixer.h) and of its one-position decode
// step (decode_kernels.h; C ABI in include/hyena_decode.h) and of the edited-window step (variant_kernels.h; C ABI in include/hyena_variant.h).
#include "cm_kernels.h"
#include "decode_kernels.h"
#include "variant_kernels.h"
#include "launch.h"
#include "../../include/hyena_fftconv.h"
#include "../../include/hyena_mixer.h"
#include "../../include/hyena_decode.h"
#include "../../include/hyena_variant.h"

using namespace hyena;

namespace {
// a (C, B, len) layout: row (c, b) at c cs + b bs; rows must not overlap
bool cm_layout_ok(long cs, int bs, int B, int len) { return bs >= len && cs >= (long)(B - 1) * bs + len; }
// zT / dzT of the post kernels may also be BATCH-major rows -- row (d, b) at d cs + b bs with bs >= (D - 1) cs + len: the (B, D, len) layout the
// convolution takes, cs = its row pitch, bs = D cs -- so that the gate between two long convolutions (HyenaOperator at order >= 3, hyena.py:414-423)
// writes the next convolution's input, and reads its gradient, in place (round 6)
bool cm_zlayout_ok(long cs, int bs, int B, int D, int len) {
    return cm_layout_ok(cs, bs, B, len) || (cs >= len && (long)bs >= (long)(D - 1) * cs + len);
}
bool cm_ok(const void* xT, const float* w, const float* b, int B, int L, int Lx, int D, long csx, int bsx, int lda, int dtype) {
    return xT != nullptr && w != nullptr && b != nullptr && B >= 1 && L >= 1 && Lx >= L && D >= 1 && cm_layout_ok(csx, bsx, B, Lx) && lda >= L &&
           (dtype == HYENA_F32 || dtype == HYENA_BF16 || dtype == HYENA_F16);
}
int cm_tiles(int L) { return (L + CM_TILE - 1) / CM_TILE; }
// (channel, batch) rows per workgroup: sequences that leave at least half of a 2048-position tile empty share it, 2 / 4 / 8 batch items of one channel
int cm_rpw(int B, int L) {
    int r = 1;
    while (r < 8 && L * 2 * r <= CM_TILE && r * 2 <= B) r *= 2;
    return r;
}
dim3 cm_grid(int B, int L, int D) { const int r = cm_rpw(B, L); return dim3(cm_tiles(L), D, (B + r - 1) / r); }
const size_t CM_SMEM = 2 * 5 * 4 * sizeof(float);

#define HY_CM_DISPATCH(kernel, smem)                                                                                      \
    do {                                                                                                                  \
        switch (dtype) {                                                                                                  \
            case HYENA_F32: HY_LAUNCH((kernel<DT_F32>), cm_grid(B, L, D), dim3(CM_THREADS), smem, stream, a); break;      \
            case HYENA_BF16: HY_LAUNCH((kernel<DT_BF16>), cm_grid(B, L, D), dim3(CM_THREADS), smem, stream, a); break;    \
            default: HY_LAUNCH((kernel<DT_F16>), cm_grid(B, L, D), dim3(CM_THREADS), smem, stream, a); break;             \
        }                                                                                                                 \
    } while (0)
}  // namespace

extern "C" {

size_t hyena_cm_partial_floats(int B, int L, int D) {
    if (B < 1 || L < 1 || D < 1) return 0;
    const int r = cm_rpw(B, L);
    return (size_t)3 * D * ((B + r - 1) / r) * cm_tiles(L) * CM_NP;
}

int hyena_cm_pre_fwd_ld(const void* xT, const float* bin, const float* w, const float* b, void* vg, int B, int L, int Lx, int D, long csx,
                        int bsx, int lda, int dtype, void* stream) {
    const long csz = 0; const int bsz = 0;
    if (!cm_ok(xT, w, b, B, L, Lx, D, csx, bsx, lda, dtype) || vg == nullptr) return HYENA_ERR_BAD_ARG;
    CmArgs a;
    a.xT = xT; a.bin = bin; a.w = w; a.b = b; a.a0 = nullptr; a.a1 = nullptr; a.o0 = vg; a.dxT = nullptr; a.part = nullptr;
    a.B = B; a.L = L; a.D = D; a.Lx = Lx; a.csx = csx; a.bsx = bsx; a.csz = csz; a.bsz = bsz; a.lda = lda; a.rpw = cm_rpw(B, L);
    HY_CM_DISPATCH(cm_pre_fwd_kernel, 0);
    return hy_launch_error() ? HYENA_ERR_LAUNCH : HYENA_OK;
}

int hyena_cm_post_fwd_ld(const void* y, const void* xT, const float* bin, const float* w, const float* b, void* zT, int B, int L, int Lx,
                         int D, long csx, int bsx, long csz, int bsz, int lda, int dtype, void* stream) {
    if (!cm_ok(xT, w, b, B, L, Lx, D, csx, bsx, lda, dtype) || y == nullptr || zT == nullptr || !cm_zlayout_ok(csz, bsz, B, D, L)) return HYENA_ERR_BAD_ARG;
    CmArgs a;
    a.xT = xT; a.bin = bin; a.w = w; a.b = b; a.a0 = y; a.a1 = nullptr; a.o0 = zT; a.dxT = nullptr; a.part = nullptr;
    a.B = B; a.L = L; a.D = D; a.Lx = Lx; a.csx = csx; a.bsx = bsx; a.csz = csz; a.bsz = bsz; a.lda = lda; a.rpw = cm_rpw(B, L);
    HY_CM_DISPATCH(cm_post_fwd_kernel, 0);
    return hy_launch_error() ? HYENA_ERR_LAUNCH : HYENA_OK;
}

int hyena_cm_post_bwd_ld(const void* dzT, const void* y, const void* xT, const float* bin, const float* w, const float* b, void* dy,
                         void* dxT, float* part, int B, int L, int Lx, int D, long csx, int bsx, long csz, int bsz, int lda, int dtype,
                         void* stream) {
    if (!cm_ok(xT, w, b, B, L, Lx, D, csx, bsx, lda, dtype) || !cm_zlayout_ok(csz, bsz, B, D, L) || dzT == nullptr || y == nullptr || dy == nullptr || dxT == nullptr || part == nullptr)
        return HYENA_ERR_BAD_ARG;
    CmArgs a;
    a.xT = xT; a.bin = bin; a.w = w; a.b = b; a.a0 = y; a.a1 = dzT; a.o0 = dy; a.dxT = dxT; a.part = part;
    a.B = B; a.L = L; a.D = D; a.Lx = Lx; a.csx = csx; a.bsx = bsx; a.csz = csz; a.bsz = bsz; a.lda = lda; a.rpw = cm_rpw(B, L);
    HY_CM_DISPATCH(cm_post_bwd_kernel, CM_SMEM);
    return hy_launch_error() ? HYENA_ERR_LAUNCH : HYENA_OK;
}

int hyena_cm_pre_bwd_ld(const void* dvg, const void* xT, const float* bin, const float* w, const float* b, void* dxT, float* part, int B,
                        int L, int Lx, int D, long csx, int bsx, int lda, int dtype, void* stream) {
    const long csz = 0; const int bsz = 0;
    if (!cm_ok(xT, w, b, B, L, Lx, D, csx, bsx, lda, dtype) || dvg == nullptr || dxT == nullptr || part == nullptr) return HYENA_ERR_BAD_ARG;
    CmArgs a;
    a.xT = xT; a.bin = bin; a.w = w; a.b = b; a.a0 = dvg; a.a1 = nullptr; a.o0 = nullptr; a.dxT = dxT; a.part = part;
    a.B = B; a.L = L; a.D = D; a.Lx = Lx; a.csx = csx; a.bsx = bsx; a.csz = csz; a.bsz = bsz; a.lda = lda; a.rpw = cm_rpw(B, L);
    HY_CM_DISPATCH(cm_pre_bwd_kernel, CM_SMEM);
    return hy_launch_error() ? HYENA_ERR_LAUNCH : HYENA_OK;
}

// the packed layouts: ldx = Lx, lda = L
int hyena_cm_pre_fwd(const void* xT, const float* bin, const float* w, const float* b, void* vg, int B, int L, int Lx, int D, int dtype,
                     void* stream) {
    return hyena_cm_pre_fwd_ld(xT, bin, w, b, vg, B, L, Lx, D, (long)B * Lx, Lx, L, dtype, stream);
}
int hyena_cm_post_fwd(const void* y, const void* xT, const float* bin, const float* w, const float* b, void* zT, int B, int L, int Lx,
                      int D, int dtype, void* stream) {
    return hyena_cm_post_fwd_ld(y, xT, bin, w, b, zT, B, L, Lx, D, (long)B * Lx, Lx, (long)B * L, L, L, dtype, stream);
}
int hyena_cm_post_bwd(const void* dzT, const void* y, const void* xT, const float* bin, const float* w, const float* b, void* dy,
                      void* dxT, float* part, int B, int L, int Lx, int D, int dtype, void* stream) {
    return hyena_cm_post_bwd_ld(dzT, y, xT, bin, w, b, dy, dxT, part, B, L, Lx, D, (long)B * Lx, Lx, (long)B * L, L, L, dtype, stream);
}
int hyena_cm_pre_bwd(const void* dvg, const void* xT, const float* bin, const float* w, const float* b, void* dxT, float* part, int B,
                     int L, int Lx, int D, int dtype, void* stream) {
    return hyena_cm_pre_bwd_ld(dvg, xT, bin, w, b, dxT, part, B, L, Lx, D, (long)B * Lx, Lx, L, dtype, stream);
}

}  // extern "C"

// ---- the one-position decode step (decode_kernels.h) ----------------------------------------------------------------------------------
namespace {
const int DEC_MAX_L = 1 << 20;
bool dec_dtype_ok(int dtype) { return dtype == HYENA_F32 || dtype == HYENA_BF16 || dtype == HYENA_F16; }
bool dec_aligned16(const void* p) { return (reinterpret_cast<size_t>(p) & 15) == 0; }
// the history rows: lda >= Lcap, 8-element multiple (every 8-element vector of a row is one aligned 16 / 32-byte access and never crosses its end)
bool dec_hist_ok(const void* vg, int B, int D, int Lcap, int lda, int dtype) {
    return vg != nullptr && dec_aligned16(vg) && B >= 1 && D >= 1 && Lcap >= 1 && Lcap <= DEC_MAX_L && lda >= Lcap && lda % DEC_V == 0 &&
           dec_dtype_ok(dtype);
}
int dec_chunks(int Lcap) { return (Lcap + DEC_CHUNK - 1) / DEC_CHUNK; }
DecArgs dec_args() {
    DecArgs a;
    a.x = nullptr; a.bin = nullptr; a.w = nullptr; a.b = nullptr; a.tail = nullptr; a.vg = nullptr; a.x0 = nullptr; a.k = nullptr;
    a.part = nullptr; a.fb = nullptr; a.z = nullptr; a.pos = nullptr;
    a.B = a.D = a.Bcap = a.Lcap = a.ldx = a.lda = a.ldk = 0;
    return a;
}
// S: a whole number of chunks inside the cache; the row history holds columns [S, Lcap) in rows of ldr elements; the shared one [0, S)
bool dec_fan_ok(bool shared, const void* vgs, const void* vgr, int B, int fan, int D, int Lcap, int S, int lds, int ldr, int dtype) {
    if (vgr == nullptr || !dec_aligned16(vgr) || B < 1 || fan < 1 || B % fan != 0 || D < 1 || Lcap < 1 || Lcap > DEC_MAX_L || !dec_dtype_ok(dtype))
        return false;
    if (S < 0 || S % DEC_CHUNK != 0 || S > Lcap || ldr < 1 || ldr < Lcap - S || ldr % DEC_V != 0) return false;
    return !shared || S == 0 || (vgs != nullptr && dec_aligned16(vgs) && lds >= S && lds % DEC_V == 0);   // (only decode_conv_fan reads it)
}
DecFanArgs dec_fan_args(const void* vgs, int fan, int S, int lds) {
    DecFanArgs a;
    static_cast<DecArgs&>(a) = dec_args();
    a.vgs = vgs; a.fan = fan; a.S = S; a.lds = lds;
    return a;
}
bool dec_block_T_ok(int T) { return T >= 1 && T <= DEC_TMAX; }
DecBlockArgs dec_block_args(const void* vgs, int fan, int S, int lds, int T) {
    DecBlockArgs a;
    static_cast<DecFanArgs&>(a) = dec_fan_args(vgs, fan, S, lds);
    a.T = T;
    return a;
}
static_assert(DEC_TMAX == HYENA_DECODE_TMAX, "the header's block limit");
#define HY_DEC_DISPATCH(kernel, grid, threads, smem)                                                                 \
    do {                                                                                                              \
        switch (dtype) {                                                                                              \
            case HYENA_F32: HY_LAUNCH((kernel<DT_F32>), grid, dim3(threads), smem, stream, a); break;                 \
            case HYENA_BF16: HY_LAUNCH((kernel<DT_BF16>), grid, dim3(threads), smem, stream, a); break;               \
            default: HY_LAUNCH((kernel<DT_F16>), grid, dim3(threads), smem, stream, a); break;                        \
        }                                                                                                             \
    } while (0)
// the automaton instantiation of a kernel template <DT, AUTO, Args> (decode_sample_con_kernel, decode_beam_kernel)
#define HY_DEC_DISPATCH_AUTO(kernel, Args, grid, threads, smem)                                                      \
    do {                                                                                                              \
        switch (dtype) {                                                                                              \
            case HYENA_F32: HY_LAUNCH((kernel<DT_F32, true, Args>), grid, dim3(threads), smem, stream, a); break;     \
            case HYENA_BF16: HY_LAUNCH((kernel<DT_BF16, true, Args>), grid, dim3(threads), smem, stream, a); break;   \
            default: HY_LAUNCH((kernel<DT_F16, true, Args>), grid, dim3(threads), smem, stream, a); break;            \
        }                                                                                                             \
    } while (0)
}  // namespace

extern "C" {

size_t hyena_decode_partial_floats(int B, int D, int Lcap) {
    if (B < 1 || D < 1 || Lcap < 1 || Lcap > DEC_MAX_L) return 0;
    return (size_t)dec_chunks(Lcap) * B * D;
}

int hyena_decode_pre(const void* x, int ldx, const float* bin, const float* w, const float* b, float* tail, void* vg, float* x0, const int* pos,
                     int B, int Bcap, int D, int Lcap, int lda, int dtype, void* stream) {
    if (x == nullptr || w == nullptr || b == nullptr || tail == nullptr || x0 == nullptr || pos == nullptr || !dec_hist_ok(vg, B, D, Lcap, lda, dtype) ||
        Bcap < B || ldx < 3 * D || (long)Bcap * D > (1L << 30))
        return HYENA_ERR_BAD_ARG;
    DecArgs a = dec_args();
    a.x = x; a.bin = bin; a.w = w; a.b = b; a.tail = tail; a.vg = vg; a.x0 = x0; a.pos = const_cast<int*>(pos);
    a.B = B; a.D = D; a.Bcap = Bcap; a.Lcap = Lcap; a.ldx = ldx; a.lda = lda;
    HY_DEC_DISPATCH(decode_pre_kernel, dim3((B * D + DEC_THREADS - 1) / DEC_THREADS), DEC_THREADS, 0);
    return hy_launch_error() ? HYENA_ERR_LAUNCH : HYENA_OK;
}

int hyena_decode_conv(const float* k, int ldk, const void* vg, float* part, const int* pos, int B, int D, int Lcap, int lda, int dtype,
                      void* stream) {
    if (k == nullptr || !dec_aligned16(k) || ldk < Lcap || ldk % 4 != 0 || part == nullptr || pos == nullptr ||
        !dec_hist_ok(vg, B, D, Lcap, lda, dtype) || D > 65535)
        return HYENA_ERR_BAD_ARG;
    DecArgs a = dec_args();
    a.k = k; a.vg = const_cast<void*>(vg); a.part = part; a.pos = const_cast<int*>(pos);
    a.B = B; a.D = D; a.Lcap = Lcap; a.lda = lda; a.ldk = ldk;
    HY_DEC_DISPATCH(decode_conv_kernel, dim3(dec_chunks(Lcap), D), DEC_THREADS, (DEC_KLDS + 8) * sizeof(float));
    return hy_launch_error() ? HYENA_ERR_LAUNCH : HYENA_OK;
}

int hyena_decode_post(const float* part, const void* vg, const float* fb, const float* x0, void* z, int* pos, int B, int D, int Lcap, int lda,
                      int dtype, void* stream) {
    if (part == nullptr || x0 == nullptr || z == nullptr || pos == nullptr || !dec_hist_ok(vg, B, D, Lcap, lda, dtype) || (long)B * D > (1L << 30))
        return HYENA_ERR_BAD_ARG;
    DecArgs a = dec_args();
    a.part = const_cast<float*>(part); a.vg = const_cast<void*>(vg); a.fb = fb; a.x0 = const_cast<float*>(x0); a.z = z; a.pos = pos;
    a.B = B; a.D = D; a.Lcap = Lcap; a.lda = lda;
    HY_DEC_DISPATCH(decode_post_kernel, dim3(1), DEC_POST_THREADS, 0);
    return hy_launch_error() ? HYENA_ERR_LAUNCH : HYENA_OK;
}

// ---- per-row positions: pos points at B ints, row b stands at pos[b] (same argument checks, same grids) ----------------------------------
int hyena_decode_pre_rows(const void* x, int ldx, const float* bin, const float* w, const float* b, float* tail, void* vg, float* x0,
                          const int* pos, int B, int Bcap, int D, int Lcap, int lda, int dtype, void* stream) {
    if (x == nullptr || w == nullptr || b == nullptr || tail == nullptr || x0 == nullptr || pos == nullptr || !dec_hist_ok(vg, B, D, Lcap, lda, dtype) ||
        Bcap < B || ldx < 3 * D || (long)Bcap * D > (1L << 30))
        return HYENA_ERR_BAD_ARG;
    DecArgs a = dec_args();
    a.x = x; a.bin = bin; a.w = w; a.b = b; a.tail = tail; a.vg = vg; a.x0 = x0; a.pos = const_cast<int*>(pos);
    a.B = B; a.D = D; a.Bcap = Bcap; a.Lcap = Lcap; a.ldx = ldx; a.lda = lda;
    HY_DEC_DISPATCH(decode_pre_rows_kernel, dim3((B * D + DEC_THREADS - 1) / DEC_THREADS), DEC_THREADS, 0);
    return hy_launch_error() ? HYENA_ERR_LAUNCH : HYENA_OK;
}

int hyena_decode_conv_rows(const float* k, int ldk, const void* vg, float* part, const int* pos, int B, int D, int Lcap, int lda, int dtype,
                           void* stream) {
    if (k == nullptr || !dec_aligned16(k) || ldk < Lcap || ldk % 4 != 0 || part == nullptr || pos == nullptr ||
        !dec_hist_ok(vg, B, D, Lcap, lda, dtype) || D > 65535)
        return HYENA_ERR_BAD_ARG;
    DecArgs a = dec_args();
    a.k = k; a.vg = const_cast<void*>(vg); a.part = part; a.pos = const_cast<int*>(pos);
    a.B = B; a.D = D; a.Lcap = Lcap; a.lda = lda; a.ldk = ldk;
    HY_DEC_DISPATCH(decode_conv_rows_kernel, dim3(dec_chunks(Lcap), D), DEC_THREADS, (DEC_KLDS + 8) * sizeof(float));
    return hy_launch_error() ? HYENA_ERR_LAUNCH : HYENA_OK;
}

int hyena_decode_post_rows(const float* part, const void* vg, const float* fb, const float* x0, void* z, int* pos, int B, int D, int Lcap,
                           int lda, int dtype, void* stream) {
    if (part == nullptr || x0 == nullptr || z == nullptr || pos == nullptr || !dec_hist_ok(vg, B, D, Lcap, lda, dtype) || (long)B * D > (1L << 30))
        return HYENA_ERR_BAD_ARG;
    DecArgs a = dec_args();
    a.part = const_cast<float*>(part); a.vg = const_cast<void*>(vg); a.fb = fb; a.x0 = const_cast<float*>(x0); a.z = z; a.pos = pos;
    a.B = B; a.D = D; a.Lcap = Lcap; a.lda = lda;
    HY_DEC_DISPATCH(decode_post_rows_kernel, dim3(1), DEC_POST_THREADS, 0);
    return hy_launch_error() ? HYENA_ERR_LAUNCH : HYENA_OK;
}

// ---- fan-out: B = G fan rows, columns [0, S) of a group's history shared, [S, Lcap) per row (same grids) ---------------------------------
int hyena_decode_pre_fan(const void* x, int ldx, const float* bin, const float* w, const float* b, float* tail, void* vgr, float* x0,
                         const int* pos, int B, int Bcap, int D, int Lcap, int S, int ldr, int dtype, void* stream) {
    if (x == nullptr || w == nullptr || b == nullptr || tail == nullptr || x0 == nullptr || pos == nullptr ||
        !dec_fan_ok(false, nullptr, vgr, B, 1, D, Lcap, S, 0, ldr, dtype) || Bcap < B || ldx < 3 * D || (long)Bcap * D > (1L << 30))
        return HYENA_ERR_BAD_ARG;
    DecFanArgs a = dec_fan_args(nullptr, 1, S, 0);
    a.x = x; a.bin = bin; a.w = w; a.b = b; a.tail = tail; a.vg = vgr; a.x0 = x0; a.pos = const_cast<int*>(pos);
    a.B = B; a.D = D; a.Bcap = Bcap; a.Lcap = Lcap; a.ldx = ldx; a.lda = ldr;
    HY_DEC_DISPATCH(decode_pre_fan_kernel, dim3((B * D + DEC_THREADS - 1) / DEC_THREADS), DEC_THREADS, 0);
    return hy_launch_error() ? HYENA_ERR_LAUNCH : HYENA_OK;
}

int hyena_decode_conv_fan(const float* k, int ldk, const void* vgs, const void* vgr, float* part, const int* pos, int B, int fan, int D,
                          int Lcap, int S, int lds, int ldr, int dtype, void* stream) {
    if (k == nullptr || !dec_aligned16(k) || ldk < Lcap || ldk % 4 != 0 || part == nullptr || pos == nullptr ||
        !dec_fan_ok(true, vgs, vgr, B, fan, D, Lcap, S, lds, ldr, dtype) || D > 65535)
        return HYENA_ERR_BAD_ARG;
    DecFanArgs a = dec_fan_args(vgs, fan, S, lds);
    a.k = k; a.vg = const_cast<void*>(vgr); a.part = part; a.pos = const_cast<int*>(pos);
    a.B = B; a.D = D; a.Lcap = Lcap; a.lda = ldr; a.ldk = ldk;
    HY_DEC_DISPATCH(decode_conv_fan_kernel, dim3(dec_chunks(Lcap), D), DEC_THREADS, (DEC_KLDS + 8) * sizeof(float));
    return hy_launch_error() ? HYENA_ERR_LAUNCH : HYENA_OK;
}

int hyena_decode_post_fan(const float* part, const void* vgr, const float* fb, const float* x0, void* z, int* pos, int B, int fan, int D,
                          int Lcap, int S, int ldr, int dtype, void* stream) {
    if (part == nullptr || x0 == nullptr || z == nullptr || pos == nullptr || !dec_fan_ok(false, nullptr, vgr, B, fan, D, Lcap, S, 0, ldr, dtype) ||
        (long)B * D > (1L << 30))
        return HYENA_ERR_BAD_ARG;
    DecFanArgs a = dec_fan_args(nullptr, fan, S, 0);
    a.part = const_cast<float*>(part); a.vg = const_cast<void*>(vgr); a.fb = fb; a.x0 = const_cast<float*>(x0); a.z = z; a.pos = pos;
    a.B = B; a.D = D; a.Lcap = Lcap; a.lda = ldr;
    HY_DEC_DISPATCH(decode_post_fan_kernel, dim3(1), DEC_POST_THREADS, 0);
    return hy_launch_error() ? HYENA_ERR_LAUNCH : HYENA_OK;
}

// ---- block step: T positions per call (decode_*_block_kernel; one set of kernels, the plain layout is S = 0, fan = 1) -----------------------
size_t hyena_decode_block_partial_floats(int B, int D, int Lcap, int T) {
    if (B < 1 || D < 1 || Lcap < 1 || Lcap > DEC_MAX_L || !dec_block_T_ok(T)) return 0;
    return (size_t)dec_chunks(Lcap) * B * T * D;
}

int hyena_decode_pre_block_fan(const void* x, int ldx, const float* bin, const float* w, const float* b, float* tail, void* vgr, float* x0,
                               const int* pos, int B, int Bcap, int D, int Lcap, int S, int ldr, int T, int dtype, void* stream) {
    if (!dec_block_T_ok(T) || x == nullptr || w == nullptr || b == nullptr || tail == nullptr || x0 == nullptr || pos == nullptr ||
        !dec_fan_ok(false, nullptr, vgr, B, 1, D, Lcap, S, 0, ldr, dtype) || Bcap < B || ldx < 3 * D || (long)Bcap * D > (1L << 30))
        return HYENA_ERR_BAD_ARG;
    DecBlockArgs a = dec_block_args(nullptr, 1, S, 0, T);
    a.x = x; a.bin = bin; a.w = w; a.b = b; a.tail = tail; a.vg = vgr; a.x0 = x0; a.pos = const_cast<int*>(pos);
    a.B = B; a.D = D; a.Bcap = Bcap; a.Lcap = Lcap; a.ldx = ldx; a.lda = ldr;
    HY_DEC_DISPATCH(decode_pre_block_kernel, dim3((B * D + DEC_THREADS - 1) / DEC_THREADS), DEC_THREADS, 0);
    return hy_launch_error() ? HYENA_ERR_LAUNCH : HYENA_OK;
}

int hyena_decode_conv_block_fan(const float* k, int ldk, const void* vgs, const void* vgr, float* part, const int* pos, int B, int fan, int D,
                                int Lcap, int S, int lds, int ldr, int T, int dtype, void* stream) {
    if (!dec_block_T_ok(T) || k == nullptr || !dec_aligned16(k) || ldk < Lcap || ldk % 4 != 0 || part == nullptr || pos == nullptr ||
        !dec_fan_ok(true, vgs, vgr, B, fan, D, Lcap, S, lds, ldr, dtype) || D > 65535)
        return HYENA_ERR_BAD_ARG;
    DecBlockArgs a = dec_block_args(vgs, fan, S, lds, T);
    a.k = k; a.vg = const_cast<void*>(vgr); a.part = part; a.pos = const_cast<int*>(pos);
    a.B = B; a.D = D; a.Lcap = Lcap; a.lda = ldr; a.ldk = ldk;
    HY_DEC_DISPATCH(decode_conv_block_kernel, dim3(dec_chunks(Lcap), D), DEC_THREADS, (DEC_KLDS_BLOCK + DEC_RED_BLOCK) * sizeof(float));
    return hy_launch_error() ? HYENA_ERR_LAUNCH : HYENA_OK;
}

int hyena_decode_post_block_fan(const float* part, const void* vgr, const float* fb, const float* x0, void* z, int* pos, int B, int fan, int D,
                                int Lcap, int S, int ldr, int T, int dtype, void* stream) {
    if (!dec_block_T_ok(T) || part == nullptr || x0 == nullptr || z == nullptr || pos == nullptr ||
        !dec_fan_ok(false, nullptr, vgr, B, fan, D, Lcap, S, 0, ldr, dtype) || (long)B * D > (1L << 30) / DEC_TMAX)
        return HYENA_ERR_BAD_ARG;
    DecBlockArgs a = dec_block_args(nullptr, fan, S, 0, T);
    a.part = const_cast<float*>(part); a.vg = const_cast<void*>(vgr); a.fb = fb; a.x0 = const_cast<float*>(x0); a.z = z; a.pos = pos;
    a.B = B; a.D = D; a.Lcap = Lcap; a.lda = ldr;
    HY_DEC_DISPATCH(decode_post_block_kernel, dim3((unsigned)(((size_t)B * T * D + DEC_THREADS - 1) / DEC_THREADS)), DEC_THREADS, 0);
    if (hy_launch_error()) return HYENA_ERR_LAUNCH;
    HY_LAUNCH(decode_advance_block_kernel, dim3(1), dim3(64), 0, stream, pos, T, S, Lcap);   // after every read of the position
    return hy_launch_error() ? HYENA_ERR_LAUNCH : HYENA_OK;
}

// the plain cache: nothing shared (S = 0, fan = 1), the history (Bcap, D, lda) with lda >= Lcap
int hyena_decode_pre_block(const void* x, int ldx, const float* bin, const float* w, const float* b, float* tail, void* vg, float* x0,
                           const int* pos, int B, int Bcap, int D, int Lcap, int lda, int T, int dtype, void* stream) {
    if (!dec_hist_ok(vg, B, D, Lcap, lda, dtype)) return HYENA_ERR_BAD_ARG;
    return hyena_decode_pre_block_fan(x, ldx, bin, w, b, tail, vg, x0, pos, B, Bcap, D, Lcap, 0, lda, T, dtype, stream);
}

int hyena_decode_conv_block(const float* k, int ldk, const void* vg, float* part, const int* pos, int B, int D, int Lcap, int lda, int T,
                            int dtype, void* stream) {
    if (!dec_hist_ok(vg, B, D, Lcap, lda, dtype)) return HYENA_ERR_BAD_ARG;
    return hyena_decode_conv_block_fan(k, ldk, nullptr, vg, part, pos, B, 1, D, Lcap, 0, 0, lda, T, dtype, stream);
}

int hyena_decode_post_block(const float* part, const void* vg, const float* fb, const float* x0, void* z, int* pos, int B, int D, int Lcap,
                            int lda, int T, int dtype, void* stream) {
    if (!dec_hist_ok(vg, B, D, Lcap, lda, dtype)) return HYENA_ERR_BAD_ARG;
    return hyena_decode_post_block_fan(part, vg, fb, x0, z, pos, B, 1, D, Lcap, 0, lda, T, dtype, stream);
}

// ---- lookahead carry (decode_carry_kernel, decode_conv_la_kernel, decode_post_la_kernel): the plain cache only -------------------------------
size_t hyena_decode_carry_partial_floats(int B, int D, int Lcap, int W) {
    if (B < 1 || D < 1 || Lcap < 1 || Lcap > DEC_MAX_L || !dec_block_T_ok(W)) return 0;
    return (size_t)dec_chunks(Lcap) * B * W * D;
}

int hyena_decode_carry(const float* k, int ldk, const void* vg, float* part, float* carry, const int* pos, int* base, int B, int D, int Lcap,
                       int lda, int W, int dtype, void* stream) {
    if (!dec_block_T_ok(W) || k == nullptr || !dec_aligned16(k) || ldk < Lcap || ldk % 4 != 0 || part == nullptr || carry == nullptr ||
        pos == nullptr || base == nullptr || !dec_hist_ok(vg, B, D, Lcap, lda, dtype) || D > 65535 || (long)B * D > (1L << 30) / DEC_TMAX)
        return HYENA_ERR_BAD_ARG;
    DecLaArgs a;
    static_cast<DecArgs&>(a) = dec_args();
    a.k = k; a.vg = const_cast<void*>(vg); a.part = part; a.carry = carry; a.pos = const_cast<int*>(pos); a.base = base; a.W = W;
    a.B = B; a.D = D; a.Lcap = Lcap; a.lda = lda; a.ldk = ldk;
    HY_DEC_DISPATCH(decode_carry_kernel, dim3(dec_chunks(Lcap), D), DEC_THREADS, (DEC_KLDS_BLOCK + DEC_RED_BLOCK) * sizeof(float));
    if (hy_launch_error()) return HYENA_ERR_LAUNCH;
    HY_LAUNCH(decode_carry_reduce_kernel, dim3((unsigned)(((size_t)B * W * D + DEC_THREADS - 1) / DEC_THREADS)), dim3(DEC_THREADS), 0, stream, a);
    if (hy_launch_error()) return HYENA_ERR_LAUNCH;
    HY_LAUNCH(decode_set_base_kernel, dim3(1), dim3(64), 0, stream, pos, base, Lcap);   // after every read of the position
    return hy_launch_error() ? HYENA_ERR_LAUNCH : HYENA_OK;
}

int hyena_decode_conv_la(const float* k, int ldk, const void* vg, float* part, const int* pos, const int* base, int B, int D, int Lcap, int lda,
                         int W, int dtype, void* stream) {
    if (!dec_block_T_ok(W) || k == nullptr || !dec_aligned16(k) || ldk < Lcap || ldk % 4 != 0 || part == nullptr || pos == nullptr ||
        base == nullptr || !dec_hist_ok(vg, B, D, Lcap, lda, dtype) || D > 65535)
        return HYENA_ERR_BAD_ARG;
    DecLaArgs a;
    static_cast<DecArgs&>(a) = dec_args();
    a.k = k; a.vg = const_cast<void*>(vg); a.part = part; a.carry = nullptr; a.pos = const_cast<int*>(pos); a.base = const_cast<int*>(base);
    a.W = W; a.B = B; a.D = D; a.Lcap = Lcap; a.lda = lda; a.ldk = ldk;
    HY_DEC_DISPATCH(decode_conv_la_kernel, dim3(2, D), DEC_THREADS, (DEC_KLDS_LA + 8) * sizeof(float));
    return hy_launch_error() ? HYENA_ERR_LAUNCH : HYENA_OK;
}

int hyena_decode_post_la(const float* part, const float* carry, const void* vg, const float* fb, const float* x0, void* z, int* pos,
                         const int* base, int B, int D, int Lcap, int lda, int W, int dtype, void* stream) {
    if (!dec_block_T_ok(W) || part == nullptr || carry == nullptr || x0 == nullptr || z == nullptr || pos == nullptr || base == nullptr ||
        !dec_hist_ok(vg, B, D, Lcap, lda, dtype) || (long)B * D > (1L << 30) / DEC_TMAX)
        return HYENA_ERR_BAD_ARG;
    DecLaArgs a;
    static_cast<DecArgs&>(a) = dec_args();
    a.part = const_cast<float*>(part); a.carry = const_cast<float*>(carry); a.vg = const_cast<void*>(vg); a.fb = fb;
    a.x0 = const_cast<float*>(x0); a.z = z; a.pos = pos; a.base = const_cast<int*>(base); a.W = W;
    a.B = B; a.D = D; a.Lcap = Lcap; a.lda = lda;
    HY_DEC_DISPATCH(decode_post_la_kernel, dim3(1), DEC_POST_THREADS, 0);
    return hy_launch_error() ? HYENA_ERR_LAUNCH : HYENA_OK;
}

// ---- token sampling (decode_sample_kernel): one wavefront per logit row -------------------------------------------------------------------
int hyena_decode_sample(const void* logits, long ldl, int dtype, int B, int V, int Vlive, float temperature, int top_k, float top_p,
                        const unsigned long long* seed, int eos, int pad, int* col, int* done, long long* seq, long lds, int ncols,
                        long long* next, long ldn, float* scores, float* u_out, void* stream) {
    if (logits == nullptr || seed == nullptr || col == nullptr || done == nullptr || seq == nullptr || next == nullptr || B < 1 || V < 1 ||
        V > SMP_VMAX || Vlive < 1 || Vlive > V || !(top_p > 0.f && top_p <= 1.f) || !dec_dtype_ok(dtype) || ldl < V || ncols < 1 ||
        lds < ncols || ldn < 1)
        return HYENA_ERR_BAD_ARG;
    SampleArgs a;
    a.logits = logits; a.scores = scores; a.u_out = u_out; a.seed = seed; a.col = col; a.done = done; a.seq = seq; a.next = next;
    a.ldl = ldl; a.lds = lds; a.ldn = ldn;
    a.B = B; a.V = V; a.Vlive = Vlive; a.ncols = ncols; a.top_k = top_k; a.eos = eos; a.pad = pad;
    a.T = temperature > 1e-6f ? temperature : 1e-6f;
    a.top_p = top_p;
    HY_DEC_DISPATCH(decode_sample_kernel, dim3(B < SMP_MAX_GRID ? B : SMP_MAX_GRID), SMP_VMAX, SMP_LDS_BYTES);
    return hy_launch_error() ? HYENA_ERR_LAUNCH : HYENA_OK;
}

// ---- constrained token sampling (decode_sample_con_kernel): the same, with an allowed set per new token and the token's log-prob -------------
int hyena_decode_sample_constrained(const void* logits, long ldl, int dtype, int B, int V, int Vlive, float temperature, int top_k, float top_p,
                                    const unsigned long long* seed, int eos, int pad, int* col, int* done, long long* seq, long lds,
                                    int ncols, long long* next, long ldn, float* scores, float* u_out, const unsigned long long* allow,
                                    long lda, int nallow, const int* start, float* logprobs, long ldp, void* stream) {
    if (logits == nullptr || seed == nullptr || col == nullptr || done == nullptr || seq == nullptr || next == nullptr || B < 1 || V < 1 ||
        V > SMP_VMAX || Vlive < 1 || Vlive > V || !(top_p > 0.f && top_p <= 1.f) || !dec_dtype_ok(dtype) || ldl < V || ncols < 1 ||
        lds < ncols || ldn < 1)
        return HYENA_ERR_BAD_ARG;
    if ((allow != nullptr || logprobs != nullptr) && start == nullptr) return HYENA_ERR_BAD_ARG;
    if (allow != nullptr && (nallow < 1 || (lda != 0 && lda < nallow))) return HYENA_ERR_BAD_ARG;
    if (logprobs != nullptr && ldp < 1) return HYENA_ERR_BAD_ARG;
    SampleConArgs a;
    a.logits = logits; a.scores = scores; a.u_out = u_out; a.seed = seed; a.col = col; a.done = done; a.seq = seq; a.next = next;
    a.ldl = ldl; a.lds = lds; a.ldn = ldn;
    a.B = B; a.V = V; a.Vlive = Vlive; a.ncols = ncols; a.top_k = top_k; a.eos = eos; a.pad = pad;
    a.T = temperature > 1e-6f ? temperature : 1e-6f;
    a.top_p = top_p;
    a.allow = allow; a.start = start; a.logprobs = logprobs; a.lda = lda; a.ldp = ldp; a.nallow = allow != nullptr ? nallow : 0;
    HY_DEC_DISPATCH(decode_sample_con_kernel, dim3(B < SMP_MAX_GRID ? B : SMP_MAX_GRID), SMP_VMAX, SMP_CON_LDS_BYTES);
    return hy_launch_error() ? HYENA_ERR_LAUNCH : HYENA_OK;
}

// ---- automaton-constrained sampling (decode_sample_con_kernel, AUTO): the mask comes from M at the row's automaton state -------------------
static bool dec_auto_ok(const unsigned long long* M, int Nt, int S, const int* delta, int Vdelta, const int* dstate, int V) {
    return M != nullptr && delta != nullptr && dstate != nullptr && S >= 1 && S <= HYENA_DECODE_AUTOMATON_MAX_STATES && Nt >= 1 &&
           (long)Nt * S <= HYENA_DECODE_AUTOMATON_MAX_TABLE && Vdelta == V;
}

int hyena_decode_sample_automaton(const void* logits, long ldl, int dtype, int B, int V, int Vlive, float temperature, int top_k, float top_p,
                                  const unsigned long long* seed, int eos, int pad, int* col, int* done, long long* seq, long lds, int ncols,
                                  long long* next, long ldn, float* scores, float* u_out, const unsigned long long* M, int Nt, int S,
                                  const int* delta, int Vdelta, int* dstate, const int* start, float* logprobs, long ldp, void* stream) {
    if (logits == nullptr || seed == nullptr || col == nullptr || done == nullptr || seq == nullptr || next == nullptr || B < 1 || V < 1 ||
        V > SMP_VMAX || Vlive < 1 || Vlive > V || !(top_p > 0.f && top_p <= 1.f) || !dec_dtype_ok(dtype) || ldl < V || ncols < 1 ||
        lds < ncols || ldn < 1)
        return HYENA_ERR_BAD_ARG;
    if (start == nullptr || !dec_auto_ok(M, Nt, S, delta, Vdelta, dstate, V)) return HYENA_ERR_BAD_ARG;
    if (logprobs != nullptr && ldp < 1) return HYENA_ERR_BAD_ARG;
    SampleAutoArgs a;
    a.logits = logits; a.scores = scores; a.u_out = u_out; a.seed = seed; a.col = col; a.done = done; a.seq = seq; a.next = next;
    a.ldl = ldl; a.lds = lds; a.ldn = ldn;
    a.B = B; a.V = V; a.Vlive = Vlive; a.ncols = ncols; a.top_k = top_k; a.eos = eos; a.pad = pad;
    a.T = temperature > 1e-6f ? temperature : 1e-6f;
    a.top_p = top_p;
    a.allow = nullptr; a.start = start; a.logprobs = logprobs; a.lda = 0; a.ldp = ldp; a.nallow = 0;
    a.t.dstate = dstate; a.t.M = M; a.t.delta = delta; a.t.S = S; a.t.Nt = Nt;
    HY_DEC_DISPATCH_AUTO(decode_sample_con_kernel, SampleAutoArgs, dim3(B < SMP_MAX_GRID ? B : SMP_MAX_GRID), SMP_VMAX, SMP_CON_LDS_BYTES);
    return hy_launch_error() ? HYENA_ERR_LAUNCH : HYENA_OK;
}

// ---- beam search (decode_beam_kernel, decode_reorder_fan_kernel, decode_beam_backtrack_kernel) ---------------------------------------------
static_assert(BEAM_MAX == HYENA_DECODE_BEAM_MAX, "the header's beam limit");

int hyena_decode_beam(const void* logits, long ldl, int dtype, int B, int fan, int V, int Vlive, int eos, int pad, int* col, int* done,
                      float* beam_score, const int* start, int* parent, long long* next, long ldn, int ncols,
                      const unsigned long long* allow, long lda, int nallow, int* tok_hist, int* parent_hist, float* lp_hist, long ldh,
                      int nrec, void* stream) {
    if (logits == nullptr || col == nullptr || done == nullptr || beam_score == nullptr || start == nullptr || parent == nullptr ||
        next == nullptr || B < 1 || fan < 1 || fan > BEAM_MAX || B % fan != 0 || V < 1 || V > SMP_VMAX || Vlive < 1 || Vlive > V ||
        !dec_dtype_ok(dtype) || ldl < V || ncols < 1 || ldn < 1)
        return HYENA_ERR_BAD_ARG;
    if (allow != nullptr && (nallow < 1 || (lda != 0 && lda < nallow))) return HYENA_ERR_BAD_ARG;
    const bool rec = tok_hist != nullptr || parent_hist != nullptr || lp_hist != nullptr;
    if (rec && (nrec < 1 || ldh < nrec)) return HYENA_ERR_BAD_ARG;
    BeamArgs a;
    a.logits = logits; a.score = beam_score; a.col = col; a.done = done; a.start = start; a.parent = parent; a.next = next;
    a.allow = allow; a.tok_hist = tok_hist; a.parent_hist = parent_hist; a.lp_hist = lp_hist;
    a.ldl = ldl; a.ldn = ldn; a.lda = lda; a.ldh = ldh;
    a.B = B; a.fan = fan; a.V = V; a.Vlive = Vlive; a.ncols = ncols; a.eos = eos; a.pad = pad;
    a.nallow = allow != nullptr ? nallow : 0; a.nrec = rec ? nrec : 0;
    const int G = B / fan;
    HY_DEC_DISPATCH(decode_beam_kernel, dim3(G < SMP_MAX_GRID ? G : SMP_MAX_GRID), SMP_VMAX, BEAM_LDS_BYTES);
    return hy_launch_error() ? HYENA_ERR_LAUNCH : HYENA_OK;
}

// ---- the beam step with the rows' allowed sets from an automaton (decode_beam_kernel, AUTO) ----------------------------------------------
int hyena_decode_beam_automaton(const void* logits, long ldl, int dtype, int B, int fan, int V, int Vlive, int eos, int pad, int* col,
                                int* done, float* beam_score, const int* start, int* parent, long long* next, long ldn, int ncols,
                                const unsigned long long* M, int Nt, int S, const int* delta, int Vdelta, int* dstate, int* tok_hist,
                                int* parent_hist, float* lp_hist, long ldh, int nrec, void* stream) {
    if (logits == nullptr || col == nullptr || done == nullptr || beam_score == nullptr || start == nullptr || parent == nullptr ||
        next == nullptr || B < 1 || fan < 1 || fan > BEAM_MAX || B % fan != 0 || V < 1 || V > SMP_VMAX || Vlive < 1 || Vlive > V ||
        !dec_dtype_ok(dtype) || ldl < V || ncols < 1 || ldn < 1)
        return HYENA_ERR_BAD_ARG;
    if (!dec_auto_ok(M, Nt, S, delta, Vdelta, dstate, V)) return HYENA_ERR_BAD_ARG;
    const bool rec = tok_hist != nullptr || parent_hist != nullptr || lp_hist != nullptr;
    if (rec && (nrec < 1 || ldh < nrec)) return HYENA_ERR_BAD_ARG;
    BeamAutoArgs a;
    a.logits = logits; a.score = beam_score; a.col = col; a.done = done; a.start = start; a.parent = parent; a.next = next;
    a.allow = nullptr; a.tok_hist = tok_hist; a.parent_hist = parent_hist; a.lp_hist = lp_hist;
    a.ldl = ldl; a.ldn = ldn; a.lda = 0; a.ldh = ldh;
    a.B = B; a.fan = fan; a.V = V; a.Vlive = Vlive; a.ncols = ncols; a.eos = eos; a.pad = pad;
    a.nallow = 0; a.nrec = rec ? nrec : 0;
    a.t.dstate = dstate; a.t.M = M; a.t.delta = delta; a.t.S = S; a.t.Nt = Nt;
    const int G = B / fan;
    HY_DEC_DISPATCH_AUTO(decode_beam_kernel, BeamAutoArgs, dim3(G < SMP_MAX_GRID ? G : SMP_MAX_GRID), SMP_VMAX, BEAM_AUTO_LDS_BYTES);
    return hy_launch_error() ? HYENA_ERR_LAUNCH : HYENA_OK;
}

int hyena_decode_reorder_fan(void* vgr, float* tail, const int* parent, const int* pos, int B, int Bcap, int fan, int D, int Lcap, int S,
                             int c0, int ldr, int dtype, void* stream) {
    if (tail == nullptr || parent == nullptr || pos == nullptr || !dec_fan_ok(false, nullptr, vgr, B, fan, D, Lcap, S, 0, ldr, dtype) ||
        fan > BEAM_MAX || Bcap < B || c0 < S || c0 > Lcap)
        return HYENA_ERR_BAD_ARG;
    ReorderArgs a;
    a.vg = vgr; a.tail = tail; a.parent = parent; a.pos = pos;
    a.B = B; a.Bcap = Bcap; a.fan = fan; a.D = D; a.Lcap = Lcap; a.S = S; a.c0 = c0; a.lda = ldr;
    const size_t items = (size_t)(B / fan) * D * ((size_t)(Lcap - c0) + 6);
    const size_t blocks = (items + DEC_THREADS - 1) / DEC_THREADS;
    HY_DEC_DISPATCH(decode_reorder_fan_kernel, dim3((unsigned)(blocks < 8192 ? blocks : 8192)), DEC_THREADS, 0);
    return hy_launch_error() ? HYENA_ERR_LAUNCH : HYENA_OK;
}

int hyena_decode_beam_backtrack(const int* tok_hist, const int* parent_hist, const float* lp_hist, long ldh, int B, int fan, int n_done,
                                int n_ret, long long* seq, long lds, int P, float* logprobs, long ldp, void* stream) {
    if (tok_hist == nullptr || parent_hist == nullptr || seq == nullptr || B < 1 || fan < 1 || fan > BEAM_MAX || B % fan != 0 || n_ret < 1 ||
        n_ret > fan || n_done < 0 || ldh < n_done || ldh < 1 || P < 0 || lds < (long)P + n_done ||
        (logprobs != nullptr && (lp_hist == nullptr || ldp < n_done || ldp < 1)))
        return HYENA_ERR_BAD_ARG;
    BacktrackArgs a;
    a.tok_hist = tok_hist; a.parent_hist = parent_hist; a.lp_hist = lp_hist; a.seq = seq; a.logprobs = logprobs;
    a.ldh = ldh; a.lds = lds; a.ldp = ldp;
    a.B = B; a.fan = fan; a.n_done = n_done; a.n_ret = n_ret; a.P = P;
    const int rows = B / fan * n_ret;
    HY_LAUNCH(decode_beam_backtrack_kernel, dim3((rows + DEC_THREADS - 1) / DEC_THREADS), dim3(DEC_THREADS), 0, stream, a);
    return hy_launch_error() ? HYENA_ERR_LAUNCH : HYENA_OK;
}

}  // extern "C"

// ---- edited windows of a reference sequence (variant_kernels.h) ---------------------------------------------------------------------------
static_assert(VAR_TMAX == HYENA_VARIANT_TMAX, "the header's window limit");
namespace {
bool var_shape_ok(int M, int D, int T, int dtype) {
    return M >= 1 && D >= 1 && D <= 65535 && T >= 1 && T <= VAR_TMAX && (long)M * T * D <= (1L << 38) && dec_dtype_ok(dtype);
}
}  // namespace

extern "C" {

int hyena_variant_pre(const void* x3, int ldx, const float* bin, const float* w, const float* b, const float* tail, const int* pos,
                      const void* vg_ref, float* x0, float* delta, int M, int D, int T, int dtype, void* stream) {
    if (x3 == nullptr || w == nullptr || b == nullptr || tail == nullptr || pos == nullptr || vg_ref == nullptr || x0 == nullptr ||
        delta == nullptr || !var_shape_ok(M, D, T, dtype) || ldx < 3 * D)
        return HYENA_ERR_BAD_ARG;
    VarPreArgs a;
    a.x = x3; a.bin = bin; a.w = w; a.b = b; a.tail = tail; a.pos = pos; a.vg_ref = vg_ref; a.x0 = x0; a.delta = delta;
    a.M = M; a.D = D; a.T = T; a.ldx = ldx;
    HY_DEC_DISPATCH(variant_pre_kernel, dim3((unsigned)(((size_t)M * T * D + VAR_THREADS - 1) / VAR_THREADS)), VAR_THREADS, 0);
    return hy_launch_error() ? HYENA_ERR_LAUNCH : HYENA_OK;
}

int hyena_variant_conv(const float* y_ref, const float* delta, const float* k, int ldk, const float* fb, const float* x0, void* z, int M, int D,
                       int T, int dtype, void* stream) {
    if (y_ref == nullptr || delta == nullptr || k == nullptr || x0 == nullptr || z == nullptr || !var_shape_ok(M, D, T, dtype) || ldk < T)
        return HYENA_ERR_BAD_ARG;
    VarConvArgs a;
    a.y_ref = y_ref; a.delta = delta; a.k = k; a.fb = fb; a.x0 = x0; a.z = z;
    a.M = M; a.D = D; a.T = T; a.ldk = ldk;
    a.cw = var_cw(D, T); a.pp = var_pairs(T); a.stride = var_stride(T);
    HY_DEC_DISPATCH(variant_conv_kernel, dim3(M, (D + a.cw - 1) / a.cw), VAR_THREADS, (size_t)2 * a.cw * a.stride * sizeof(float));
    return hy_launch_error() ? HYENA_ERR_LAUNCH : HYENA_OK;
}

}  // extern "C"
