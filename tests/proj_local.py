"""fp64 references and derived bounds for the matrix-core kernels of csrc/proj_kernels.h and csrc/proj2_kernels.h -- in_proj (both generations),
mlp_kernel<0> / <1>, out_proj (both generations, with and without the LayerNorm epilogue), outproj_dgrad_gate_bwd, colsum -- each called ON ITS OWN
through the C ABI on caller-made buffers.  Shared by tests/test_proj_local_emu.py and tests/test_gpu_proj_local.py.  Plain torch, device-agnostic;
not a test file.  Derivations, measured figures, margins and mutants: profiles/proj_local.md.  Notation of tests/shell_local.py: u = 2^-24,
gamma_k = k u / (1 - k u); every reference starts from the STORED 16-bit operands widened exactly to fp64; EVERY element is compared.

    product   s = sum_k w_k x_k (+ bias)     E32 = gamma_(K + c) (sum_k |w_k| |x_k| + |bias|),  c = 1 with a bias, else 0
        (a product of two 16-bit values is exact in fp32; the matrix instructions add K of them onto a zero accumulator, chained over the K-steps,
         and the kernel adds the bias behind them: K + c additions in SOME order, each assumed to round to nearest -- any order obeys gamma_(K + c))
    16-bit output      |got - ref64| <= E + half_ulp_io(|ref64| + E)        E = E32 propagated through what follows the product
    tanh-GELU (pm_gelu / pm_dgelu, evaluated on the ROUNDED a)               gelu_err / dgelu_err below, operation by operation
    sums      |got - ref64| <= gamma_(n + t) (S + H) + H                     n = depth of the additions read from the kernel, t = roundings in a term
"""
import math

import torch

from tests import shell_local as SL
from tests.shell_local import SENTINEL, U, Buf, gamma, half_ulp_io

NT = 64                                                   # positions per tile (PJ_NT)
DTYPES = [torch.bfloat16, torch.float16]
NAME = SL.NAME
W_SCALE = 2.0 ** -4                                       # weights: magnitudes in [2^-5, 2^-3): sums of K = 128 / 256 products stay O(1)
S2PI = math.sqrt(2.0 / math.pi)
LOG2E = 1.0 / math.log(2.0)


def _op(shape, g, T, dev, scale=1.0):
    """magnitudes in [0.5, 2) * scale (a power of two: the rounding to T is the same) with random signs"""
    return (SL._operand(shape, g, torch.float64, "cpu") * scale).to(T).to(dev)


def _ceil(a, b):
    return -(-a // b)


def schedule(tiles, cap, floor):
    """csrc/proj.hip: `cap` runs at most, runs of at least `floor` tiles once there are that many -> (runs, tiles per run)"""
    runs = min(cap, tiles)
    tpw = _ceil(tiles, runs)
    if tpw < floor and tiles >= floor:
        tpw = floor
    return _ceil(tiles, tpw), tpw


class _Stats(SL._Stats):
    def line(self, label):
        return f"[proj-local] {label} " + " ".join(f"{k}={v:.3g}" for k, v in self.items())


def _hold16(st, name, buf, index, ref, E, T, where=None):
    """every element of buf.view[index] within E + half an ulp of T; the sentinel everywhere else; a failure names the worst element"""
    got = buf.view[index]
    assert bool(torch.isfinite(got).all()), name + ": not finite"
    assert buf.untouched(index), name + ": an element the contract leaves alone was written"
    bound = E + half_ulp_io(ref.abs() + E, T)
    diff = (got.double() - ref).abs()
    if not bool((diff <= bound).all()):
        i = int((diff / bound.clamp_min(1e-300)).argmax())
        idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), diff.shape))
        raise AssertionError((name, "worst element", idx, where(idx) if where else None, float(diff[idx]), float(bound[idx]), int((diff > bound).sum())))
    st.hold(name, got, ref, bound)
    return bound


def product64(W, x, bias=None):
    """W (C, K), x (P, K) fp64, bias (C,) or None -> s (C, P), E32 (C, P)"""
    s, A = W @ x.t(), W.abs() @ x.abs().t()
    if bias is not None:
        s, A = s + bias[:, None], A + bias.abs()[:, None]
    return s, gamma(W.shape[1] + (bias is not None)) * A


# ---- tanh-GELU as pm_gelu / pm_dgelu evaluate it ------------------------------------------------------------------------------------------
#   x2 = x x;  p = fma(x2, C2, C1);  w = x p;  e = exp2(w);  sg = rcp(1 + e);  gelu = x sg
#   q = x fma(x2, C4, C3);  gelu' = fma(q sg, 1 - sg, sg)
# C1 .. C4 are fp32 roundings of the exact constants (one u each).  C1 and C2 have one sign and so have C3 and C4: |w| and |q| are the sums of
# the magnitudes, so w and q carry gamma_4 RELATIVE (the x^2 term passes x2, the constant, the fma and the product; the other one three of them).
# exp2 turns the absolute error of w into the relative error expm1(ln 2 dw) of e (its conditioning |w| ln 2); v_exp_f32 and v_rcp_f32 enter
# with 1 ulp = 2 u relative each (the ISA documentation; the emulator's exp2f and 1 / d are at least that good).
def _z2(x):
    return 2.0 * S2PI * (x + 0.044715 * x ** 3)


def gelu64(x):
    return x * torch.sigmoid(_z2(x))


def dgelu64(x):
    sg = torch.sigmoid(_z2(x))
    return sg + x * sg * (1.0 - sg) * (2.0 * S2PI * (1.0 + 3.0 * 0.044715 * x * x))


def _sg_rel(x):
    """(sg64, relative error bound of the computed sg)"""
    w = -_z2(x) * LOG2E
    dw = gamma(4) * w.abs()
    e = torch.exp2(w)
    rel_e = torch.expm1(math.log(2.0) * dw) * (1.0 + 2 * U) + 2 * U
    de = e * rel_e / (1.0 + e)                                      # relative error of 1 + e before its own rounding
    rel_d = de + U * (1.0 + de)
    return torch.sigmoid(_z2(x)), rel_d / (1.0 - rel_d) * (1.0 + 2 * U) + 2 * U


def gelu_err(x):
    sg, rel = _sg_rel(x)
    return x.abs() * sg * ((1.0 + rel) * (1.0 + U) - 1.0)


def dgelu_err(x):
    sg, rel = _sg_rel(x)
    q = x * (2.0 * S2PI * (1.0 + 3.0 * 0.044715 * x * x))
    t1 = (q * sg).abs()
    rel_t1 = (1.0 + gamma(4)) * (1.0 + rel) * (1.0 + U) - 1.0
    om = (1.0 - sg).abs()
    e_om = sg * rel + U * (om + sg * rel)
    e = t1 * rel_t1 * (om + e_om) + t1 * e_om + sg * rel
    return e + U * (dgelu64(x).abs() + e)


# ---- in_proj + the front of the shell ---------------------------------------------------------------------------------------------------
def _generation(_lib, family, gen):
    prev = _lib.proj_kernel_generation(family)
    assert _lib.proj_kernel_generation(family, gen) == gen
    return prev


def run_inproj(_lib, dev, T, B, Lx, Lc, D, gen, xlayout="cm", rows=True, bias=True, seed=0, label="", path=""):
    """hyena_inproj_pre_fwd_ld of generation `gen`: xT at every (c, b, l < Lx) against the fp64 product, vg against shell_local's fp64 short conv +
    gate of the kernel's OWN stored xT (zero history at each sequence start), sentinels, bit-equal repeat, the wrapper's bits."""
    lib, rp = _lib.lib(), _lib.row_pitch
    code, stream = _lib.dtype_code(T), _lib._backend.stream(dev)
    g = torch.Generator().manual_seed(seed)
    w, b, bin_ = SL._params(3 * D, g, dev, bias)
    u, W = _op((B, Lx, D), g, T, dev), _op((3 * D, D), g, T, dev, W_SCALE)
    xs, csx, bsx = SL.x_strides(3 * D, B, Lx, xlayout, rp)
    vs, ldv = SL.rows_strides(B, D, Lc, rows, rp)
    runs, tpw = schedule(_ceil(B * Lx, NT), 2048 // (D // 64) if gen == 1 else 1024 // (D // 128), 8 if gen == 1 else 16)
    st = _Stats()
    prev = _generation(_lib, 1, gen)
    try:
        assert _lib.proj_supported(B, Lx, D, T)
        with _lib._backend.guard(dev):
            def call():
                xT, vg = Buf((3 * D, B, Lx), xs, T, dev, SENTINEL), Buf((B, D, Lc), vs, T, dev, SENTINEL)
                _lib.check(lib.hyena_inproj_pre_fwd_ld(u.data_ptr(), W.data_ptr(), SL._ptr(bin_), w.data_ptr(), b.data_ptr(), xT.flat.data_ptr(),
                                                       vg.flat.data_ptr(), B, Lx, Lc, D, csx, bsx, ldv, code, stream))
                return xT, vg
            xT, vg = call()
            again = call()
            full = (slice(None),) * 3
            ref, E32 = product64(W.double(), u.double().reshape(B * Lx, D))

            def where(i):
                p = i[1] * Lx + i[2]
                return dict(channel=i[0], seq=i[1], pos=i[2], tile=p // NT, run=p // NT // tpw)
            bx = _hold16(st, "xT", xT, full, ref.view(3 * D, B, Lx), E32.view(3 * D, B, Lx), T, where)
            rv, Ev = SL.pre_fwd64(xT.view.double(), SL._d(bin_), w.double(), b.double(), Lc)
            _hold16(st, "vg", vg, full, rv, Ev, T, lambda i: dict(seq=i[0], channel=i[1], pos=i[2], tile=(i[0] * Lx + i[2]) // NT))
            assert torch.equal(xT.flat, again[0].flat) and torch.equal(vg.flat, again[1].flat), "inproj_pre_fwd is not repeatable bit for bit"
            xw, vw = _lib.inproj_pre_fwd(u, W, bin_, w, b, Lc)
            assert torch.equal(xw, xT.view) and torch.equal(vw, vg.view)
        # a dropped or twice-counted product term is at least min |W| min |u| large
        st["margin"] = float(bx.max()) / (float(W.double().abs().min()) * float(u.double().abs().min()))
    finally:
        _lib.proj_kernel_generation(1, prev)
    print(st.line(f"{label} inproj{gen} {NAME[T]} B={B} Lx={Lx} Lc={Lc} D={D} x={xlayout} rows={int(rows)} bin={int(bias)} runs={runs}x{tpw} [{path}]"),
          flush=True)
    if T == torch.float16:          # bf16: half an ulp of a large |xT| (2^-9 |xT|) can exceed the smallest product; the fp16 run of the case holds the power
        assert st["margin"] < 1.0, st["margin"]
    return st


# ---- the MLP's kernels --------------------------------------------------------------------------------------------------------------------
def mlp_schedule(P, N):
    return schedule(_ceil(P, NT), 2048 // (N // 256), 8)


def run_mlp(_lib, dev, T, P, K, N, seed=0, label="", path=""):
    """hyena_mlp_fc1_gelu_fwd: a against x W1^T + b1, h against the fp64 tanh-GELU of the STORED a (mlp_kernel reads the rounded a back from LDS).
    hyena_mlp_dh_dgelu_bwd on an a of its own (magnitudes in [1, 2): |gelu'| >= 0.08 there, so every da is a full-sized term): da against
    (dy W2) gelu'(a) with dh's 16-bit rounding inside the bound, the records of `part`, db1 against the fp64 column sums of the stored da."""
    lib = _lib.lib()
    code, stream = _lib.dtype_code(T), _lib._backend.stream(dev)
    g = torch.Generator().manual_seed(seed)
    x, W1 = _op((P, K), g, T, dev), _op((N, K), g, T, dev, W_SCALE)
    b1 = _op((N,), g, T, dev, 0.25).float()
    # the backward's operands carry one random sign per k: every product dy_k W2_k is positive, dh cannot cancel, every da is a full-sized term of
    # db1 whose sign is that of gelu'(a) (mixed-sign products are the forward's, the same product loop)
    sgn = _op((K,), g, T, dev).sign()
    dy, W2T = _op((P, K), g, T, dev).abs() * sgn, _op((N, K), g, T, dev, W_SCALE).abs() * sgn
    a_in = (SL._operand((P, N), g, torch.float64, "cpu").sign() * (1.0 + torch.rand((P, N), generator=g, dtype=torch.float64))).to(T).to(dev)
    runs, tpw = mlp_schedule(P, N)
    Pp = _ceil(P, NT) * NT + 1                                   # the outputs own one row behind the last (ragged) tile: all of it keeps the sentinel
    own = (slice(0, P), slice(None))
    st = _Stats()
    assert _lib.mlp_supported(P, K, N, T)
    assert lib.hyena_mlp_partial_floats(P, N) == runs * N, "runs"

    def where(i):
        return dict(pos=i[0], unit=i[1], tile=i[0] // NT, run=i[0] // NT // tpw)
    with _lib._backend.guard(dev):
        def fwd():
            a, h = Buf((Pp, N), (N, 1), T, dev, SENTINEL), Buf((Pp, N), (N, 1), T, dev, SENTINEL)
            _lib.check(lib.hyena_mlp_fc1_gelu_fwd(x.data_ptr(), W1.data_ptr(), b1.data_ptr(), a.flat.data_ptr(), h.flat.data_ptr(), P, K, N, code, stream))
            return a, h

        def bwd():
            da, part = Buf((Pp, N), (N, 1), T, dev, SENTINEL), Buf((runs + 1, N), (N, 1), torch.float32, dev, SENTINEL)
            _lib.check(lib.hyena_mlp_dh_dgelu_bwd(dy.data_ptr(), W2T.data_ptr(), a_in.data_ptr(), da.flat.data_ptr(), part.flat.data_ptr(), P, K, N, code,
                                                  stream))
            return da, part
        a, h = fwd()
        again = fwd()
        ref, E32 = product64(W1.double(), x.double(), b1.double())
        ba = _hold16(st, "a", a, own, ref.t(), E32.t(), T, where)
        a64 = a.view[own].double()
        st["max|a|"] = float(a64.abs().max())
        _hold16(st, "h", h, own, gelu64(a64), gelu_err(a64), T, where)
        assert torch.equal(a.flat, again[0].flat) and torch.equal(h.flat, again[1].flat), "mlp_fc1_gelu_fwd is not repeatable bit for bit"
        da, part = bwd()
        again = bwd()
        dh, E32 = product64(W2T.double(), dy.double())
        dh, E32 = dh.t(), E32.t()
        e_dh = E32 + half_ulp_io(dh.abs() + E32, T)                 # dh is rounded to T before the multiply (`the rounding of the unfused dh tensor`)
        a64 = a_in.double()
        gp, Eg = dgelu64(a64), dgelu_err(a64)
        E = e_dh * gp.abs() + (dh.abs() + e_dh) * Eg + U * (dh.abs() + e_dh) * (gp.abs() + Eg)
        _hold16(st, "da", da, own, dh * gp, E, T, where)
        rec = (slice(0, runs), slice(None))
        assert bool(torch.isfinite(part.view[rec]).all()) and part.untouched(rec), "part: every record of the schedule finite, none behind them"
        # depth of the additions: a lane adds 8 positions of every tile of its run, the 8 lanes of a piece are added in row order, the host adds the records
        n = 8 * tpw + 8 + runs
        d64 = da.view[own].double()
        bsum = gamma(n) * d64.abs().sum(0)
        st.hold("db1", part.view[rec].sum(0), d64.sum(0), bsum)
        st["margin"] = float((bsum / d64.abs().min(0).values).max())
        assert torch.equal(da.flat, again[0].flat) and torch.equal(part.flat, again[1].flat), "mlp_dh_dgelu_bwd is not repeatable bit for bit"
        aw, hw = _lib.mlp_fc1_gelu_fwd(x, W1, b1)
        dw, db1 = _lib.mlp_dh_dgelu_bwd(dy, W2T, a_in)
        assert torch.equal(aw, a.view[own]) and torch.equal(hw, h.view[own]) and torch.equal(dw, da.view[own])
        st.hold("db1", db1, d64.sum(0), bsum)
        st["margin_a"] = float(ba.max()) / (float(W1.double().abs().min()) * float(x.double().abs().min()))
    print(st.line(f"{label} mlp {NAME[T]} P={P} K={K} N={N} runs={runs}x{tpw} [{path}]"), flush=True)
    assert st["margin"] < 1.0, st["margin"]
    if T == torch.float16:
        assert st["margin_a"] < 1.0, st["margin_a"]
    return st


# ---- out_proj with the second gate on its operand load ----------------------------------------------------------------------------------
def _x0(B, Lx, L, D, g, T, dev, xlayout, rp):
    """xT (3D, B, Lx) of which the kernels may read rows [0, D), positions < L: NaN everywhere else (the other rows, positions >= L, every pad)"""
    v = torch.full((3 * D, B, Lx), float("nan"), dtype=T, device=dev)
    v[:D, :, :L] = _op((D, B, L), g, T, dev)
    xs, csx, bsx = SL.x_strides(3 * D, B, Lx, xlayout, rp)
    return Buf.input(v, xs), xs, csx, bsx


def addnorm64(o, Eo, res, lw, lb, eps, K, T):
    """the LayerNorm epilogue (block_kernels.h's arithmetic): v = round_T(acc + bias) + res;  mean = (sum v) / K;  var = sum (v - mean)^2 / K;
    rstd = 1 / sqrt(var + eps);  out = ((v - mean) rstd) w + b.  o, Eo: the fp64 product + bias and its E32.  A lane adds its K / 64 values, six
    butterfly steps add the lanes: sums of depth K / 64 + 5; 1 / K is a power of two.  sqrtf and the division: one ulp (2 u) each at most.
    -> dict name -> (ref, bound) for residual', mean, rstd, and (ref, E) for normed (its rounding to T is added by the caller)"""
    ns = K // 64 + 5
    Eo = Eo + half_ulp_io(o.abs() + Eo, T)
    v = o if res is None else o + res
    Ev = Eo if res is None else Eo + U * (v.abs() + Eo)
    m = v.mean(1, keepdim=True)
    Em = Ev.mean(1, keepdim=True) + gamma(ns) * (v.abs() + Ev).mean(1, keepdim=True)
    d = v - m
    Ed = Ev + Em + U * (d.abs() + Ev + Em)
    sq = (d.abs() + Ed) ** 2
    Esq = 2 * d.abs() * Ed + Ed ** 2 + U * sq
    var = (d * d).mean(1, keepdim=True)
    Evar = Esq.mean(1, keepdim=True) + gamma(ns) * sq.mean(1, keepdim=True)
    s = var + eps
    Es = Evar + U * (s + Evar) + U * eps                                                 # (eps itself is a rounded fp32 value)
    rstd = s ** -0.5
    rel = ((1.0 - Es / s) ** -0.5) * (1.0 + 2 * U) ** 2 - 1.0
    t = d * rstd
    Et = Ed * rstd * (1.0 + rel) + d.abs() * rstd * rel
    Et = Et + U * (t.abs() + Et)
    y = t * lw + lb
    Ey = Et * lw.abs()
    Ey = Ey + U * (t.abs() * lw.abs() + Ey)
    Ey = Ey + U * (y.abs() + Ey)
    return {"residual": (v, Ev), "mean": (m[:, 0], Em[:, 0]), "rstd": (rstd[:, 0], (rstd * rel)[:, 0]), "normed": (y, Ey)}


def run_outproj(_lib, dev, T, B, L, Lx, D, gen, xlayout="cm", rows=True, zpacked=False, bias=True, norm=False, seed=0, label="", path="", lda=None,
                rowbuf=Buf):
    """hyena_outproj_gate_fwd_ld of generation `gen`: zT against shell_local's post_fwd reference, out at EVERY element against zT_stored W^T + bias,
    bit-equal without the zT side output, bit-equal repeat, the wrapper's bits; norm: hyena_outproj_gate_addnorm_fwd_ld with and without an incoming
    residual against the fp64 add + LayerNorm of the fp64 product.  lda / rowbuf: the caller's own row pitch of y, in a buffer of that class
    (tests/limits_local.py: rows gigabytes apart)."""
    lib, rp = _lib.lib(), _lib.row_pitch
    code, stream = _lib.dtype_code(T), _lib._backend.stream(dev)
    g = torch.Generator().manual_seed(seed)
    # z = y c0 is the product's operand: taps, biases and x0 are positive and b_sc >= 1, so c0 >= 1 cannot cancel and |z| >= 0.5 -- a single term of
    # `out` stays above its bound (the margin).  y keeps random signs; mixed-sign filters are the dgrad cases' and tests/shell_local.py's.
    w, b, bin_ = SL._params(3 * D, g, dev, bias)
    w, b, bin_ = w.abs(), 1.0 + b.abs(), None if bin_ is None else bin_.abs()
    x, xs, csx, bsx = _x0(B, Lx, L, D, g, T, dev, xlayout, rp)
    x.view[:D, :, :L] = x.view[:D, :, :L].abs()
    ys, lda = SL.rows_strides(B, D, L, rows, rp, lda)
    y = rowbuf.input(_op((B, D, L), g, T, dev), ys)
    W = _op((D, D), g, T, dev, W_SCALE)
    ob = _op((D,), g, T, dev, 0.25).float() if bias else None
    zs, csz, bsz = ((B * L, L, 1), B * L, L) if zpacked else SL.z_strides(D, B, L, False, rp)
    tps = _ceil(L, NT)
    runs, tpw = schedule(B * tps, 2048 if gen == 1 else (1024 if D == 256 else 2048), 8)
    P = B * L
    own, full = (slice(0, P), slice(None)), (slice(None),) * 3
    st = _Stats()

    def where(i):
        t = (i[0] // L) * tps + min(i[0] % L, L - 1) // NT
        return dict(seq=i[0] // L, pos=i[0] % L, channel=i[1], tile=t, run=t // tpw)
    prev = _generation(_lib, 0, gen)
    try:
        assert _lib.outproj_supported(B, L, Lx, D, T)
        with _lib._backend.guard(dev):
            def call(want_z, ln=None, res=None):
                out, zT = Buf((P + 1, D), (D, 1), T, dev, SENTINEL), Buf((D, B, L), zs, T, dev, SENTINEL)
                extra = [Buf((P + 1, D), (D, 1), torch.float32, dev, SENTINEL), Buf((P + 1,), (1,), torch.float32, dev, SENTINEL),
                         Buf((P + 1,), (1,), torch.float32, dev, SENTINEL)] if ln else [None] * 3
                _lib.check(lib.hyena_outproj_gate_addnorm_fwd_ld(
                    y.flat.data_ptr(), x.flat.data_ptr(), SL._ptr(bin_), w.data_ptr(), b.data_ptr(), W.data_ptr(), SL._ptr(ob), SL._ptr(res),
                    ln[0].data_ptr() if ln else None, ln[1].data_ptr() if ln else None, 1e-5 if ln else 0.0, out.flat.data_ptr(),
                    extra[0].flat.data_ptr() if ln else None, extra[1].flat.data_ptr() if ln else None, extra[2].flat.data_ptr() if ln else None,
                    zT.flat.data_ptr() if want_z else None, B, L, Lx, D, csx, bsx, csz, bsz, lda, code, stream))
                return [out, zT] + extra
            out, zT = call(True)[:2]
            x64 = torch.zeros((3 * D, B, L), dtype=torch.float64, device=dev)
            x64[:D] = x.view[:D, :, :L].double()
            rz, Ez = SL.post_fwd64(x64, SL._d(bin_), w.double(), b.double(), y.view.double(), L)
            _hold16(st, "zT", zT, full, rz, Ez, T, lambda i: dict(channel=i[0], seq=i[1], pos=i[2], tile=i[1] * tps + i[2] // NT))
            z2 = zT.view.double().permute(1, 2, 0).reshape(P, D)
            ref, E32 = product64(W.double(), z2, SL._d(ob))
            ref, E32 = ref.t(), E32.t()
            bo = _hold16(st, "out", out, own, ref, E32, T, where)
            st["margin"] = float(bo.max()) / (float(W.double().abs().min()) * float(z2.abs().min()))
            again, noz = call(True), call(False)
            assert torch.equal(out.flat, again[0].flat) and torch.equal(zT.flat, again[1].flat), "outproj_gate_fwd is not repeatable bit for bit"
            assert torch.equal(noz[0].flat, out.flat) and bool((noz[1].flat == SENTINEL).all()), "want_z = False: other bits of out, or zT written"
            ow, zw = _lib.outproj_gate_fwd(y.view, x.view, bin_, w, b, W, ob, want_z=True)
            assert torch.equal(ow.reshape(P, D), out.view[own]) and torch.equal(zw, zT.view)
            if norm:
                lw, lb = (1.0 + 0.25 * torch.randn(D, generator=g)).to(dev), (0.25 * torch.randn(D, generator=g)).to(dev)
                for res in (_op((P, D), g, torch.float32, dev, 2.0), None):
                    o, z, r, mean, rstd = call(True, (lw, lb), res)
                    assert torch.equal(z.flat, zT.flat)
                    R = addnorm64(ref, E32, SL._d(res), lw.double(), lb.double(), float(torch.tensor(1e-5, dtype=torch.float32)), D, T)
                    tag = ".res" if res is not None else ""
                    _hold16(st, "ln.normed" + tag, o, own, *R["normed"], T, where)
                    _hold16(st, "ln.residual" + tag, r, own, *R["residual"], torch.float32, where)
                    _hold16(st, "ln.mean" + tag, mean, (slice(0, P),), *R["mean"], torch.float32)
                    _hold16(st, "ln.rstd" + tag, rstd, (slice(0, P),), *R["rstd"], torch.float32)
                    again = call(True, (lw, lb), res)
                    assert all(torch.equal(p.flat, q.flat) for p, q in zip((o, z, r, mean, rstd), again)), "the LayerNorm epilogue is not repeatable"
    finally:
        _lib.proj_kernel_generation(0, prev)
    print(st.line(f"{label} outproj{gen} {NAME[T]} B={B} L={L} Lx={Lx} D={D} x={xlayout} rows={int(rows)} zpacked={int(zpacked)} bias={int(bias)} "
                  f"norm={int(norm)} runs={runs}x{tpw} [{path}]"), flush=True)
    if T == torch.float16:
        assert st["margin"] < 1.0, st["margin"]
    return st


# ---- out_proj's input gradient with the gate's backward -------------------------------------------------------------------------------------
def dgrad_schedule(B, L, D):
    return schedule(B * _ceil(L, NT), 512 // (D // 128), 16)


def run_dgrad(_lib, dev, T, B, L, Lx, D, exact, xlayout="cm", rows=True, bias=True, seed=0, label="", path="", lda=None, rowbuf=Buf):
    """hyena_outproj_dgrad_gate_bwd_ld: dyc, dxT[0:D] and the five sums of every channel against shell_local's post_bwd expressions at the fp64
    dz^T = W_out^T dy^T, the kernel's rounding of dz^T to T (never stored) inside every bound.  exact: dy in {-1, 1} and three non-zero columns
    of W_out^T in {-1, 1} -- dz^T in {+-1, +-3} is exact in fp32 in any order and in T, its error term vanishes and the bound of every sum stays
    below the smallest single term (asserted): a dropped or twice-counted position cannot hide.  With random operands half an ulp of T of every
    dz^T enters each sum's bound, which then exceeds a single term at any useful size in either type (profiles/proj_local.md)."""
    lib, rp = _lib.lib(), _lib.row_pitch
    code, stream = _lib.dtype_code(T), _lib._backend.stream(dev)
    g = torch.Generator().manual_seed(seed)
    w, b, bin_ = SL._params(3 * D, g, dev, bias)
    if exact:
        dy2 = (torch.randint(0, 2, (B * L, D), generator=g) * 2 - 1).to(T).to(dev)
        Wt = torch.zeros((D, D), dtype=T, device=dev)
        Wt[:, [1, D // 2, D - 1]] = (torch.randint(0, 2, (D, 3), generator=g) * 2 - 1).to(T).to(dev)
    else:
        dy2, Wt = _op((B * L, D), g, T, dev), _op((D, D), g, T, dev, W_SCALE)
    x, xs, csx, bsx = _x0(B, Lx, L, D, g, T, dev, xlayout, rp)
    ys, lda = SL.rows_strides(B, D, L, rows, rp, lda)                              # (lda / rowbuf: as in run_outproj; y and dyc)
    y = rowbuf.input(_op((B, D, L), g, T, dev), ys)
    tps = _ceil(L, NT)
    runs, tpw = dgrad_schedule(B, L, D)
    st = _Stats()
    assert _lib.outproj_dgrad_supported(B, L, D, T)
    assert lib.hyena_outproj_dgrad_partial_floats(B, L, D) == D * runs * 8, "runs"
    with _lib._backend.guard(dev):
        def call():
            dyc, dx = rowbuf((B, D, L), ys, T, dev, SENTINEL), Buf((3 * D, B, Lx), xs, T, dev, SENTINEL)
            part = Buf((D, runs, 8), (runs * 8, 8, 1), torch.float32, dev, SENTINEL)
            _lib.check(lib.hyena_outproj_dgrad_gate_bwd_ld(dy2.data_ptr(), Wt.data_ptr(), y.flat.data_ptr(), x.flat.data_ptr(), SL._ptr(bin_), w.data_ptr(),
                                                           b.data_ptr(), dyc.flat.data_ptr(), dx.flat.data_ptr(), part.flat.data_ptr(), B, L, Lx, D, csx,
                                                           bsx, lda, code, stream))
            return dyc, dx, part
        dyc, dx, part = call()
        again = call()
        dz, E32 = product64(Wt.double(), dy2.double())
        dz, E32 = dz.view(D, B, L), E32.view(D, B, L)
        e_dz = torch.zeros_like(dz) if exact else E32 + half_ulp_io(dz.abs() + E32, T)
        x64, w64, b64, bin64 = x.view[:D, :, :L].double(), w[:D].double(), b[:D].double(), None if bin_ is None else bin_[:D].double()
        c0, e0 = SL._sc(x64, bin64, w64, b64, 0, D, L)
        yT = y.view.double().permute(1, 0, 2)
        dzm = dz.abs() + e_dz
        da, h = dz * yT, e_dz * yT.abs()

        def where(i):
            t = i[1] * tps + i[2] // NT
            return dict(channel=i[0], seq=i[1], pos=i[2], tile=t, run=t // tpw)
        _hold16(st, "dyc", dyc, (slice(None),) * 3, (dz * c0).permute(1, 0, 2),
                (e_dz * c0.abs() + dzm * e0 + U * dzm * (c0.abs() + e0)).permute(1, 0, 2), T, lambda i: where((i[1], i[0], i[2])))
        _hold16(st, "dxT", dx, (slice(0, D), slice(None), slice(0, L)), SL.convT64(w64, da), SL._convT_err(w64, da, h + U * (da.abs() + h)), T, where)
        rec = (slice(None), slice(None), slice(0, 5))
        assert bool(torch.isfinite(part.view[rec]).all()) and part.untouched(rec), "records: five finite floats each, floats 5 - 7 left alone"
        ref, S, H, small = SL._sums64(da, h, x64, bin64, w64, L)
        # depth of the additions: a lane adds the 8 positions of its piece in every tile of its run, three butterfly steps add the 8 pieces of a
        # channel, the host adds the records
        bound = SL.sums_bound(S, H, 8 * tpw + 3 + runs)
        got = part.view[:, :, :5].sum(1).double()
        diff = (got - ref).abs()
        if not bool((diff <= bound).all()):
            i = int((diff / bound.clamp_min(1e-300)).argmax())
            raise AssertionError(("sums", "worst", dict(channel=i // 5, which=i % 5), float(diff.view(-1)[i]), float(bound.view(-1)[i]), int((diff > bound).sum())))
        st.hold("sums", got, ref, bound)                                              # each channel, each of the five, against its own bound
        st["margin"] = float(bound.max()) / small
        assert all(p.same(q) for p, q in zip((dyc, dx, part), again)), "outproj_dgrad_gate_bwd is not repeatable bit for bit"
        del again
        dxw = Buf((3 * D, B, Lx), xs, T, dev, SENTINEL)
        dw, pw = _lib.outproj_dgrad_gate_bwd(dy2, Wt, y.view, x.view, bin_, w, b, dxw.view)
        assert torch.equal(dw, dyc.view) and torch.equal(dxw.flat, dx.flat) and torch.equal(pw[:, :, :5], part.view[:, :, :5])
    print(st.line(f"{label} dgrad {NAME[T]} B={B} L={L} Lx={Lx} D={D} exact={int(exact)} x={xlayout} rows={int(rows)} bin={int(bias)} runs={runs}x{tpw} "
                  f"[{path}]"), flush=True)
    if exact:
        assert st["margin"] < 1.0, st["margin"]
    return st


def post_bwd_sum_scales(dzT, y, xT, bin_, w, L, chunk=16):
    """S (D, 5): the sums of the MAGNITUDES of the terms of (dw0, dw1, dw2, db_sc, db_in) of channels [0, D) -- what two fp32 evaluations of those
    sums in different orders may differ by is (gamma_(n1 + 4) + gamma_(n2 + 4)) S per channel.  Evaluated in fp64, `chunk` channels at a time."""
    out = []
    for lo in range(0, dzT.shape[0], chunk):
        hi = lo + chunk
        da = dzT[lo:hi].double() * y[:, lo:hi].permute(1, 0, 2).double()
        out.append(SL._sums64(da, torch.zeros_like(da), xT[lo:hi, :, :L].double(), None if bin_ is None else bin_[lo:hi].double(), w[lo:hi].double(), L)[1])
    return torch.cat(out)


def dgrad_vs_cm_sums_bound(S, B, L, D, nrec_cm, T, exact):
    """per channel and sum: the fused kernel's records against cm_post_bwd's on the same operands.  exact: the same terms in two orders.  Otherwise the
    two dz^T differ by rounding flips, at most one ulp of T (2^-7 / 2^-10 of its magnitude) in every term."""
    runs, tpw = dgrad_schedule(B, L, D)
    bound = (gamma(8 * tpw + 3 + runs + 4) + gamma(SL.CM_V + 6 + 2 + nrec_cm + 4)) * S
    return bound if exact else bound + (2.0 ** -7 if T == torch.bfloat16 else 2.0 ** -10) * S


def mlp_db1_bound(da, P, N):
    """db1 against the fp64 column sums of the stored da: gamma_n sum |da|, n = the depth of the additions (run_mlp)"""
    runs, tpw = mlp_schedule(P, N)
    return gamma(8 * tpw + 8 + runs) * da.double().abs().sum(0)


# ---- colsum ---------------------------------------------------------------------------------------------------------------------------------
def run_colsum(_lib, dev, T, P, N, seed=0, label="", path=""):
    lib = _lib.lib()
    code, stream = _lib.dtype_code(T), _lib._backend.stream(dev)
    x = _op((P, N), torch.Generator().manual_seed(seed), T, dev)
    g0 = min(max(_ceil(P, 512), 1), 512)
    rpw = _ceil(P, g0)
    G, rstep = _ceil(P, rpw), 256 // (N // 8)
    assert lib.hyena_colsum_supported(P, N, code) and lib.hyena_colsum_partial_floats(P, N) == g0 * N
    st = _Stats()
    with _lib._backend.guard(dev):
        def call():
            part, out = Buf((g0 + 1, N), (N, 1), torch.float32, dev, SENTINEL), Buf((N + 8,), (1,), torch.float32, dev, SENTINEL)
            _lib.check(lib.hyena_colsum(x.data_ptr(), part.flat.data_ptr(), out.flat.data_ptr(), P, N, code, stream))
            return part, out
        part, out = call()
        again = call()
        assert part.untouched((slice(0, G), slice(None))) and out.untouched((slice(0, N),))
        # a thread adds every rstep-th row of its workgroup's, the rstep threads of a piece are added in order, then a quarter of the G records in order
        # and the four quarters
        n = _ceil(rpw, rstep) + (rstep - 1) + _ceil(G, 4) + 3
        x64 = x.double()
        bound = gamma(n) * x64.abs().sum(0)
        st.hold("colsum", out.view[:N], x64.sum(0), bound)
        st["margin"] = float((bound / x64.abs().min(0).values).max())
        assert torch.equal(part.flat, again[0].flat) and torch.equal(out.flat, again[1].flat)
        assert torch.equal(_lib.colsum(x), out.view[:N])
    print(st.line(f"{label} colsum {NAME[T]} P={P} N={N} G={G} rows={rpw} [{path}]"), flush=True)
    assert st["margin"] < 1.0, st["margin"]
    return st


# ---- the cases: the smallest shapes that reach each path of the schedules in csrc/proj.hip ---------------------------------------------------
# in_proj: tiles = ceil(B Lx / 64) over the FLATTENED positions.  Generation 1: runs of 8 tiles once there are 8 (below: one tile per run), grid
# rounded up to 8 runs; generation 2: runs of 16.  A run's first tile takes its halo from a warm-up tile; the halo is zeroed at a sequence start.
INPROJ_CASES = [
    # (B, Lx, Lc, D, path)
    (1, 8, 8, 128, "the minimum: one ragged tile"), (1, 9, 7, 128, "ragged tile, Lc < Lx"), (2, 63, 63, 128, "sequence start inside tile 0"),
    (1, 64, 64, 256, "one whole tile"), (3, 65, 64, 128, "sequence starts 1, 2 positions into tiles 1, 2; Lc < Lx"), (2, 127, 127, 128, "4 tiles, ragged end"),
    (1, 128, 120, 256, "two whole tiles, Lc < Lx"), (3, 129, 129, 128, "7 tiles: 7 runs of one, one idle workgroup slot"),
    (1, 512, 512, 128, "8 tiles: one run of 8 (gen 1), 8 runs (gen 2)"), (1, 520, 509, 256, "9 tiles: runs of 8 + 1 ragged (gen 1)"),
    (2, 512, 512, 128, "16 tiles; a sequence starts ON the second run's first tile (gen 1): the warm-up tile's halo must be zeroed"),
    (2, 511, 511, 128, "16 tiles; run boundary 1 position after a sequence start (gen 1)"),
    (2, 510, 500, 128, "16 tiles; run boundary 2 positions after a sequence start (gen 1)"),
    (1, 1030, 1030, 128, "17 tiles: runs 8, 8, 1 (gen 1); 16 + 1 (gen 2), ragged last tile"),
    (3, 320, 320, 128, "15 tiles: two runs (gen 1), 15 runs of one (gen 2)"),
    (2, 1023, 1023, 128, "32 tiles; run boundary 1 position after a sequence start (gen 2)"),
    (2, 1024, 1024, 128, "32 tiles; a sequence starts ON a run's first tile (gen 2)"),
    (1, 2106, 2100, 256, "33 tiles: runs 16, 16, 1 (gen 2), 8 x 4 + 1 (gen 1); d_model 256"),
]
MLP_CASES = [
    (1, 128, 256, "one position"), (7, 256, 256, "one ragged tile"), (63, 128, 512, "ragged tile, two unit groups"), (64, 256, 1024, "one whole tile, four unit groups"),
    (65, 128, 256, "whole + ragged: 2 runs of one tile"), (77, 256, 512, "2 runs of one tile"), (7 * 64, 128, 256, "7 tiles: 7 runs, one idle workgroup"),
    (8 * 64, 128, 256, "8 tiles: one run of 8, counted waits"), (9 * 64 - 5, 128, 256, "9 tiles: runs 8 + 1 ragged"), (16 * 64, 128, 256, "16 tiles: 2 runs of 8"),
    (17 * 64 - 63, 256, 256, "17 tiles: runs 8, 8, 1; the last tile holds one position"),
]
# out_proj: tiles never cross a sequence; a sequence's last tile is pulled back to end at L (l0 = L - 64; L = 65: l0 = 1, a one-position halo)
OUTPROJ_CASES = [
    # (B, L, Lx - L, D, norm, path)
    (1, 64, 0, 128, True, "the minimum"), (2, 65, 1, 128, True, "pulled-back tile starts at 1"), (3, 66, 3, 128, False, "pulled-back tile starts at 2: the first whole halo"),
    (5, 71, 11, 128, False, "rows at every 2-byte offset"), (9, 127, 0, 128, False, "18 tiles: runs 8, 8, 2 across sequences"), (3, 129, 1, 256, True, "9 tiles: runs 8 + 1"),
    (2, 191, 3, 256, False, "6 tiles: 6 runs of one"), (1, 7 * 64, 0, 128, False, "7 tiles"), (1, 8 * 64, 11, 128, False, "8 tiles: one run"),
    (1, 16 * 64 + 1, 0, 128, False, "17 tiles: runs 8, 8, 1, the last one pulled back over its neighbour"), (2, 8 * 64, 0, 256, False, "16 tiles, d_model 256"),
]
# dgrad: tiles never cross a sequence, the last one ragged and zero-filled; runs of 16 once there are 16 tiles, walked downwards with a warm-up tile above
DGRAD_CASES = [
    (1, 1, 128, "one position"), (2, 7, 128, "one ragged tile per sequence"), (3, 63, 128, "ragged, 3 runs of one"), (1, 64, 256, "one whole tile"),
    (2, 65, 128, "whole + one-position tile"), (3, 127, 256, "6 tiles"), (2, 130, 128, "6 tiles, piece ends inside a piece"),
    (1, 15 * 64 - 3, 128, "15 tiles: 15 runs of one"), (2, 8 * 64, 128, "16 tiles: one run of 16 across two sequences (no warm-up across the boundary)"),
    (1, 17 * 64 - 9, 128, "17 tiles: runs 16 + 1, warm-up tile above the first"), (3, 11 * 64 - 1, 128, "33 tiles: runs 16, 16, 1; boundaries inside sequences"),
]
COLSUM_CASES = [(1, 64), (7, 256), (63, 128), (64, 1024), (65, 64), (77, 256), (511, 128), (512, 64), (513, 256), (1023, 1024), (1025, 128), (1537, 64)]
XL = SL.X_LAYOUTS


def inproj_kwargs(i):
    B, Lx, Lc, D, path = INPROJ_CASES[i]
    return dict(B=B, Lx=Lx, Lc=Lc, D=D, xlayout=XL[(i + 2) % 3], rows=bool(i % 2), bias=i % 4 != 3, seed=100 + i, path=path)


def outproj_kwargs(i):
    B, L, extra, D, norm, path = OUTPROJ_CASES[i]
    return dict(B=B, L=L, Lx=L + extra, D=D, xlayout=XL[(i + 2) % 3], rows=bool((i + 1) % 2), zpacked=bool(i % 3 == 1), bias=i % 4 != 3, norm=norm,
                seed=200 + i, path=path)


def dgrad_kwargs(i):
    B, L, D, path = DGRAD_CASES[i]
    return dict(B=B, L=L, Lx=L + (0, 1, 3, 11)[i % 4], D=D, xlayout=XL[(i + 2) % 3], rows=bool((i + 1) % 2), bias=i % 4 != 3, seed=300 + i, path=path)
