"""Element-wise fp64 references and derived bounds for the operator's element-wise shell: the four channel-major kernels of
csrc/cm_kernels.h and the eight position-major ones of csrc/mixer_kernels.h, each called ON ITS OWN through the C ABI on caller-made buffers.
Shared by the emulator tests (tests/test_shell_emu.py) and the GPU tests (tests/test_gpu_shell.py).  Plain torch, device-agnostic; not a
test file.  Derivations and measured figures: profiles/shell_local.md.

Every reference starts from the stored operands the kernel read (16-bit inputs widened exactly to fp64), in channel-major orientation:
x (3D, B, Lx), y / dvg (B, D, L), dz (D, B, L).  With u = 2^-24, gamma_k = k u / (1 - k u), |.| element-wise and every bound evaluated in fp64:

    xc[c, t] = b[c] + sum_j w[c, j] (x[c, t-2+j] + bin[c])   for t-2+j >= 0            e_sc = gamma_4 (|b| + sum_j |w_j| (|x_j| + |bin|))
        (one add of bin, then three chained FMAs: the first tap passes four roundings, the bias three)
    vg = xc[2D+d] xc[D+d]       E = |c1| e_v + |c_v| e_1 + e_1 e_v + u (|c1| + e_1)(|c_v| + e_v)
    z  = y xc[d]                E = |y| e_0 + u |y| (|c0| + e_0)                         dy = dz xc[d] likewise
    da = dz y   (post_bwd)      e_da = u |da|                     da = dvg xc[other] (pre_bwd)    e_da = h + u (|da| + h),  h = |dvg| e_other
    dx[m] = w2 da[m] + w1 da[m+1] + w0 da[m+2]  (da = 0 from L on)                      E = (1 + gamma_3) convT(|w|, e_da) + gamma_3 convT(|w|, |da|)
        (one multiply and two chained FMAs behind the rounding of da)

    |got - ref64| <= E + half_ulp_io(|ref64| + E)                 at EVERY element (half_ulp_io = 0 for fp32 I/O)

The position-major kernels leave the contraction of `b + w0 x + w1 x + w2 x` to the compiler; evaluated without any FMA the first tap still passes
four roundings (its product and three sums), so the same gamma_4 / gamma_3 hold; a fused step is one rounding instead of two.

The five sums per channel -- dw0, dw1, dw2, db_sc, db_in, the host's part[..., :5].sum(1) -- are sums of terms da x_j, da and dx[m]:

    |got - ref64| <= gamma_(n + 4) (S + H) + H        S = sum |terms| with |da|, |x| + |bin|, convT(|w|, |da|);  H = the same sums with h in place of |da|

n = the worst-case depth of the additions (channel-major: 8 per thread + 6 butterfly steps + 2 across wavefronts + the records the host adds); the 4
covers the roundings inside one term (da, x + bin, the product; a dx term: four).  H is zero for post_bwd, whose terms are products of stored operands;
in pre_bwd da inherits the absolute error of a short-conv output, which no multiple of |term| covers where that output cancelled."""
import torch

U = 2.0 ** -24
CM_TILE, CM_V, CM_NP = 2048, 8, 8
MIX_T, MIX_NT, MIX_RUN = 64, 16, 1024
SENTINEL = 1536.0                       # exact in fp32 / bf16 / fp16, two orders of magnitude above any value the cases produce
_FMT = {torch.bfloat16: (7, -126), torch.float16: (10, -14)}     # explicit mantissa bits, exponent of the smallest normal
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
NAME = {torch.float32: "fp32", torch.bfloat16: "bf16", torch.float16: "fp16"}


def gamma(k):
    return k * U / (1.0 - k * U)


def half_ulp_io(x, T):
    """half the spacing of T in the binade of x >= 0 (fp64), the subnormal spacing below T's smallest normal; zero for fp32 I/O"""
    if T == torch.float32:
        return torch.zeros_like(x)
    mb, emin = _FMT[T]
    e = torch.frexp(x)[1] - 1
    e = torch.where(x == 0, torch.full_like(e, emin), e).clamp_min(emin)
    return 0.5 * torch.ldexp(torch.ones_like(x), e - mb)


# ---- the fp64 references (channel-major orientation) --------------------------------------------------------------------------------------
def _rows(t, lo, hi):
    return None if t is None else t[lo:hi]


def _taps(x, bin_):
    """x + bin behind two zero positions: [..., j:j + n] is tap j of positions 0 .. n - 1 (taps before position 0 are zero, not bin)"""
    xb = x if bin_ is None else x + bin_[:, None, None]
    return torch.nn.functional.pad(xb, (2, 0))


def sc64(x, bin_, w, b):
    """x (C, B, Lx) fp64, bin_ (C,) or None, w (C, 3), b (C,) -> xc (C, B, Lx)"""
    n = x.shape[-1]
    xp = _taps(x, bin_)
    return b[:, None, None] + sum(w[:, j, None, None] * xp[..., j:j + n] for j in range(3))


def sc_err(x, bin_, w, b):
    """the fp32 bound of sc64's value: gamma_4 times the magnitude sum"""
    return gamma(4) * sc64(x.abs(), None if bin_ is None else bin_.abs(), w.abs(), b.abs())


def convT64(w, da):
    """dx[m] = w2 da[m] + w1 da[m + 1] + w0 da[m + 2], da zero beyond its last position"""
    n = da.shape[-1]
    dp = torch.nn.functional.pad(da, (0, 2))
    return sum(w[:, 2 - j, None, None] * dp[..., j:j + n] for j in range(3))


def _convT_err(w, da, eda):
    return (1.0 + gamma(3)) * convT64(w.abs(), eda) + gamma(3) * convT64(w.abs(), da.abs())


def _sc(x, bin_, w, b, lo, hi, L):
    a = (x[lo:hi], _rows(bin_, lo, hi), w[lo:hi], b[lo:hi])
    return sc64(*a)[..., :L], sc_err(*a)[..., :L]


def _sums64(da, h, x, bin_, w, L):
    """the five sums of the channels of da (C, B, L) -> (ref (C, 5), S (C, 5), H (C, 5), smallest |term| of dw0..2 / db_sc)"""
    xp = _taps(x, bin_)[..., :L + 2]
    ap = _taps(x.abs(), None if bin_ is None else bin_.abs())[..., :L + 2]
    ref, S, H, small = [], [], [], []
    for j in range(3):
        t = da * xp[..., j:j + L]
        ref.append(t.sum((1, 2)))
        S.append((da.abs() * ap[..., j:j + L]).sum((1, 2)))
        H.append((h * ap[..., j:j + L]).sum((1, 2)))
        if L > 2 - j:
            small.append(t[..., 2 - j:].abs().min())
    ref.append(da.sum((1, 2)))
    S.append(da.abs().sum((1, 2)))
    H.append(h.sum((1, 2)))
    small.append(da.abs().min())
    ref.append(convT64(w, da).sum((1, 2)))
    S.append(convT64(w.abs(), da.abs()).sum((1, 2)))
    H.append(convT64(w.abs(), h).sum((1, 2)))
    return torch.stack(ref, 1), torch.stack(S, 1), torch.stack(H, 1), float(torch.stack(small).min())


def pre_fwd64(x, bin_, w, b, L):
    """-> vg (B, D, L), E32"""
    D = x.shape[0] // 3
    c1, e1 = _sc(x, bin_, w, b, D, 2 * D, L)
    cv, ev = _sc(x, bin_, w, b, 2 * D, 3 * D, L)
    E = c1.abs() * ev + cv.abs() * e1 + e1 * ev + U * (c1.abs() + e1) * (cv.abs() + ev)
    return (cv * c1).permute(1, 0, 2), E.permute(1, 0, 2)


def post_fwd64(x, bin_, w, b, y, L):
    """y (B, D, L) -> z (D, B, L), E32"""
    D = x.shape[0] // 3
    c0, e0 = _sc(x, bin_, w, b, 0, D, L)
    yT = y.permute(1, 0, 2)
    return yT * c0, yT.abs() * e0 + U * yT.abs() * (c0.abs() + e0)


def post_bwd64(x, bin_, w, b, y, dz, L):
    """y (B, D, L), dz (D, B, L) -> dict: dy (B, D, L), dx (D, B, L) = rows [0, D) of dxT, their E32, and the sums of channels [0, D)"""
    D = x.shape[0] // 3
    c0, e0 = _sc(x, bin_, w, b, 0, D, L)
    da = dz * y.permute(1, 0, 2)
    zero = torch.zeros_like(da)
    ref, S, H, small = _sums64(da, zero, x[:D], _rows(bin_, 0, D), w[:D], L)
    return {"dy": (dz * c0).permute(1, 0, 2), "E_dy": (dz.abs() * e0 + U * dz.abs() * (c0.abs() + e0)).permute(1, 0, 2),
            "dx": convT64(w[:D], da), "E_dx": _convT_err(w[:D], da, U * da.abs()), "sums": ref, "S": S, "H": H, "small": small}


def pre_bwd64(x, bin_, w, b, dvg, L):
    """dvg (B, D, L) -> dict: dx (2D, B, L) = rows [D, 3D) of dxT, its E32, and the sums of channels [D, 3D)"""
    D = x.shape[0] // 3
    c1, e1 = _sc(x, bin_, w, b, D, 2 * D, L)
    cv, ev = _sc(x, bin_, w, b, 2 * D, 3 * D, L)
    g = dvg.permute(1, 0, 2)
    da = torch.cat([g * cv, g * c1], 0)                                # gradient of x1c = dvg vc; of vc = dvg x1c
    h = torch.cat([g.abs() * ev, g.abs() * e1], 0)
    ref, S, H, small = _sums64(da, h, x[D:], _rows(bin_, D, 3 * D), w[D:], L)
    return {"dx": convT64(w[D:], da), "E_dx": _convT_err(w[D:], da, h + U * (da.abs() + h)), "sums": ref, "S": S, "H": H, "small": small}


def sums_bound(S, H, n):
    return gamma(n + 4) * (S + H) + H


# ---- buffers: a flat storage the test owns to the last element, and a strided logical view of it ---------------------------------------------
class Buf:
    def __init__(self, shape, strides, dtype, dev, fill):
        self.shape, self.strides = tuple(shape), tuple(strides)
        n = max(s * st for s, st in zip(self.shape, self.strides))
        self.flat = torch.full((n,), fill, dtype=dtype, device=dev)
        self.view = torch.as_strided(self.flat, self.shape, self.strides)

    @classmethod
    def input(cls, values, strides):
        """values behind `strides`, NaN in every gap"""
        b = cls(values.shape, strides, values.dtype, values.device, float("nan"))
        b.view.copy_(values)
        return b

    def untouched(self, index):
        """True if every element outside view[index] still holds the sentinel"""
        own = torch.zeros(self.flat.numel(), dtype=torch.bool, device=self.flat.device)
        torch.as_strided(own, self.shape, self.strides)[index] = True
        return bool((self.flat[~own] == SENTINEL).all())

    def same(self, other):
        """bit for bit, every element of the storage (tests/limits_local.py's FarBuf: every row and every poisoned band)"""
        return torch.equal(self.flat, other.flat)


def rows_strides(B, D, L, pitched, row_pitch, ld=None):
    """ld: the caller's own pitch (tests/limits_local.py: rows gigabytes apart)"""
    if ld is None:
        ld = row_pitch(L) if pitched else L
    return (D * ld, ld, 1), ld


def x_strides(C, B, Lx, layout, row_pitch, cs=None):
    """packed / per-sequence pitched / channel rows pitched over the flattened positions -> (strides, csx, bsx); cs: the caller's own channel
    stride over sequences Lx apart"""
    if cs is not None:
        assert cs >= B * Lx
        return (cs, Lx, 1), cs, Lx
    if layout == "packed":
        cs, bs = B * Lx, Lx
    elif layout == "seq":
        bs = row_pitch(Lx)
        cs = B * bs
    else:
        assert layout == "cm"
        cs, bs = row_pitch(B * Lx), Lx
    return (cs, bs, 1), cs, bs


def z_strides(D, B, L, rows, row_pitch):
    """zT / dzT (D, B, L): channel-major as _lib.empty_cm lays it out, or the (B, D, L) tensor of pitched rows addressed as rows (d, b)"""
    if rows:
        ld = row_pitch(L)
        return (ld, D * ld, 1), ld, D * ld
    cs = row_pitch(B * L)
    return (cs, L, 1), cs, L


def cm_rpw(B, L):
    r = 1
    while r < 8 and L * 2 * r <= CM_TILE and r * 2 <= B:
        r *= 2
    return r


def _operand(shape, g, T, dev):
    """magnitudes in [0.5, 2) with random signs (every product of stored operands stays away from zero: the reduction margin), in T"""
    v = (0.5 + 1.5 * torch.rand(shape, generator=g)) * (torch.randint(0, 2, shape, generator=g) * 2 - 1)
    return v.to(T).to(dev)


def _params(C, g, dev, bias):
    w = (torch.randn(C, 3, generator=g) * 0.5).to(dev)
    b = (torch.randn(C, generator=g) * 0.2).to(dev)
    bin_ = ((torch.rand(C, generator=g) - 0.5) * 0.5).to(dev) if bias else None
    return w, b, bin_


def _d(t):
    return None if t is None else t.double()


def _ptr(t):
    return None if t is None else t.data_ptr()


class _Stats(dict):
    def hold(self, name, got, ref, bound):
        diff = (got.double() - ref).abs()
        r = float((diff / bound.clamp_min(1e-300)).max()) if diff.numel() else 0.0
        self[name] = max(self.get(name, 0.0), r)
        assert bool((diff <= bound).all()), (name, r, int((diff > bound).sum()))

    def line(self, label):
        return f"[shell-local] {label} " + " ".join(f"{k}={v:.3g}" for k, v in self.items())


def _hold_elem(st, name, buf, index, ref, E, T):
    got = buf.view[index]
    assert bool(torch.isfinite(got).all()), name + ": not finite"
    assert buf.untouched(index), name + ": an element the contract leaves alone was written"
    st.hold(name, got, ref, E + half_ulp_io(ref.abs() + E, T))


# ---- the channel-major kernels ----------------------------------------------------------------------------------------------------------
def run_cm(_lib, dev, T, B, L, Lx, D, xlayout="packed", rows=False, zrows=False, dzrows=False, bias=True, seed=0, rpw=None, label="", lda=None,
           csx=None, rowbuf=Buf, xbuf=Buf):
    """cm_pre_fwd, cm_post_fwd, cm_post_bwd, cm_pre_bwd, each on its own on caller-made buffers: every condition of the module docstring, the
    sentinels, bitwise repeatability of the backward kernels, and the bits of the _lib wrappers on the same layouts.  Returns the figures.
    lda / csx: the caller's own row pitch of the (B, D, L) tensors / channel stride of xT and dxT, in buffers of class rowbuf / xbuf (a Buf that
    need not fill what lies between its rows: tests/limits_local.py)."""
    lib, rp = _lib.lib(), _lib.row_pitch
    code, stream = _lib.dtype_code(T), _lib._backend.stream(dev)
    g = torch.Generator().manual_seed(seed)
    w, b, bin_ = _params(3 * D, g, dev, bias)
    xs, csx, bsx = x_strides(3 * D, B, Lx, xlayout, rp, csx)
    rs, lda = rows_strides(B, D, L, rows, rp, lda)
    zs, csz, bsz = z_strides(D, B, L, zrows, rp)
    dzs, csdz, bsdz = z_strides(D, B, L, dzrows, rp)
    x = xbuf.input(_operand((3 * D, B, Lx), g, T, dev), xs)
    y = rowbuf.input(_operand((B, D, L), g, T, dev), rs)
    dvg = rowbuf.input(_operand((B, D, L), g, T, dev), rs)
    dz = Buf.input(_operand((D, B, L), g, T, dev), dzs)
    r = cm_rpw(B, L)
    assert rpw is None or r == rpw
    nrec = -(-B // r) * -(-L // CM_TILE)
    assert lib.hyena_cm_partial_floats(B, L, D) == 3 * D * nrec * CM_NP, "rows per workgroup"
    x64, w64, b64, bin64 = x.view.double(), w.double(), b.double(), _d(bin_)
    st = _Stats()
    own_l = (slice(None), slice(None), slice(0, L))

    def out(shape, strides, dtype=T):
        cls = rowbuf if strides == rs else xbuf if strides == xs else Buf
        return cls(shape, strides, dtype, dev, SENTINEL)
    with _lib._backend.guard(dev):
        # ---- forward
        vg = out((B, D, L), rs)
        _lib.check(lib.hyena_cm_pre_fwd_ld(x.flat.data_ptr(), _ptr(bin_), w.data_ptr(), b.data_ptr(), vg.flat.data_ptr(), B, L, Lx, D, csx, bsx, lda,
                                           code, stream))
        ref, E = pre_fwd64(x64, bin64, w64, b64, L)
        _hold_elem(st, "pre_fwd", vg, own_l, ref, E, T)
        zT = out((D, B, L), zs)
        _lib.check(lib.hyena_cm_post_fwd_ld(y.flat.data_ptr(), x.flat.data_ptr(), _ptr(bin_), w.data_ptr(), b.data_ptr(), zT.flat.data_ptr(), B, L, Lx, D,
                                            csx, bsx, csz, bsz, lda, code, stream))
        ref, E = post_fwd64(x64, bin64, w64, b64, y.view.double(), L)
        _hold_elem(st, "post_fwd", zT, own_l, ref, E, T)
        # the wrappers of _lib on the same caller-made layouts: the same bits (here, so that vg need not outlive the forward)
        assert torch.equal(_lib.cm_pre_fwd(x.view, bin_, w, b, L), vg.view)
        zw = _lib.cm_post_fwd(y.view, x.view, bin_, w, b, rows_out=zrows)
        assert torch.equal(zw.permute(1, 0, 2) if zrows else zw, zT.view)
        del vg, zw

        # ---- backward, each kernel twice into fresh sentinel-filled buffers
        def post_bwd():
            dy, dx, part = out((B, D, L), rs), out((3 * D, B, Lx), xs), out((3 * D, nrec, CM_NP), (nrec * CM_NP, CM_NP, 1), torch.float32)
            _lib.check(lib.hyena_cm_post_bwd_ld(dz.flat.data_ptr(), y.flat.data_ptr(), x.flat.data_ptr(), _ptr(bin_), w.data_ptr(), b.data_ptr(),
                                                dy.flat.data_ptr(), dx.flat.data_ptr(), part.flat.data_ptr(), B, L, Lx, D, csx, bsx, csdz, bsdz, lda,
                                                code, stream))
            return dy, dx, part

        def pre_bwd():
            dx, part = out((3 * D, B, Lx), xs), out((3 * D, nrec, CM_NP), (nrec * CM_NP, CM_NP, 1), torch.float32)
            _lib.check(lib.hyena_cm_pre_bwd_ld(dvg.flat.data_ptr(), x.flat.data_ptr(), _ptr(bin_), w.data_ptr(), b.data_ptr(), dx.flat.data_ptr(),
                                               part.flat.data_ptr(), B, L, Lx, D, csx, bsx, lda, code, stream))
            return dx, part
        dy, dx0, part0 = post_bwd()
        again = post_bwd()
        assert all(p.same(q) for p, q in zip((dy, dx0, part0), again)), "cm_post_bwd is not repeatable bit for bit"
        del again
        dx1, part1 = pre_bwd()
        again = pre_bwd()
        assert all(p.same(q) for p, q in zip((dx1, part1), again)), "cm_pre_bwd is not repeatable bit for bit"
        del again
        R0 = post_bwd64(x64, bin64, w64, b64, y.view.double(), dz.view.double(), L)
        R1 = pre_bwd64(x64, bin64, w64, b64, dvg.view.double(), L)
        _hold_elem(st, "post_bwd.dy", dy, own_l, R0["dy"], R0["E_dy"], T)
        _hold_elem(st, "post_bwd.dxT", dx0, (slice(0, D), slice(None), slice(0, L)), R0["dx"], R0["E_dx"], T)       # rows [D, 3D) and positions >= L: left alone
        _hold_elem(st, "pre_bwd.dxT", dx1, (slice(D, 3 * D), slice(None), slice(0, L)), R1["dx"], R1["E_dx"], T)
        n = CM_V + 6 + 2 + nrec
        for name, part, R, sl in (("post_bwd.sums", part0, R0, slice(0, D)), ("pre_bwd.sums", part1, R1, slice(D, 3 * D))):
            idx = (sl, slice(None), slice(0, 5))
            assert bool(torch.isfinite(part.view[idx]).all()) and part.untouched(idx), name + ": records"
            st.hold(name, part.view[sl, :, :5].sum(1), R["sums"], sums_bound(R["S"], R["H"], n))
        margin = float(sums_bound(R0["S"], R0["H"], n).max()) / R0["small"]
        st["margin"] = margin
        # ---- the wrappers of _lib on the same caller-made layouts: the same bits
        dxw, partw = out((3 * D, B, Lx), xs), _lib.cm_partials(x.view, L)
        assert tuple(partw.shape) == (3 * D, nrec, CM_NP)
        dyw = _lib.cm_post_bwd(dz.view.permute(1, 0, 2) if dzrows else dz.view, y.view, x.view, bin_, w, b, dxw.view, partw, dz_rows=dzrows)
        _lib.cm_pre_bwd(dvg.view, x.view, bin_, w, b, dxw.view, partw)
        assert torch.equal(dyw, dy.view) and torch.equal(dxw.view[:D], dx0.view[:D]) and torch.equal(dxw.view[D:], dx1.view[D:])
        assert dxw.untouched(own_l)
        assert torch.equal(partw[:D, :, :5], part0.view[:D, :, :5]) and torch.equal(partw[D:, :, :5], part1.view[D:, :, :5])
    print(st.line(f"{label} cm {NAME[T]} B={B} L={L} Lx={Lx} D={D} x={xlayout} rows={int(rows)} z={int(zrows)} dz={int(dzrows)} bin={int(bias)} rpw={r}"),
          flush=True)
    assert margin < 1.0, ("the bound of the sums exceeds the smallest single term: the case is too large to see a dropped term", margin)
    return st


# ---- the position-major kernels ---------------------------------------------------------------------------------------------------------
def run_pm(_lib, dev, T, B, L, Lx, D, seed=0, label=""):
    """mixer_pre_fwd / post_fwd / post_bwd / pre_bwd (narrow: one wavefront; wide when D % 64 == 0) through the same references, transposed"""
    lib = _lib.lib()
    code, stream = _lib.dtype_code(T), _lib._backend.stream(dev)
    g = torch.Generator().manual_seed(seed)
    w, b, _ = _params(3 * D, g, dev, False)
    x = _operand((B, Lx, 3 * D), g, T, dev)
    y, dvg = _operand((B, D, L), g, T, dev), _operand((B, D, L), g, T, dev)
    dz = _operand((B, L, D), g, T, dev)
    nruns = -(-L // MIX_RUN)
    assert lib.hyena_mixer_partial_floats(B, L, D) == B * nruns * 3 * D * 4
    x64, w64, b64 = x.permute(2, 0, 1).double(), w.double(), b.double()
    dz64 = dz.permute(2, 0, 1).double()
    st = _Stats()
    full = (slice(None),) * 3

    def out(shape, dtype=T):
        strides = [1]
        for s in reversed(shape[1:]):
            strides.insert(0, strides[0] * s)
        return Buf(shape, strides, dtype, dev, SENTINEL)
    with _lib._backend.guard(dev):
        vg = out((B, D, L))
        _lib.check(lib.hyena_mixer_pre_fwd(x.data_ptr(), w.data_ptr(), b.data_ptr(), vg.flat.data_ptr(), B, L, Lx, D, code, stream))
        ref, E = pre_fwd64(x64, None, w64, b64, L)
        _hold_elem(st, "pre_fwd", vg, full, ref, E, T)
        z = out((B, L, D))
        _lib.check(lib.hyena_mixer_post_fwd(y.data_ptr(), x.data_ptr(), w.data_ptr(), b.data_ptr(), z.flat.data_ptr(), B, L, Lx, D, code, stream))
        ref, E = post_fwd64(x64, None, w64, b64, y.double(), L)
        _hold_elem(st, "post_fwd", z, full, ref.permute(1, 2, 0), E.permute(1, 2, 0), T)

        def post_bwd():
            dy, dx, part = out((B, D, L)), out((B, Lx, 3 * D)), out((B, nruns, 3 * D, 4), torch.float32)
            _lib.check(lib.hyena_mixer_post_bwd(dz.data_ptr(), y.data_ptr(), x.data_ptr(), w.data_ptr(), b.data_ptr(), dy.flat.data_ptr(),
                                                dx.flat.data_ptr(), part.flat.data_ptr(), B, L, Lx, D, code, stream))
            return dy, dx, part

        def pre_bwd():
            dx, part = out((B, Lx, 3 * D)), out((B, nruns, 3 * D, 4), torch.float32)
            _lib.check(lib.hyena_mixer_pre_bwd(dvg.data_ptr(), x.data_ptr(), w.data_ptr(), b.data_ptr(), dx.flat.data_ptr(), part.flat.data_ptr(),
                                               B, L, Lx, D, code, stream))
            return dx, part
        dy, dx0, part0 = post_bwd()
        again = post_bwd()
        assert all(torch.equal(p.flat, q.flat) for p, q in zip((dy, dx0, part0), again)), "mixer_post_bwd is not repeatable bit for bit"
        dx1, part1 = pre_bwd()
        again = pre_bwd()
        assert all(torch.equal(p.flat, q.flat) for p, q in zip((dx1, part1), again)), "mixer_pre_bwd is not repeatable bit for bit"
        R0 = post_bwd64(x64, None, w64, b64, y.double(), dz64, L)
        R1 = pre_bwd64(x64, None, w64, b64, dvg.double(), L)
        _hold_elem(st, "post_bwd.dy", dy, full, R0["dy"], R0["E_dy"], T)
        _hold_elem(st, "post_bwd.dx", dx0, (slice(None), slice(0, L), slice(0, D)), R0["dx"].permute(1, 2, 0), R0["E_dx"].permute(1, 2, 0), T)
        _hold_elem(st, "pre_bwd.dx", dx1, (slice(None), slice(0, L), slice(D, 3 * D)), R1["dx"].permute(1, 2, 0), R1["E_dx"].permute(1, 2, 0), T)
        # depth of the additions: a lane of the narrow kernels walks its run's positions one by one; a thread of the wide ones adds every fourth
        # position of 16 tiles, then the four phases are added; then the host adds the records
        n = (MIX_NT * MIX_T // 4 + 3 if D % 64 == 0 else min(L, MIX_RUN)) + B * nruns
        for name, part, R, sl in (("post_bwd.sums", part0, R0, slice(0, D)), ("pre_bwd.sums", part1, R1, slice(D, 3 * D))):
            idx = (slice(None), slice(None), sl, slice(None))
            assert bool(torch.isfinite(part.view[idx]).all()) and part.untouched(idx), name + ": records"
            st.hold(name, part.view[:, :, sl].sum(dim=(0, 1)), R["sums"][:, :4], sums_bound(R["S"], R["H"], n)[:, :4])
        st["margin"] = float(sums_bound(R0["S"], R0["H"], n)[:, :4].max()) / R0["small"]
    print(st.line(f"{label} pm {'wide' if D % 64 == 0 else 'narrow'} {NAME[T]} B={B} L={L} Lx={Lx} D={D}"), flush=True)
    return st


# ---- decode_pre against cm_pre_fwd --------------------------------------------------------------------------------------------------------
def run_decode_pre(_lib, dev, T, B, D, exact, ts=(0, 1, 2, 5), seed=0, label=""):
    """decode_pre at position t, its tail taken from xT, writes into history column t what cm_pre_fwd produces at position t from the same xT:
    bit for bit (`exact`), or with at most 2e-5 of the elements on the neighbouring value of T (the allowance tests/test_gpu_proj.py grants the
    same effect of the device compiler)"""
    g = torch.Generator().manual_seed(seed)
    Lx = max(ts) + 1
    w, b, bin_ = _params(3 * D, g, dev, True)
    xT = _operand((3 * D, B, Lx), g, T, dev)
    vg = _lib.cm_pre_fwd(xT, bin_, w, b, Lx)
    lda = _lib.row_pitch(Lx)
    neq, total = 0, 0
    for t in ts:
        hist = torch.full((B, D, lda), SENTINEL, dtype=T, device=dev)
        tail = torch.full((3 * D, B, 2), float("nan"), device=dev)       # positions before 0 are never read as values
        if t >= 2:
            tail[:, :, 0] = xT[:, :, t - 2].float()
        if t >= 1:
            tail[:, :, 1] = xT[:, :, t - 1].float()
        x2 = xT[:, :, t].t().contiguous()
        x0 = torch.empty(B, D, device=dev)
        pos = torch.tensor([t], dtype=torch.int32, device=dev)
        _lib.decode_pre(x2, bin_, w, b, tail, hist, x0, pos, Lx)
        other = torch.ones(lda, dtype=torch.bool, device=dev)
        other[t] = False
        assert bool((hist[:, :, other] == SENTINEL).all())
        got, want = hist[:, :, t], vg[:, :, t]
        assert bool(torch.isfinite(got).all())
        if exact:
            assert torch.equal(got, want), (t, int((got != want).sum()))
        else:
            eps = 2.0 ** -8 if T == torch.bfloat16 else 2.0 ** -11
            assert bool(((got.float() - want.float()).abs() <= 2 * eps * want.float().abs() + 1e-7).all()), t
            neq += int((got != want).sum())
        total += got.numel()
    print(f"[shell-local] {label} decode_pre {NAME[T]} B={B} D={D} differing={neq}/{total}", flush=True)
    assert neq <= 2e-5 * total, (neq, total)


# ---- the cases ------------------------------------------------------------------------------------------------------------------------------
CM_LENGTHS = [1, 2, 3, 7, 8, 9, 17, 1023, 1024, 1025, 2047, 2048, 2049, 2050, 4097]
CM_EXTRA = [0, 1, 2, 3, 11]                                     # Lx - L: the truncated operator
CM_RPW = [(1, 300, 1), (3, 1024, 2), (5, 512, 4), (9, 257, 4), (19, 128, 8), (9, 255, 8)]          # (B, L, rows per workgroup); ragged last groups
X_LAYOUTS = ["packed", "seq", "cm"]
PM_LENGTHS = [1, 2, 3, 63, 64, 65, 66, 1023, 1024, 1025, 1026, 2049]
PM_EXTRA = [0, 1, 3]
PM_NARROW, PM_WIDE = [1, 3, 65, 70], [64, 128]


def cm_length_cases(L):
    """every Lx - L at one length; the layouts, the batch size, the channel count and the bias cycle so that every length meets every x layout,
    both row layouts, both layouts of zT and of dzT, and bin_ = None"""
    i = CM_LENGTHS.index(L)
    for k, extra in enumerate(CM_EXTRA):
        j = i + k
        yield dict(B=1 + j % 3, L=L, Lx=L + extra, D=1 + (j // 2) % 3, xlayout=X_LAYOUTS[j % 3], rows=bool((j + k) % 2), zrows=bool((j // 2) % 2),
                   dzrows=bool((j // 3) % 2), bias=(j % 4 != 3), seed=1000 * L + extra)


def pm_cases(D, L):
    i = PM_LENGTHS.index(L)
    for k, extra in enumerate(PM_EXTRA):
        B = 3 if (i + k) % 2 and 3 * (L + extra) * 3 * D <= 1 << 20 else 1
        yield dict(B=B, L=L, Lx=L + extra, D=D, seed=1000 * L + 10 * D + extra)
