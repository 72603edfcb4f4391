"""Element-wise fp64 references and derived bounds for the residual glue of a block, csrc/block_kernels.h: add_norm_fwd / add_norm_bwd (plain and
embedding-gathering), the np = 3 column sums of dx0, and the pooled readout (add_norm_pool_fwd / _finish / _bwd), each called ON ITS OWN through the
C ABI on caller-made buffers.  Shared by the emulator tests (tests/test_block_local_emu.py) and the GPU tests (tests/test_gpu_block_local.py).
Plain torch, device-agnostic; not a test file.  Derivations, measured figures and mutants: profiles/block_local.md.

Every reference starts from the stored operands (16-bit inputs widened exactly to fp64; keep_scale, eps, and the dropout threshold as the C ABI
forms them from a float p).  Notation of tests/shell_local.py: u = 2^-24, gamma_k = k u / (1 - k u), |.| element-wise, every bound evaluated in
fp64.  A lane holds E = D / 64 channels; a row statistic is E sequential adds and 6 butterfly steps, then a product with 1 / D (exact: D is a
power of two).  sqrtf and the division are correctly rounded under build.py's flags (no fast-math; hipcc's default
-fhip-fp32-correctly-rounded-divide-sqrt): half an ulp each.  Contraction to FMA only removes roundings.

Forward  (c_r = roundings of r: one for keep_scale, one for the residual add)
    r    = keep * scale * x0 + residual                e_r  = gamma_(c_r) (|keep scale x0| + |residual|)                 -> res_out
    mean = sum r / D                                   e_m  = (gamma_(E+6) sum(|r| + e_r) + sum e_r) / D
    d    = r - mean                                    e_d  = e_r + e_m + u (|d| + e_r + e_m)
    a    = sum d^2 / D + eps                           e_a  = e_v + u (a + e_v),   e_v = ((1 + gamma_(E+7)) sum(2 |d| e_d + e_d^2) + gamma_(E+7) sum d^2) / D
    rstd = 1 / sqrt(a)                                 e_s  = rstd ((1 - e_a / a)^(-1/2) (1 + u) / (1 - u) - 1)
    xh   = d rstd                                      e_xh = P + u (|xh| + P),    P = |d| e_s + rstd e_d + e_d e_s
    out  = xh w + b                                    E    = |w| e_xh + gamma_2 (|w| (|xh| + e_xh) + |b|)
  The error of mean enters out as the ABSOLUTE term rstd |w| e_m (through e_d): no multiple of |out| covers it where r - mean cancels.

Backward, from the STORED mean, rstd, saved (general form; the plain kernel has gw = g w, e_gw = u |gw|, e_xh = gamma_2 |xh|)
    s1 = sum gw / D                                    e_s1 = ((1 + gamma_(E+6)) sum e_gw + gamma_(E+6) sum |gw|) / D
    s2 = sum gw xh / D                                 e_s2 = ((1 + gamma_(E+7)) sum T + gamma_(E+7) sum |gw xh|) / D,   T = |gw| e_xh + |xh| e_gw + e_gw e_xh
    A  = gw - s1 - xh s2                               e_A  = (1 + gamma_3) (e_gw + e_s1 + |xh| e_s2 + |s2| e_xh + e_xh e_s2) + gamma_3 (|gw| + |s1| + |xh s2|)
    dr = rstd A + h                                    E    = (1 + gamma_2) rstd e_A + gamma_2 rstd |A| + u |h|           -> d_residual
    dx0 = keep * scale * dr                            E_dx = scale E + u scale (|dr| + E)   (exactly zero where dropped)
The pooled backward rebuilds r in fp32 (e_r as above, so e_xh = (1 + gamma_2) rstd e_r + gamma_2 |xh|), forms gv = fl(fl(1 / n) g) (gamma_2) and
gw = fl(gv w) (gamma_3), and has no h.

    |got - ref64| <= E + half_ulp_io(|ref64| + E)                 at EVERY element (half_ulp_io = 0 for fp32 outputs)

Sums: |got - ref64| <= gamma_(n + c) (S + H) + H, S = sum |terms|, H = sum of the terms' inherited absolute errors, n the worst-case depth of the
additions (rows of a wavefront, + 4 across the wavefronts, + ceil(slots / 16) + 16 in filter_reduce_multi_kernel / the finish kernel), c the roundings
inside a term: dweight g xh: 3, H = 0; dbias g: 0; column sums of the dx0 AS STORED: 0 (the reference sums the kernel's own dx0, which is held on its
own); d_table: 0, H = sum E_dx; pooled: 1 (the division by n), H = sum E_out; pooled dweight gv xh: 3, H = sum |gv| e_xh; pooled dbias: 3.
The operands are drawn so that every sum's bound stays below its smallest non-zero term (`margin`, asserted): a dropped or doubled row cannot hide."""
import ctypes

import torch

from tests.shell_local import DTYPES, NAME, SENTINEL, U, gamma, half_ulp_io  # noqa: F401

BLK_WAVES, BLK_MAX_GRID, BLK_VMAX = 4, 2048, 16
EPS = 1e-5
SEED = 0x0123_4567_89AB_CDEF
_M32 = 0xFFFFFFFF
NAN = float("nan")
BAD_ID = 1 << 40                                   # what the guards of `ids` hold


def f32(x):
    """the value a C float parameter receives"""
    return ctypes.c_float(x).value


def dropout_params(p):
    """(threshold, keep_scale as fp64) as blk_set_dropout forms them from the float p of the C ABI"""
    pf = f32(p)
    return int(pf * 4294967296.0), f32(1.0 / (1.0 - pf))


# ---- Philox 4x32-10 from (seed, linear index), vectorised in int64 ---------------------------------------------------------------------------
def _mulhilo(a, b):
    """a: 32-bit constant, b: int64 tensor of 32-bit values -> (hi, lo) of the 64-bit product, without leaving the positive int64 range"""
    t = a * (b & 0xFFFF)
    s = a * (b >> 16)
    low = t + ((s & 0xFFFF) << 16)
    return (s >> 16) + (low >> 32), low & _M32


def philox_words(seed, n, dev):
    """the 32 random bits of elements 0 .. n - 1: word i & 3 of Philox4x32-10(counter (i >> 2, 0, 0, 0), key seed); n < 2^34"""
    assert n < 1 << 34
    c = torch.arange((n + 3) // 4, dtype=torch.int64, device=dev)
    x0, x1, x2, x3 = c & _M32, c >> 32, torch.zeros_like(c), torch.zeros_like(c)
    k0, k1 = seed & _M32, (seed >> 32) & _M32
    for _ in range(10):
        h0, l0 = _mulhilo(0xD2511F53, x0)
        h1, l1 = _mulhilo(0xCD9E8D57, x2)
        x0, x1, x2, x3 = h1 ^ x1 ^ k0, l1, h0 ^ x3 ^ k1, l0
        k0, k1 = (k0 + 0x9E3779B9) & _M32, (k1 + 0xBB67AE85) & _M32
    return torch.stack([x0, x1, x2, x3], 1).reshape(-1)[:n]


def keep_mask(p, shape, dev):
    """(keep as fp64 0 / 1, keep_scale); (None, 1.0) without dropout"""
    if p == 0.0:
        return None, 1.0
    thr, ks = dropout_params(p)
    n = 1
    for s in shape:
        n *= s
    return (philox_words(SEED, n, dev) >= thr).double().reshape(shape), ks


# ---- the fp64 references ------------------------------------------------------------------------------------------------------------------
def fwd64(x0, res, w, b, keep, ks, eps=None):
    """x0 (..., D) fp64, res or None, keep or None -> dict of references and bounds of add_norm_fwd_kernel's values"""
    eps = f32(EPS) if eps is None else eps
    D = x0.shape[-1]
    E = D // 64
    kx = x0 if keep is None else keep * ks * x0
    r = kx if res is None else kx + res
    c_r = (keep is not None) + (res is not None)
    e_r = gamma(c_r) * (kx.abs() + (0 if res is None else res.abs())) if c_r else torch.zeros_like(r)
    mean = r.mean(-1, keepdim=True)
    e_m = (gamma(E + 6) * (r.abs() + e_r).sum(-1, keepdim=True) + e_r.sum(-1, keepdim=True)) / D
    d = r - mean
    e_d = e_r + e_m + U * (d.abs() + e_r + e_m)
    a = (d * d).mean(-1, keepdim=True) + eps
    e_v = ((1 + gamma(E + 7)) * (2 * d.abs() * e_d + e_d * e_d).sum(-1, keepdim=True) + gamma(E + 7) * (d * d).sum(-1, keepdim=True)) / D
    e_a = e_v + U * (a + e_v)
    assert bool((e_a < a).all())
    rstd = a.rsqrt()
    e_s = rstd * ((1 - e_a / a) ** -0.5 * (1 + U) / (1 - U) - 1)
    xh = d * rstd
    P = d.abs() * e_s + rstd * e_d + e_d * e_s
    e_xh = P + U * (xh.abs() + P)
    out = xh * w + b
    E_out = w.abs() * e_xh + gamma(2) * (w.abs() * (xh.abs() + e_xh) + b.abs())
    return {"r": r, "e_r": e_r, "mean": mean.squeeze(-1), "e_m": e_m.squeeze(-1), "rstd": rstd.squeeze(-1), "e_s": e_s.squeeze(-1),
            "out": out, "E_out": E_out}


def _dr64(gw, e_gw, xh, e_xh, rstd, h):
    """rstd (gw - s1 - xh s2) + h and its fp32 bound; rstd (..., 1)"""
    D = gw.shape[-1]
    E = D // 64
    s1 = gw.mean(-1, keepdim=True)
    e_s1 = ((1 + gamma(E + 6)) * e_gw.sum(-1, keepdim=True) + gamma(E + 6) * gw.abs().sum(-1, keepdim=True)) / D
    s2 = (gw * xh).mean(-1, keepdim=True)
    T = gw.abs() * e_xh + xh.abs() * e_gw + e_gw * e_xh
    e_s2 = ((1 + gamma(E + 7)) * T.sum(-1, keepdim=True) + gamma(E + 7) * (gw * xh).abs().sum(-1, keepdim=True)) / D
    A = gw - s1 - xh * s2
    e_A = (1 + gamma(3)) * (e_gw + e_s1 + xh.abs() * e_s2 + s2.abs() * e_xh + e_xh * e_s2) + gamma(3) * (gw.abs() + s1.abs() + (xh * s2).abs())
    dr = rstd * A
    E_dr = (1 + gamma(2)) * rstd * e_A + gamma(2) * dr.abs()
    if h is not None:
        dr, E_dr = dr + h, E_dr + U * h.abs()
    return dr, E_dr


def _mask64(dr, E_dr, keep, ks):
    if keep is None:
        return dr, E_dr
    return keep * ks * dr, keep * (ks * E_dr + U * ks * (dr.abs() + E_dr))


def bwd64(g, saved, mean, rstd, w, h, keep, ks):
    """add_norm_bwd_kernel from the stored operands: g (rows, D), saved, mean / rstd (rows,), h or None -> references, bounds, and the terms of the sums"""
    xh = (saved - mean[:, None]) * rstd[:, None]
    gw = g * w
    dr, E_dr = _dr64(gw, U * gw.abs(), xh, gamma(2) * xh.abs(), rstd[:, None], h)
    dx, E_dx = _mask64(dr, E_dr, keep, ks)
    return {"dr": dr, "E_dr": E_dr, "dx": dx, "E_dx": E_dx, "t_dw": g * xh, "t_db": g}


def pool_fwd64(x0, res, w, b, keep, ks, n, mode):
    """x0 (B, L, D), n (B,) clamped lengths (int64) -> fwd64's dict + pooled (B, D), its S and H"""
    B, L, D = x0.shape
    R = fwd64(x0, res, w, b, keep, ks)
    valid = (torch.arange(L, device=x0.device)[None, :] < n[:, None]).double()[..., None]
    scale = torch.where(n > 0, 1.0 / n.clamp_min(1).double(), torch.zeros_like(n, dtype=torch.float64)) if mode == "mean" else torch.ones_like(n, dtype=torch.float64)
    sc = scale[:, None]
    R.update(valid=valid, scale=scale, pooled=sc * (valid * R["out"]).sum(1), S=sc * (valid * R["out"].abs()).sum(1), H=sc * (valid * R["E_out"]).sum(1))
    return R


def pool_bwd64(g, x0, res, mean, rstd, w, keep, ks, n, mode):
    """add_norm_pool_bwd_kernel from the stored x0, residual, mean, rstd (B, L), g (B, D).  Pad rows: NaN-free zeros (the inputs may hold NaN there)."""
    B, L, D = x0.shape
    valid = torch.arange(L, device=x0.device)[None, :] < n[:, None]
    v3 = valid[..., None]
    z = torch.zeros((), dtype=torch.float64, device=x0.device)
    kx = x0 if keep is None else keep * ks * x0
    r = kx if res is None else kx + res
    c_r = (keep is not None) + (res is not None)
    e_r = gamma(c_r) * (kx.abs() + (0 if res is None else res.abs())) if c_r else torch.zeros_like(r)
    r, e_r = torch.where(v3, r, z), torch.where(v3, e_r, z)
    mean, rstd = torch.where(valid, mean, z)[..., None], torch.where(valid, rstd, z)[..., None]
    xh = (r - mean) * rstd
    e_xh = (1 + gamma(2)) * rstd * e_r + gamma(2) * xh.abs()
    scale = torch.where(n > 0, 1.0 / n.clamp_min(1).double(), torch.zeros_like(n, dtype=torch.float64)) if mode == "mean" else torch.ones_like(n, dtype=torch.float64)
    gv = (scale[:, None] * g)[:, None, :]
    gw = (gv * w).expand(B, L, D)
    dr, E_dr = _dr64(gw, gamma(3) * gw.abs(), xh, e_xh, rstd, None)
    dr, E_dr = torch.where(v3, dr, z), torch.where(v3, E_dr, z)
    dx, E_dx = _mask64(dr, E_dr, keep, ks)
    vd = v3.double()
    return {"dr": dr, "E_dr": E_dr, "dx": dx, "E_dx": E_dx, "valid": valid, "t_dw": vd * gv * xh, "H_dw": vd * gv.abs() * e_xh, "t_db": vd * gv.expand(B, L, D)}


def sum_bound(S, H, n, c):
    return gamma(n + c) * (S + H) + H


def blk_grid(rows):
    return min(-(-rows // BLK_WAVES), BLK_MAX_GRID)


def red_depth(slots):
    """filter_reduce_multi_kernel / add_norm_pool_finish_kernel over `slots` partial rows: a thread row adds every 16th, thread row 0 the 16 slices"""
    return -(-slots // 16) + 16


def blk_depth(rows):
    """additions behind one element of dweight / dbias / colsum / d_table: the rows of a wavefront, the 4 wavefronts, the reduction over the workgroups"""
    g = blk_grid(rows)
    return -(-rows // (BLK_WAVES * g)) + BLK_WAVES + red_depth(g)


def pool_chunk_rows(B, L):
    """csrc/fftconv.hip pool_chunk_rows: at most BLK_MAX_GRID workgroups over the batch, a multiple of BLK_WAVES rows each"""
    cap = max(BLK_MAX_GRID // B, 1)
    return -(-(-(-L // cap)) // BLK_WAVES) * BLK_WAVES


def pool_chunks(B, L):
    return -(-L // pool_chunk_rows(B, L))


# ---- buffers the test owns to the last element: one guard row before and after ---------------------------------------------------------------
class Guarded:
    def __init__(self, shape, dtype, dev, fill, guard=None):
        shape = tuple(shape)
        self.g = guard if guard is not None else (shape[-1] if len(shape) > 1 else 16)
        self.n = 1
        for s in shape:
            self.n *= s
        self.flat = torch.full((self.n + 2 * self.g,), fill, dtype=dtype, device=dev)
        self.t = self.flat[self.g:self.g + self.n].view(shape)

    @classmethod
    def input(cls, values, guard_fill=NAN):
        b = cls(values.shape, values.dtype, values.device, guard_fill)
        b.t.copy_(values)
        return b

    @property
    def ptr(self):
        return self.t.data_ptr()

    def guards_intact(self):
        return bool((self.flat[:self.g] == SENTINEL).all()) and bool((self.flat[self.g + self.n:] == SENTINEL).all())


def _out(shape, dtype, dev, guard=None):
    return Guarded(shape, dtype, dev, SENTINEL, guard)


def _p(b):
    return None if b is None else b.ptr


class _Stats(dict):
    def hold(self, name, got, ref, bound):
        assert bool(torch.isfinite(got).all()), name + ": not finite"
        diff = (got.double() - ref).abs()
        r = float((diff / bound.clamp_min(1e-300)).max()) if diff.numel() else 0.0
        self[name] = max(self.get(name, 0.0), r)
        assert bool((diff <= bound).all()), (name, r, int((diff > bound).sum()))

    def elem(self, name, buf, ref, E, T):
        assert buf.guards_intact(), name + ": a guard row was written"
        self.hold(name, buf.t, ref, E + half_ulp_io(ref.abs() + E, T))

    def total(self, name, buf, terms, H, n, c, dims=0):
        """a sum over `dims` of `terms`: the bound, and the margin of the bound to the smallest non-zero |term| of the same sum"""
        assert buf.guards_intact(), name + ": a guard row was written"
        S = terms.abs().sum(dims)
        Hs = torch.zeros_like(S) if H is None else H.sum(dims)
        bound = sum_bound(S, Hs, n, c)
        self.hold(name, buf.t, terms.sum(dims), bound)
        small = torch.where(terms != 0, terms.abs(), torch.full_like(terms, float("inf"))).amin(dims)
        m = float((bound / small).max())
        self["margin"] = max(self.get("margin", 0.0), m)

    def line(self, label):
        return f"[block-local] {label} " + " ".join(f"{k}={v:.3g}" for k, v in self.items())


def _same(a, b):
    """bit for bit, guards included"""
    return all(torch.equal(p.flat, q.flat) for p, q in zip(a, b) if p is not None)


# ---- operand draws -------------------------------------------------------------------------------------------------------------------------
def _mag(shape, g, lo=1.0):
    return lo * (1.0 + torch.rand(shape, generator=g, dtype=torch.float64))


def _sign(shape, g):
    return (torch.randint(0, 2, shape, generator=g) * 2 - 1).double()


def _order(lead, D, g):
    """a random channel order per row: channel -> its place in the order"""
    return torch.rand(tuple(lead) + (D,), generator=g).argsort(-1).argsort(-1)


def _quads(lead, D, g, idx=None):
    """over a random channel order (the row's own, or `idx`), groups of four channels that share one magnitude a in [1, 2) and one q in [1, 2), with
    signs tau = (+ - + -) and sigma = (+ + - -): sum tau a = sum sigma q = sum sigma q tau a = 0 over a row, whatever the magnitudes"""
    lead = tuple(lead)
    idx = _order(lead, D, g) if idx is None else idx.expand(lead + (D,)).contiguous()
    quad = idx // 4
    a = torch.gather(_mag(lead + (D // 4,), g), -1, quad)
    q = torch.gather(_mag(lead + (D // 4,), g), -1, quad)
    tau = 1.0 - 2.0 * (idx % 2).double()
    sigma = 1.0 - 2.0 * ((idx // 2) % 2).double()
    return a, tau, q, sigma


def draw_rows(lead, D, g, amp=1.0, idx=None):
    """values c + tau a amp with a row constant c in +-[1/8, 1/4) (amp = 1) or +-[2, 4) (amp = 2: dropout without a residual, where a dropped
    element sits at 0 and must stay away from the row mean ~ c): every |value - row mean| >= amp, and the mean is not zero"""
    a, tau, q, sigma = _quads(lead, D, g, idx)
    c = _sign(tuple(lead) + (1,), g) * _mag(tuple(lead) + (1,), g, 0.125) * (1.0 if amp <= 1.0 else 8.0 * amp)
    return c + tau * a * amp, tau, q, sigma


def draw_gw(tau, q, sigma, g, lead):
    """gw = sigma q + alpha + beta tau: s1 = alpha, s2 ~ beta, and |gw - s1 - xh s2| stays near q >= 1"""
    alpha = _sign(tuple(lead) + (1,), g) * _mag(tuple(lead) + (1,), g, 0.125)
    beta = _sign(tuple(lead) + (1,), g) * _mag(tuple(lead) + (1,), g, 0.125)
    return sigma * q + alpha + beta * tau


def draw_params(D, g, dev):
    w = (_sign((D,), g) * _mag((D,), g)).float().to(dev)
    b = (_sign((D,), g) * _mag((D,), g, 0.05)).float().to(dev)
    return w, b


def draw_forward(lead, D, T, with_res, p, g, dev, idx=None):
    """x0 (T) and residual (fp32) whose r = dropout(x0) + residual keeps every |r - mean| away from zero"""
    lead = tuple(lead)
    if with_res:
        res = draw_rows(lead, D, g, idx=idx)[0]
        x0 = (_sign(lead + (D,), g) * _mag(lead + (D,), g, 1.0 / 16)).to(T)
        return x0.to(dev), res.float().to(dev)
    return draw_rows(lead, D, g, amp=1.0 if p == 0.0 else 2.0, idx=idx)[0].to(T).to(dev), None


# ---- add_norm_fwd / add_norm_bwd ---------------------------------------------------------------------------------------------------------
def _seed(dev, p):
    return torch.tensor([SEED], dtype=torch.int64, device=dev) if p > 0.0 else None


def run_add_norm(_lib, dev, rows, D, XT, OT, with_res, p, np_, seed=0, label="", wrappers=True):
    """add_norm_fwd_kernel<XT, OT> and add_norm_bwd_kernel<OT, XT> (dout has the forward's out type, dx0 its x0 type) on caller-made buffers"""
    lib, code, stream = _lib.lib(), _lib.dtype_code, _lib._backend.stream(dev)
    g = torch.Generator().manual_seed(seed)
    w, b = draw_params(D, g, dev)
    x0, res = draw_forward((rows,), D, XT, with_res, p, g, dev)
    keep, ks = keep_mask(p, (rows, D), dev)
    sd = _seed(dev, p)
    wb, bb = Guarded.input(w), Guarded.input(b)
    st = _Stats()
    with _lib._backend.guard(dev):
        # ---- forward
        xb, rb = Guarded.input(x0), None if res is None else Guarded.input(res)

        def fwd():
            o = (_out((rows, D), OT, dev), _out((rows, D), torch.float32, dev), _out((rows,), torch.float32, dev), _out((rows,), torch.float32, dev))
            _lib.check(lib.hyena_dropout_add_norm_fwd(xb.ptr, code(XT), _p(rb), wb.ptr, bb.ptr, EPS, p, None if sd is None else sd.data_ptr(), o[0].ptr, code(OT),
                                                      o[1].ptr, o[2].ptr, o[3].ptr, rows, D, stream))
            return o
        out, ro, mean, rstd = fwd()
        assert _same((out, ro, mean, rstd), fwd()), "add_norm_fwd is not repeatable bit for bit"
        R = fwd64(x0.double(), None if res is None else res.double(), w.double(), b.double(), keep, ks)
        st.elem("res_out", ro, R["r"], R["e_r"], torch.float32)
        st.elem("mean", mean, R["mean"], R["e_m"], torch.float32)
        st.elem("rstd", rstd, R["rstd"], R["e_s"], torch.float32)
        st.elem("out", out, R["out"], R["E_out"], OT)
        if wrappers:
            ow = _lib.add_norm_fwd(x0, res, w, b, EPS, OT, dropout_p=p, seed=sd)
            assert all(torch.equal(a_, b_.t) for a_, b_ in zip(ow, (out, ro, mean, rstd))), "the wrapper's bits"
        # ---- backward: caller-made saved, mean, rstd (the fp64 values rounded once), dout of type OT, dx0 of type XT
        sv64, tau, q, sigma = draw_rows((rows,), D, g)
        saved = sv64.float().to(dev)
        s64 = saved.double()
        mu = s64.mean(-1).float()
        rs = ((s64 - s64.mean(-1, keepdim=True)) ** 2).mean(-1).add(f32(EPS)).rsqrt().float()
        dout = (draw_gw(tau, q, sigma, g, (rows,)).to(dev) / w.double()).to(OT)
        h = (sigma * _mag((rows, D), g, 0.5)).float().to(dev) if with_res else None             # the sign of the leading term of dr: no cancellation
        gb, sb, mb, sb2, hb = Guarded.input(dout), Guarded.input(saved), Guarded.input(mu), Guarded.input(rs), None if h is None else Guarded.input(h)
        grid = blk_grid(rows)
        nf = lib.hyena_add_norm_partial_floats(rows, D)
        assert nf == grid * 3 * D

        def bwd():
            o = (_out((rows, D), XT, dev), _out((rows, D), torch.float32, dev) if with_res else None, _out((D,), torch.float32, dev),
                 _out((D,), torch.float32, dev), _out((D,), torch.float32, dev) if np_ == 3 else None, _out((nf,), torch.float32, dev, D))
            _lib.check(lib.hyena_dropout_add_norm_bwd_colsum(gb.ptr, code(OT), _p(hb), sb.ptr, wb.ptr, mb.ptr, sb2.ptr, p, None if sd is None else sd.data_ptr(),
                                                             o[0].ptr, code(XT), _p(o[1]), o[2].ptr, o[3].ptr, _p(o[4]), o[5].ptr, rows, D, stream))
            return o
        dx, dres, dw, db, cs, part = bwd()
        assert _same((dx, dres, dw, db, cs, part), bwd()), "add_norm_bwd is not repeatable bit for bit"
        assert part.guards_intact(), "partials: a guard row was written"
        Rb = bwd64(dout.double(), s64, mu.double(), rs.double(), w.double(), None if h is None else h.double(), keep, ks)
        if dres is not None:
            st.elem("d_residual", dres, Rb["dr"], Rb["E_dr"], torch.float32)
        st.elem("dx0", dx, Rb["dx"], Rb["E_dx"], XT)
        n = blk_depth(rows)
        st.total("dweight", dw, Rb["t_dw"], None, n, 3)
        st.total("dbias", db, Rb["t_db"], None, n, 0)
        if cs is not None:
            st.total("colsum", cs, dx.t.double(), None, n, 0)
        if wrappers:
            from hyena_dna_amd import _gradsum
            was = _gradsum.ENABLED
            bw = _lib.add_norm_bwd(dout, h, saved, w, mu, rs, XT, need_dres=with_res, dropout_p=p, seed=sd, offer_colsum=False)
            assert _gradsum.ENABLED == was
            assert torch.equal(bw[0], dx.t) and (dres is None or torch.equal(bw[1], dres.t)) and torch.equal(bw[2], dw.t) and torch.equal(bw[3], db.t)
    print(st.line(f"{label} add_norm {NAME[XT]}->{NAME[OT]} rows={rows} D={D} res={int(with_res)} p={p} np={np_}"), flush=True)
    assert st["margin"] < 1.0, ("the bound of a sum exceeds its smallest term: the case is too large to see a dropped term", st["margin"])
    return st


# ---- the embedding-gathering forms -------------------------------------------------------------------------------------------------------
def draw_ids(rows, V, g, empty=True):
    """ids in [0, V) that leave some classes empty (V > 2: the odd classes above 2 never occur)"""
    ids = torch.randint(0, V, (rows,), generator=g)
    if empty and V > 2:
        ids = torch.where((ids % 2 == 1) & (ids > 2), ids - 1, ids)
    return ids


def emb_bwd_ref(dout, saved, mu, rs, w, h, keep, ks, ids, V, live=None):
    """references of embed_add_norm_bwd over the rows `live` (all by default) -> (Rb, class one-hot (rows, V))"""
    Rb = bwd64(dout.double(), saved.double(), mu.double(), rs.double(), w.double(), None if h is None else h.double(), keep, ks)
    onehot = (ids[:, None] == torch.arange(V, device=ids.device)[None, :]).double()
    if live is not None:
        onehot = onehot * live[:, None].double()
    return Rb, onehot


def hold_emb_bwd(st, rows, D, V, Rb, onehot, dt, dw, db, live=None):
    n = blk_depth(rows)
    lv = torch.ones(rows, dtype=torch.float64, device=onehot.device) if live is None else live.double()
    z = torch.zeros((), dtype=torch.float64, device=onehot.device)
    sel = lv[:, None] > 0
    st.total("dweight", dw, torch.where(sel, Rb["t_dw"], z), None, n, 3)
    st.total("dbias", db, torch.where(sel, Rb["t_db"], z), None, n, 0)
    terms = onehot[:, :, None] * torch.where(sel, Rb["dx"], z)[:, None, :]                   # (rows, V, D)
    H = onehot[:, :, None] * torch.where(sel, Rb["E_dx"], z)[:, None, :]
    assert bool((dt.flat[dt.g + V * D:dt.g + dt.n] == SENTINEL).all()), "d_table: rows [V, 16) were written"
    assert dt.guards_intact(), "d_table: a guard row was written"
    S, Hs = terms.abs().sum(0), H.sum(0)
    bound = sum_bound(S, Hs, n, 0)
    st.hold("d_table", dt.t[:V], terms.sum(0), bound)
    small = torch.where(terms != 0, terms.abs(), torch.full_like(terms, float("inf"))).amin(0)
    st["margin"] = max(st.get("margin", 0.0), float((bound / small).max()))


def run_embed(_lib, dev, rows, D, V, OT, p, seed=0, label="", wrappers=True):
    """add_norm_fwd_kernel<fp32, OT, E, EMB> and add_norm_bwd_kernel<OT, fp32, E, EMB>: x0 = table[ids], d_table the per-class sums of dx0 before rounding"""
    lib, code, stream = _lib.lib(), _lib.dtype_code, _lib._backend.stream(dev)
    g = torch.Generator().manual_seed(seed)
    w, b = draw_params(D, g, dev)
    ids = draw_ids(rows, V, g).to(dev)
    tv, _, _, _ = draw_rows((V,), D, g, amp=1.0 if p == 0.0 else 2.0)
    table = Guarded((BLK_VMAX, D), torch.float32, dev, NAN)                                    # rows [V, 16) and the guards: NaN
    table.t[:V] = tv.float().to(dev)
    keep, ks = keep_mask(p, (rows, D), dev)
    sd = _seed(dev, p)
    sdp = None if sd is None else sd.data_ptr()
    wb, bb, ib = Guarded.input(w), Guarded.input(b), Guarded.input(ids, BAD_ID)
    st = _Stats()
    with _lib._backend.guard(dev):
        def fwd():
            o = (_out((rows, D), OT, dev), _out((rows, D), torch.float32, dev), _out((rows,), torch.float32, dev), _out((rows,), torch.float32, dev))
            _lib.check(lib.hyena_embed_add_norm_fwd(ib.ptr, table.ptr, V, wb.ptr, bb.ptr, EPS, p, sdp, o[0].ptr, code(OT), o[1].ptr, o[2].ptr, o[3].ptr,
                                                    rows, D, stream))
            return o
        out, ro, mean, rstd = fwd()
        assert _same((out, ro, mean, rstd), fwd()), "embed_add_norm_fwd is not repeatable bit for bit"
        R = fwd64(table.t[:V].double()[ids], None, w.double(), b.double(), keep, ks)
        st.elem("res_out", ro, R["r"], R["e_r"], torch.float32)
        st.elem("mean", mean, R["mean"], R["e_m"], torch.float32)
        st.elem("rstd", rstd, R["rstd"], R["e_s"], torch.float32)
        st.elem("out", out, R["out"], R["E_out"], OT)
        if wrappers:
            ow = _lib.embed_add_norm_fwd(ids, table.t[:V], w, b, EPS, OT, dropout_p=p, seed=sd)
            assert all(torch.equal(a_, b_.t) for a_, b_ in zip(ow, (out, ro, mean, rstd))), "the wrapper's bits"
        # ---- backward on caller-made saved / mean / rstd; with and without the gradient of residual' by the parity of the seed
        sv64, tau, q, sigma = draw_rows((rows,), D, g)
        saved = sv64.float().to(dev)
        s64 = saved.double()
        mu = s64.mean(-1).float()
        rs = ((s64 - s64.mean(-1, keepdim=True)) ** 2).mean(-1).add(f32(EPS)).rsqrt().float()
        dout = (draw_gw(tau, q, sigma, g, (rows,)).to(dev) / w.double()).to(OT)
        h = (sigma * _mag((rows, D), g, 0.5)).float().to(dev) if seed % 2 == 0 else None
        bufs = (Guarded.input(dout), None if h is None else Guarded.input(h), Guarded.input(saved), Guarded.input(mu), Guarded.input(rs))
        dt, dw, db, part = emb_bwd_call(_lib, dev, bufs, ib, wb, V, OT, p, sdp, rows, D)
        assert _same((dt, dw, db, part), emb_bwd_call(_lib, dev, bufs, ib, wb, V, OT, p, sdp, rows, D)), "embed_add_norm_bwd is not repeatable bit for bit"
        Rb, onehot = emb_bwd_ref(dout, saved, mu, rs, w, h, keep, ks, ids, V)
        hold_emb_bwd(st, rows, D, V, Rb, onehot, dt, dw, db)
        if wrappers:
            bw = _lib.embed_add_norm_bwd(dout, h, saved, ids, V, w, mu, rs, dropout_p=p, seed=sd)
            assert torch.equal(bw[0], dt.t[:V]) and torch.equal(bw[1], dw.t) and torch.equal(bw[2], db.t)
    print(st.line(f"{label} embed {NAME[OT]} rows={rows} D={D} V={V} p={p} h={int(h is not None)}"), flush=True)
    assert st["margin"] < 1.0, st["margin"]
    return st, (dt, dw, db)


def emb_bwd_call(_lib, dev, bufs, ib, wb, V, OT, p, sdp, rows, D):
    """hyena_embed_add_norm_bwd into fresh sentinel-filled outputs: d_table gets all 16 rows, the contract writes the first V"""
    lib = _lib.lib()
    gb, hb, sb, mb, rb = bufs
    nf = lib.hyena_embed_add_norm_partial_floats(rows, D)
    assert nf == blk_grid(rows) * (2 + BLK_VMAX) * D
    o = (_out((BLK_VMAX, D), torch.float32, dev), _out((D,), torch.float32, dev), _out((D,), torch.float32, dev), _out((nf,), torch.float32, dev, D))
    _lib.check(lib.hyena_embed_add_norm_bwd(gb.ptr, _lib.dtype_code(OT), _p(hb), sb.ptr, ib.ptr, wb.ptr, mb.ptr, rb.ptr, p, sdp, o[0].ptr, V, o[1].ptr, o[2].ptr,
                                            o[3].ptr, rows, D, _lib._backend.stream(dev)))
    assert o[3].guards_intact(), "partials: a guard row was written"
    return o


def run_embed_bad_ids(_lib, dev, rows, D, V, OT, p, seed=0, label=""):
    """two ids outside [0, V), -1 and V: the forward poisons their rows of out / residual' with NaN and reads no memory for them; the backward, given
    `saved` AS THE FORWARD LEFT IT, leaves the rows out of every sum (block_kernels.h, AddNormArgs::V): d_table, dweight, dbias finite and equal to the
    references over the remaining rows"""
    lib, code, stream = _lib.lib(), _lib.dtype_code, _lib._backend.stream(dev)
    g = torch.Generator().manual_seed(seed)
    w, b = draw_params(D, g, dev)
    ids = draw_ids(rows, V, g, empty=False)
    assert rows >= 3
    bad = sorted({2, rows // 2, rows - 1})[-2:]
    ids[bad[0]] = -1
    ids[bad[-1]] = V
    ids = ids.to(dev)
    live = torch.ones(rows, dtype=torch.bool, device=dev)
    live[bad] = False
    tv, _, _, _ = draw_rows((V,), D, g, amp=1.0 if p == 0.0 else 2.0)
    table = Guarded((BLK_VMAX, D), torch.float32, dev, NAN)
    table.t[:V] = tv.float().to(dev)
    keep, ks = keep_mask(p, (rows, D), dev)
    sd = _seed(dev, p)
    sdp = None if sd is None else sd.data_ptr()
    wb, bb, ib = Guarded.input(w), Guarded.input(b), Guarded.input(ids, BAD_ID)
    st = _Stats()
    with _lib._backend.guard(dev):
        o = (_out((rows, D), OT, dev), _out((rows, D), torch.float32, dev), _out((rows,), torch.float32, dev), _out((rows,), torch.float32, dev))
        _lib.check(lib.hyena_embed_add_norm_fwd(ib.ptr, table.ptr, V, wb.ptr, bb.ptr, EPS, p, sdp, o[0].ptr, code(OT), o[1].ptr, o[2].ptr, o[3].ptr, rows, D, stream))
        out, ro, mean, rstd = o
        assert all(t.guards_intact() for t in o)
        assert bool(torch.isnan(ro.t[~live]).all()) and bool(torch.isnan(out.t[~live].float()).all()), "a row with a bad id is not NaN"
        assert bool(torch.isfinite(ro.t[live]).all()) and bool(torch.isfinite(out.t[live].float()).all()) and bool(torch.isfinite(mean.t[live]).all())
        safe = torch.where(live, ids, torch.zeros_like(ids))
        R = fwd64(table.t[:V].double()[safe], None, w.double(), b.double(), keep, ks)
        E = R["E_out"] + half_ulp_io(R["out"].abs() + R["E_out"], OT)
        assert bool(((out.t.double() - R["out"]).abs() <= E)[live].all()), "a row beside a bad id"
        # ---- the backward on what the forward stored
        sigma = _sign((rows, D), g)
        dout = (sigma * _mag((rows, D), g)).to(OT).to(dev)
        bufs = (Guarded.input(dout), None, Guarded.input(ro.t.clone()), Guarded.input(mean.t.clone()), Guarded.input(rstd.t.clone()))
        dt, dw, db, part = emb_bwd_call(_lib, dev, bufs, ib, wb, V, OT, p, sdp, rows, D)
        for name, t in (("d_table", dt.t[:V]), ("dweight", dw.t), ("dbias", db.t)):
            assert bool(torch.isfinite(t).all()), name + ": not finite with two ids outside [0, V)"
        z32 = torch.zeros((), device=dev)
        lv = live[:, None]
        Rb, onehot = emb_bwd_ref(dout, torch.where(lv, ro.t, z32), torch.where(live, mean.t, z32), torch.where(live, rstd.t, z32), w, None, keep, ks, ids, V, live)
        hold_emb_bwd(st, rows, D, V, Rb, onehot, dt, dw, db, live)
    st.pop("margin")                                   # (unstructured dout: the margin belongs to run_embed's cases)
    print(st.line(f"{label} embed-bad-ids {NAME[OT]} rows={rows} D={D} V={V} p={p}"), flush=True)
    return st


# ---- the pooled readout ------------------------------------------------------------------------------------------------------------------
def pool_lengths(B, L, kind, dev):
    """None, or an int32 tensor cycling through 0, 1, chunk_rows - 1, chunk_rows, chunk_rows + 1, L - 1, L, L + 7 (clamped to L), -3 (clamped to 0)"""
    if kind == "none":
        return None
    cr = pool_chunk_rows(B, L)
    vals = [L - 1, 0, 1, cr - 1, cr, cr + 1, L, L + 7, -3]
    return torch.tensor([vals[i % len(vals)] for i in range(B)], dtype=torch.int32, device=dev)


def run_pool(_lib, dev, B, L, D, T, with_res, p, np_, mode, kind, seed=0, label="", expect=None, wrappers=True):
    """add_norm_pool_fwd_kernel + add_norm_pool_finish_kernel, and add_norm_pool_bwd_kernel on caller-made mean / rstd.  `expect` = (chunk_rows, chunks)"""
    lib, code, stream = _lib.lib(), _lib.dtype_code(T), _lib._backend.stream(dev)
    cr, ch = pool_chunk_rows(B, L), pool_chunks(B, L)
    assert expect is None or (cr, ch) == tuple(expect), (cr, ch)
    assert lib.hyena_add_norm_pool_partial_floats(B, L, D) == B * ch * 3 * D, "chunks"
    g = torch.Generator().manual_seed(seed)
    w, b = draw_params(D, g, dev)
    idx = _order((B, 1), D, g)                                         # one channel order per sequence: x0 / residual and g share it
    x0, res = draw_forward((B, L), D, T, with_res, p, g, dev, idx=idx)
    lengths = pool_lengths(B, L, kind, dev)
    n = torch.full((B,), L, dtype=torch.int64, device=dev) if lengths is None else lengths.long().clamp(0, L)
    pad = (torch.arange(L, device=dev)[None, :] >= n[:, None])
    keep, ks = keep_mask(p, (B, L, D), dev)
    sd = _seed(dev, p)
    sdp = None if sd is None else sd.data_ptr()
    R = pool_fwd64(x0.double(), None if res is None else res.double(), w.double(), b.double(), keep, ks, n, mode)
    xin = x0.clone()
    xin[pad] = NAN                                                     # rows t >= n_b are not read
    rin = None
    if res is not None:
        rin = res.clone()
        rin[pad] = NAN
    xb, rb, wb, bb = Guarded.input(xin), None if rin is None else Guarded.input(rin), Guarded.input(w), Guarded.input(b)
    lb = None if lengths is None else Guarded.input(lengths, 1 << 20)
    m = _lib.POOL_MODES[mode]
    st = _Stats()
    with _lib._backend.guard(dev):
        def fwd():
            o = (_out((B, D), torch.float32, dev), _out((B, L), torch.float32, dev), _out((B, L), torch.float32, dev), _out((B * ch * D,), torch.float32, dev, D))
            _lib.check(lib.hyena_add_norm_pool_fwd(xb.ptr, code, _p(rb), wb.ptr, bb.ptr, EPS, p, sdp, _p(lb), m, o[0].ptr, o[1].ptr, o[2].ptr, o[3].ptr, B, L, D, stream))
            return o
        pooled, mean, rstd, part = fwd()
        assert _same((pooled, mean, rstd, part), fwd()), "add_norm_pool_fwd is not repeatable bit for bit"
        assert all(t.guards_intact() for t in (pooled, mean, rstd, part))
        assert bool((mean.t[pad] == SENTINEL).all()) and bool((rstd.t[pad] == SENTINEL).all()), "mean / rstd of a pad row were written"
        valid = ~pad
        st.hold("mean", mean.t[valid], R["mean"][valid], R["e_m"][valid])
        st.hold("rstd", rstd.t[valid], R["rstd"][valid], R["e_s"][valid])
        nf = cr // BLK_WAVES + BLK_WAVES + red_depth(ch)
        bound = sum_bound(R["S"], R["H"], nf, 1)                       # (S and H carry scale_b; both are zero where n_b = 0)
        st.hold("pooled", pooled.t, R["pooled"], bound)
        assert bool((pooled.t[n == 0] == 0).all()), "n_b = 0: pooled is exactly zero"
        terms = R["scale"][:, None, None] * R["valid"] * R["out"]
        small = torch.where(terms != 0, terms.abs(), torch.full_like(terms, float("inf"))).amin(1)
        st["margin"] = float((bound / small).max())
        if wrappers:
            ow = _lib.add_norm_pool_fwd(xin, rin, w, b, EPS, lengths=lengths, mode=mode, dropout_p=p, seed=sd)
            assert torch.equal(ow[0], pooled.t) and torch.equal(ow[1].view(B, L)[valid], mean.t[valid]) and torch.equal(ow[2].view(B, L)[valid], rstd.t[valid])
        # ---- backward: caller-made mean / rstd (the fp64 values rounded once; NaN on pad rows: not read), g per sequence
        mu = torch.where(valid, R["mean"], torch.full_like(R["mean"], NAN)).float()
        rs = torch.where(valid, R["rstd"], torch.full_like(R["rstd"], NAN)).float()
        _, ta_, q_, sg_ = _quads((B,), D, g, idx[:, 0])
        gvw = draw_gw(ta_, q_, sg_, g, (B,))                           # s1 = alpha, s2 ~ beta, |gw - s1 - xh s2| near q >= 1
        gp = (gvw.to(dev) / w.double() * (n.clamp_min(1).double()[:, None] if mode == "mean" else 1.0)).float()     # scale_b g of order one for every n_b
        gb, mb, sb = Guarded.input(gp), Guarded.input(mu), Guarded.input(rs)
        slots = B * ch

        def bwd():
            o = (_out((B * L, D), T, dev), _out((B * L, D), torch.float32, dev) if with_res else None, _out((D,), torch.float32, dev), _out((D,), torch.float32, dev),
                 _out((D,), torch.float32, dev) if np_ == 3 else None, _out((slots * 3 * D,), torch.float32, dev, D))
            _lib.check(lib.hyena_add_norm_pool_bwd(gb.ptr, xb.ptr, code, _p(rb), wb.ptr, mb.ptr, sb.ptr, p, sdp, _p(lb), m, o[0].ptr, _p(o[1]), o[2].ptr, o[3].ptr,
                                                   _p(o[4]), o[5].ptr, B, L, D, stream))
            return o
        dx, dres, dw, db, cs, part = bwd()
        assert _same((dx, dres, dw, db, cs, part), bwd()), "add_norm_pool_bwd is not repeatable bit for bit"
        assert part.guards_intact(), "partials: a guard row was written"
        Rb = pool_bwd64(gp.double(), x0.double(), None if res is None else res.double(), mu.double(), rs.double(), w.double(), keep, ks, n, mode)
        padr = pad.reshape(-1)
        assert bool((dx.t[padr] == 0).all()) and (dres is None or bool((dres.t[padr] == 0).all())), "pad rows: exactly zero, and written"
        if dres is not None:
            st.elem("d_residual", dres, Rb["dr"].reshape(B * L, D), Rb["E_dr"].reshape(B * L, D), torch.float32)
        st.elem("dx0", dx, Rb["dx"].reshape(B * L, D), Rb["E_dx"].reshape(B * L, D), T)
        nb = cr // BLK_WAVES + BLK_WAVES + red_depth(slots)
        m0 = st.pop("margin")
        st.total("dweight", dw, Rb["t_dw"].reshape(B * L, D), Rb["H_dw"].reshape(B * L, D), nb, 3)
        st.total("dbias", db, Rb["t_db"].reshape(B * L, D), None, nb, 3)
        if cs is not None:
            st.total("colsum", cs, dx.t.double(), None, nb, 0)
        st["margin"] = max(st["margin"], m0) if bool((n > 0).any()) else 0.0
        if wrappers:
            bw = _lib.add_norm_pool_bwd(gp, xin, rin, w, mu.reshape(-1), rs.reshape(-1), lengths=lengths, mode=mode, need_dres=with_res, dropout_p=p, seed=sd,
                                        offer_colsum=False)
            assert torch.equal(bw[0], dx.t) and (dres is None or torch.equal(bw[1], dres.t)) and torch.equal(bw[2], dw.t) and torch.equal(bw[3], db.t)
    print(st.line(f"{label} pool {NAME[T]} B={B} L={L} D={D} res={int(with_res)} p={p} np={np_} {mode} lengths={kind} chunk_rows={cr} chunks={ch}"), flush=True)
    assert st["margin"] < 1.0, st["margin"]
    return st


# ---- the cases: the smallest shapes that reach each path -----------------------------------------------------------------------------------
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
PAIRS = [(F32, F32), (BF16, BF16), (F16, F16), (F32, BF16), (BF16, F32)]                     # (x0 / dx0 type, out / dout type)
PAIR_ID = {p: f"{NAME[p[0]]}-{NAME[p[1]]}" for p in PAIRS}
AN_D = [64, 128, 256, 512, 1024]                                     # E = 1, 2, 4, 8, 16
AN_ROWS = [1, 3, 4, 5, 37]                                           # partial workgroups, idle wavefronts
AN_P = [0.0, 0.1, 0.5]
AN_BIG = (8197, 64)                                                  # blk_grid = 2048 (capped), 8192 rows a sweep: a second, partial sweep of 5 rows


def add_norm_cases(D, pair):
    """every rows in AN_ROWS at one (D, type pair); residual, p and np cycle so that every D meets every p (D = 64 and 128, where a lane holds a part
    of a Philox group of four, included), with and without residual, np = 2 and 3"""
    i = AN_D.index(D) + PAIRS.index(pair)
    for k, rows in enumerate(AN_ROWS):
        j = i + k
        yield dict(rows=rows, D=D, XT=pair[0], OT=pair[1], with_res=bool(j % 2), p=AN_P[(j // 2 + k) % 3], np_=2 + (j // 2) % 2, seed=100 * D + 10 * rows + PAIRS.index(pair))


def add_norm_dropout_cases(D):
    """D = 64 / 128 (E = 1 / 2): every p with both np and both residual settings, fp32 and bf16"""
    for k, p in enumerate(AN_P):
        for r in (False, True):
            yield dict(rows=37, D=D, XT=PAIRS[(k + r) % 2][0], OT=PAIRS[(k + r) % 2][1], with_res=r, p=p, np_=2 + (k + r) % 2, seed=7000 + D + 10 * k + r)


EMB_D, EMB_V, EMB_ROWS = [64, 128, 256], [1, 12, 16], [1, 3, 4, 5, 37]


def embed_cases(D, V):
    i = EMB_D.index(D) + EMB_V.index(V)
    for k, rows in enumerate(EMB_ROWS):
        j = i + k
        yield dict(rows=rows, D=D, V=V, OT=DTYPES[j % 3], p=AN_P[(j + k // 2) % 3], seed=200 * D + 10 * rows + V + k)


# (B, L, D) -> (chunk_rows, chunks), from pool_chunk_rows / pool_chunks in csrc/fftconv.hip: cap = 2048 // B workgroups a sequence,
# chunk_rows = ceil(L / cap) rounded up to a multiple of 4, chunks = ceil(L / chunk_rows)
#   (4, 37, 64):    cap 512,  ceil(37 / 512) = 1 -> 4 rows, 10 chunks, the last of one row
#   (3, 9, 256):    cap 682  -> 4 rows, 3 chunks;          (2, 5, 1024): cap 1024 -> 4 rows, 2 chunks
#   (1, 460, 64):   cap 2048 -> 4 rows, 115 chunks: thread rows 0 .. 2 of the finish kernel pass c + 112 < 115 and take the unrolled round, 3 .. 15 the tail only
#   (1, 1030, 128): cap 2048 -> 4 rows, 258 chunks: c + 112 < 258 twice for thread rows 0, 1 (c = 0, 128 -> tail at 256 + cs), once and a tail for the others
#   (64, 200, 64):  cap 32,   ceil(200 / 32) = 7 -> 8 rows (two rows per wavefront), 25 chunks; B L = 12800 > 8192 is what makes chunk_rows > 4
POOL_SHAPES = {(4, 37, 64): (4, 10), (3, 9, 256): (4, 3), (2, 5, 1024): (4, 2), (1, 460, 64): (4, 115), (1, 1030, 128): (4, 258), (64, 200, 64): (8, 25)}


def pool_cases(shape, T):
    """both modes x lengths None / ragged at one (shape, type); residual, p and np cycle so that each shape meets both values of each"""
    i = list(POOL_SHAPES).index(shape) + DTYPES.index(T)
    k = 0
    for mode in ("mean", "sum"):
        for kind in ("none", "ragged"):
            j = i + k
            yield dict(B=shape[0], L=shape[1], D=shape[2], T=T, with_res=bool((j // 2 + k) % 2), p=(0.0, 0.1)[j % 2], np_=2 + (j + k // 2) % 2, mode=mode, kind=kind,
                       seed=31 * shape[1] + shape[2] + 7 * k + DTYPES.index(T), expect=POOL_SHAPES[shape])
            k += 1
