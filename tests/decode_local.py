"""Element-wise fp64 references and derived bounds for the decode kernels of csrc/decode_kernels.h: the convolution and post kernels of the four
families (single position, _rows, _fan, _block / _block_fan) and the pre kernels of the three variants, each called ON ITS OWN through the C ABI
on caller-made buffers.  Shared by the emulator tests (tests/test_decode_local_emu.py) and the GPU tests (tests/test_gpu_decode_local.py).  Plain
torch, device-agnostic; not a test file.  Derivations, observed figures and seeded defects: profiles/decode_local.md.

Every reference starts from the stored operands the kernel read (16-bit values widened exactly to fp64).  u = 2^-24, gamma_n = n u / (1 - n u).

    conv    part[chunk][slot][i][d] = sum over the chunk's s <= t0 + i of k[d, t0 + i - s] vg[., d, s]                  (fp32 for every I/O type)
                |got - ref64| <= gamma_40 sum |k vg|              40 = 32 FMAs of a lane (DEC_NV DEC_V, the product unrounded) + 6 butterfly steps
                                                                   + the two levels of (r0 + r1) + (r2 + r3); the block kernel keeps each output's chain
    post    y = the nc partials in chunk order, then fma(vg_t, fb, y)          E_y  = gamma_(nc + 1) (sum |part| + |fb vg_t|)
            yr = round_io(y)                                                   E_yr = E_y + half_ulp_io(|y64| + E_y)
            z = round_io(yr x0)      |z - y64 x0| <= e + U m + half_ulp_io(m + U m),    e = |x0| E_yr,  m = |y64 x0| + e
    pre     x0 against sc64 of group 0 within sc_err; the history column against c1 cv within pre_fwd64's bound (sc_err propagated, one fp32
            rounding) + half_ulp_io; the tail afterwards EXACTLY the last two of (old tail, the block's raw inputs)

Operands of the "flat" family: |k|, |vg| in [0.5, 1] with random signs (post: partials, fb, vg_t in [1, 2], x0 in [0.5, 1]), so the loss or the
doubling of one term moves a result by more than its bound: every runner asserts margin < 1.  The "decay" family is the filter of the existing
decode tests, randn exp(-3 j / Lcap), against a randn history: the same bound, no margin claimed.

Poison: history columns in (t, t | 7] hold SENTINEL (finite, as the header requires of what a vector load may touch), those past t | 7 NaN, k
columns past t NaN, padding columns of x NaN, rows b >= B of every Bcap-sized buffer SENTINEL, `part` NaN before conv, and for post NaN in every
slot the header says is not read.  After every call: inputs bitwise unchanged, every slot or element the contract leaves alone bitwise untouched."""
import torch

from tests import shell_local as SL
from tests.shell_local import DTYPES, NAME, SENTINEL, U, gamma, half_ulp_io, sc64, sc_err  # noqa: F401  (DTYPES, NAME: the test files' ids)

CHUNK, TMAX = 8192, 64
N_CONV = 40                              # 32 FMAs + 6 butterfly steps + 2 levels across the four wavefronts
NAN = float("nan")
FORMS = ("single", "rows", "fan", "block", "block_fan")


def _ceil(n, m):
    return (n + m - 1) // m * m


def _bits(t):
    return t.view({4: torch.int32, 2: torch.int16}[t.element_size()])


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def flat(shape, g, T, dev, lo=0.5, hi=1.0):
    """magnitudes uniform in [lo, hi] with random signs, drawn on the host and then rounded to T (which keeps them in range)"""
    v = (lo + (hi - lo) * torch.rand(shape, generator=g)) * (torch.randint(0, 2, shape, generator=g) * 2 - 1)
    return v.to(T).to(dev)


def _min_nonzero(t):
    a = t.abs().double().flatten()
    a = a[a > 0]
    return float(a.min()) if a.numel() else float("inf")


class _Stats(dict):
    def hold(self, name, got, ref, bound):
        diff = (got.double() - ref).abs()
        ok = diff <= bound
        nz = bound > 0
        r = float((diff[nz] / bound[nz]).max()) if bool(nz.any()) else 0.0
        self[name] = max(self.get(name, 0.0), r)
        assert bool(ok.all()), (name, r, int((~ok).sum()), float(diff.max()))

    def line(self, label):
        return f"[decode-local] {label} " + " ".join(f"{k}={v:.3g}" for k, v in self.items())


# ---- the convolution kernels ---------------------------------------------------------------------------------------------------------------
def conv_ref(k64, h64, t0, T, s0):
    """h64 (R, D, n): history columns s0 .. s0 + n - 1 of one chunk; k64 (D, >= t0 + T - s0).  -> ref, S (R, T, D): the fp64 sum of
    k[d, t0 + i - s] h[r, d, s] over the columns with s <= t0 + i, and the sum of the terms' magnitudes.  At most 2^22 products at a time."""
    R, D, n = h64.shape
    dev = h64.device
    j = (t0 + torch.arange(T, device=dev))[None, :] - (s0 + torch.arange(n, device=dev))[:, None]          # (n, T): the tap of (s, i)
    ok = (j >= 0).double()
    j = j.clamp_min(0)
    ref = torch.zeros(R, T, D, dtype=torch.float64, device=dev)
    S = torch.zeros_like(ref)
    step = max(1, (1 << 22) // (n * T))
    for d0 in range(0, D, step):
        km = k64[d0:d0 + step][:, j] * ok                                                                  # (dd, n, T)
        hh = h64[:, d0:d0 + step]
        ref[:, :, d0:d0 + step] = torch.einsum("rdn,dnt->rtd", hh, km)
        S[:, :, d0:d0 + step] = torch.einsum("rdn,dnt->rtd", hh.abs(), km.abs())
    return ref, S


def _conv_operands(family, G, fan, D, Lcap, S, g, T, dev):
    """k (D, Lcap) fp32, shared history (G, D, S) or None, row history (G fan, D, Lcap - S): drawn independently of each other"""
    B = G * fan
    if family == "flat":
        k = flat((D, Lcap), g, torch.float32, dev)
        hs = flat((G, D, S), g, T, dev) if S else None
        hr = flat((B, D, Lcap - S), g, T, dev)
    else:
        assert family == "decay"
        k = (torch.randn(D, Lcap, generator=g) * torch.exp(-3.0 * torch.linspace(0, 1, Lcap))[None]).to(dev)
        hs = torch.randn(G, D, S, generator=g).to(T).to(dev) if S else None
        hr = torch.randn(B, D, Lcap - S, generator=g).to(T).to(dev)
    return k, hs, hr


def _live(form, t, Tn, S, Lcap):
    return t >= S and t + Tn <= Lcap if form.startswith("block") else (S if form == "fan" else 0) <= t < Lcap


def _dense(shape, fill, dtype, dev, pitch):
    """the default `alloc` of the runners: a packed tensor (pitch = its last dimension)"""
    assert pitch == shape[-1]
    return torch.full(shape, fill, dtype=dtype, device=dev)


def _hist_buffer(hr, B, Bcap, ld, last, T, dev, alloc=_dense, pitch=None):
    """(Bcap, D, ld): row b holds its operand up to column last[b], SENTINEL in (last, last | 7], NaN beyond; a row with last[b] None (parked:
    nothing of it is read) NaN throughout; rows b >= B SENTINEL"""
    D = hr.shape[1]
    buf = alloc((Bcap, D, ld), NAN, T, dev, ld if pitch is None else pitch)
    for b in range(B):
        if last[b] is not None:
            buf[b, :, :last[b] + 1] = hr[b, :, :last[b] + 1]
            buf[b, :, last[b] + 1:(last[b] | 7) + 1] = SENTINEL
    buf[B:] = SENTINEL
    return buf


def run_conv(_lib, dev, T, form, B, Bcap, D, Lcap, pos, Tn=1, S=0, fan=1, family="flat", seed=0, ldk_extra=4, label="", kpitch=None, rpitch=None,
             alloc=_dense):
    """one call of hyena_decode_conv / _rows / _fan / _block / _block_fan.  pos: the position (rows: one per row).  Every slot of `part` the
    header names within gamma_40 sum|k vg| of its own chunk's fp64 sum, every other slot bitwise the NaN it held (block: the outputs before a
    chunk that starts inside the block untouched or exactly 0), inputs and pos unchanged.  -> (figures, part)
    kpitch / rpitch: the caller's own row pitch of k / of the row history, handed to the library instead of the rows' width; alloc(shape, fill, dtype,
    dev, pitch) then makes a tensor of `shape` whose rows lie `pitch` elements apart (tests/limits_local.py: gigabytes apart, nothing filled between)."""
    assert form in FORMS and B % fan == 0 and (form in ("fan", "block_fan") or (S == 0 and fan == 1)) and (Tn == 1 or form.startswith("block"))
    lib = _lib.lib()
    code, stream = _lib.dtype_code(T), _lib._backend.stream(dev)
    g = torch.Generator().manual_seed(seed)
    G, ns = B // fan, S // CHUNK
    kv, hs, hr = _conv_operands(family, G, fan, D, Lcap, S, g, T, dev)
    tb = [int(p) for p in pos] if form == "rows" else [int(pos)] * B
    live = [_live(form, t, Tn, S, Lcap) for t in tb]
    tmax = [t + Tn - 1 if lv else None for t, lv in zip(tb, live)]
    kmax = max([t for t in tmax if t is not None], default=-1)
    nch = -(-Lcap // CHUNK)
    nfl = lib.hyena_decode_block_partial_floats(B, D, Lcap, Tn) if form.startswith("block") else lib.hyena_decode_partial_floats(B, D, Lcap)
    assert nfl == nch * B * Tn * D
    ldk, lds, ldr = _ceil(Lcap, 4) + ldk_extra, S + 8, _ceil(max(Lcap - S, 1), 8)
    kpitch, rpitch = ldk if kpitch is None else kpitch, ldr if rpitch is None else rpitch
    k = alloc((D, ldk), NAN, torch.float32, dev, kpitch)
    k[:, :kmax + 1] = kv[:, :kmax + 1]
    vgs = None
    if S:
        vgs = torch.full((G, D, lds), NAN, dtype=T, device=dev)
        vgs[:, :, :S] = hs
    vgr = _hist_buffer(hr, B, Bcap, ldr, [None if t is None else t - S for t in tmax], T, dev, alloc, rpitch)
    part = torch.full((nch, B, Tn, D), NAN, device=dev)
    posb = torch.tensor(tb if form == "rows" else tb[:1], dtype=torch.int32, device=dev)
    ins = [k, vgr, posb] + ([vgs] if S else [])
    keep = [x.clone() for x in ins]
    part0 = part.clone()
    P = lambda x: None if x is None else x.data_ptr()  # noqa: E731
    with _lib._backend.guard(dev):
        if form == "single":
            st_ = lib.hyena_decode_conv(P(k), kpitch, P(vgr), P(part), P(posb), B, D, Lcap, rpitch, code, stream)
        elif form == "rows":
            st_ = lib.hyena_decode_conv_rows(P(k), kpitch, P(vgr), P(part), P(posb), B, D, Lcap, rpitch, code, stream)
        elif form == "fan":
            st_ = lib.hyena_decode_conv_fan(P(k), kpitch, P(vgs), P(vgr), P(part), P(posb), B, fan, D, Lcap, S, lds, rpitch, code, stream)
        elif form == "block":
            st_ = lib.hyena_decode_conv_block(P(k), kpitch, P(vgr), P(part), P(posb), B, D, Lcap, rpitch, Tn, code, stream)
        else:
            st_ = lib.hyena_decode_conv_block_fan(P(k), kpitch, P(vgs), P(vgr), P(part), P(posb), B, fan, D, Lcap, S, lds, rpitch, Tn, code, stream)
        _lib.check(st_)
    assert all(same_bits(a, b) for a, b in zip(ins, keep)), "conv wrote one of its inputs (or pos)"
    # ---- what every slot must hold
    k64 = k.double()
    named = torch.zeros(nch, B, Tn, D, dtype=torch.bool, device=dev)          # slots the header names: finite, within bound
    early = torch.zeros_like(named)                                            # block: outputs before a chunk that starts inside the block
    ref = torch.zeros(nch, B, Tn, D, dtype=torch.float64, device=dev)
    Sabs = torch.zeros_like(ref)
    for ch in range(nch):
        s0 = ch * CHUNK
        groups = {}                                                           # first position -> rows (one group unless per-row positions)
        for b in range(B):
            if live[b] and s0 <= tmax[b] and (ch >= ns or b % fan == 0):
                groups.setdefault(tb[b], []).append(b)
        for t0, rows in groups.items():
            n = min(t0 + Tn - 1, s0 + CHUNK - 1) - s0 + 1
            rr = torch.tensor(rows, device=dev)
            h = hs[rr // fan, :, s0:s0 + n] if ch < ns else hr[rr, :, s0 - S:s0 - S + n]
            r, a = conv_ref(k64, h.double(), t0, Tn, s0)
            ref[ch, rr], Sabs[ch, rr] = r, a
            i0 = max(0, s0 - t0)                                              # the first output that has a term in this chunk
            named[ch, rr, i0:] = True
            early[ch, rr, :i0] = True
    bound = gamma(N_CONV) * Sabs
    st = _Stats()
    got = part[named]
    assert bool(torch.isfinite(got).all()), "a slot the header names is not finite"
    st.hold(f"conv_{form}", got, ref[named], bound[named])
    same = _bits(part) == _bits(part0)
    zero = _bits(part) == 0
    assert bool(same[~named & ~early].all()), "conv wrote a slot of `part` that the header does not name"
    assert bool((same | zero)[early].all()), "an output before its chunk's start is neither untouched nor exactly 0"
    if bool(early.any()):
        st["early_zeroed"] = float(zero[early].double().mean())
    if family == "flat" and bool(named.any()):
        used = [hr[b, :, :tmax[b] - S + 1] for b in range(B) if live[b] and tmax[b] >= S] + ([hs] if S else [])
        small = _min_nonzero(kv[:, :kmax + 1]) * min(_min_nonzero(u) for u in used)       # no product of the case is smaller
        st["margin"] = float(bound.max()) / small
    print(st.line(f"{label} conv {form} {NAME[T]} {family} B={B}/{Bcap} D={D} Lcap={Lcap} pos={pos} T={Tn} S={S} fan={fan}"), flush=True)
    assert st.get("margin", 0.0) < 1.0, ("the bound exceeds the smallest single term: the case is too large to see a lost term", st["margin"])
    return st, part


# ---- the post kernels ----------------------------------------------------------------------------------------------------------------------
def post_bound(y64, A, nc, x0, T):
    """y64 the fp64 sum of the nc partials and fb vg_t, A the sum of their magnitudes, x0 fp64 -> the bound of |z - y64 x0|"""
    Ey = gamma(nc + 1.0) * A
    Eyr = Ey + half_ulp_io(y64.abs() + Ey, T)
    e = x0.abs() * Eyr
    m = (y64 * x0).abs() + e
    return e + U * m + half_ulp_io(m + U * m, T)


def run_post(_lib, dev, T, form, B, Bcap, D, Lcap, pos, Tn=1, S=0, fan=1, with_fb=True, seed=0, label=""):
    """one call of hyena_decode_post / _rows / _fan / _block / _block_fan on caller-made partials (magnitudes in [1, 2], NaN in every slot the
    header says is not read), x0 in [0.5, 1], fb and history column t in [1, 2] (every other history column NaN).  z within post_bound of
    y64 x0 at every element, rows b >= B and parked rows untouched, pos advanced by exactly 1 / T.  -> (figures, z)"""
    assert form in FORMS and B % fan == 0 and (form in ("fan", "block_fan") or (S == 0 and fan == 1)) and (Tn == 1 or form.startswith("block"))
    lib = _lib.lib()
    code, stream = _lib.dtype_code(T), _lib._backend.stream(dev)
    g = torch.Generator().manual_seed(seed)
    ns, nch = S // CHUNK, -(-Lcap // CHUNK)
    tb = [int(p) for p in pos] if form == "rows" else [int(pos)] * B
    live = torch.tensor([_live(form, t, Tn, S, Lcap) for t in tb], device=dev)
    ldr = _ceil(max(Lcap - S, 1), 8)
    tpos = torch.tensor(tb, device=dev)[:, None] + torch.arange(Tn, device=dev)[None, :]                    # (B, Tn): position of output (b, i)
    ch = torch.arange(nch, device=dev)[:, None, None]
    used = (ch < (tpos // CHUNK + 1)[None]) & live[None, :, None]                                           # (nch, B, Tn): element reads chunk ch
    rows = torch.arange(B, device=dev)
    src = torch.where(ch < ns, (rows // fan * fan)[None, :, None], rows[None, :, None]).expand(nch, B, Tn)  # ... from this row's slot
    ii = torch.arange(Tn, device=dev)[None, None, :].expand(nch, B, Tn)
    chh = ch.expand(nch, B, Tn)
    read = torch.zeros(nch, B, Tn, dtype=torch.bool, device=dev)
    read[chh[used], src[used], ii[used]] = True
    part = torch.full((nch, B, Tn, D), NAN, device=dev)
    part[read] = flat((int(read.sum()), D), g, torch.float32, dev, 1.0, 2.0)
    vgr = torch.full((Bcap, D, ldr), NAN, dtype=T, device=dev)
    vgr[B:] = SENTINEL
    vt = flat((B, Tn, D), g, T, dev, 1.0, 2.0)
    x0 = torch.full((Bcap, Tn, D), SENTINEL, device=dev)
    x0[:B] = flat((B, Tn, D), g, torch.float32, dev)
    for b in range(B):
        if bool(live[b]):
            vgr[b, :, tb[b] - S:tb[b] - S + Tn] = vt[b].t()
        else:
            x0[b] = NAN                                                        # a parked row, a block that does not fit: nothing is read
    fb = flat((D,), g, torch.float32, dev, 1.0, 2.0) if with_fb else None
    z = torch.full((Bcap, Tn, D), SENTINEL, dtype=T, device=dev)
    posb = torch.tensor(tb if form == "rows" else tb[:1], dtype=torch.int32, device=dev)
    ins = [part, vgr, x0] + ([fb] if with_fb else [])
    keep = [x.clone() for x in ins]
    P = lambda x: None if x is None else x.data_ptr()  # noqa: E731
    with _lib._backend.guard(dev):
        if form == "single":
            st_ = lib.hyena_decode_post(P(part), P(vgr), P(fb), P(x0), P(z), P(posb), B, D, Lcap, ldr, code, stream)
        elif form == "rows":
            st_ = lib.hyena_decode_post_rows(P(part), P(vgr), P(fb), P(x0), P(z), P(posb), B, D, Lcap, ldr, code, stream)
        elif form == "fan":
            st_ = lib.hyena_decode_post_fan(P(part), P(vgr), P(fb), P(x0), P(z), P(posb), B, fan, D, Lcap, S, ldr, code, stream)
        elif form == "block":
            st_ = lib.hyena_decode_post_block(P(part), P(vgr), P(fb), P(x0), P(z), P(posb), B, D, Lcap, ldr, Tn, code, stream)
        else:
            st_ = lib.hyena_decode_post_block_fan(P(part), P(vgr), P(fb), P(x0), P(z), P(posb), B, fan, D, Lcap, S, ldr, Tn, code, stream)
        _lib.check(st_)
    assert all(same_bits(a, b) for a, b in zip(ins, keep)), "post wrote one of its inputs"
    want = [t + Tn if bool(lv) else t for t, lv in zip(tb, live)]
    assert posb.tolist() == (want if form == "rows" else want[:1]), ("pos", posb.tolist(), want)
    terms = torch.where(used[..., None], part.double()[chh, src, ii], torch.zeros((), dtype=torch.float64, device=dev))   # (nch, B, Tn, D)
    y64, A = terms.sum(0), terms.abs().sum(0)
    small = _min_nonzero(terms)
    if with_fb:
        f = fb.double()[None, None, :] * vt.double()
        y64, A, small = y64 + f, A + f.abs(), min(small, _min_nonzero(f))
    x64 = x0[:B].double()
    nc = (tpos // CHUNK + 1).double()[..., None]
    bound = post_bound(y64, A, nc, x64, T)
    st = _Stats()
    lv = live[:, None, None].expand(B, Tn, D)
    assert bool((z[B:] == SENTINEL).all()) and bool((z[:B][~lv] == SENTINEL).all()), "post wrote a z row that the contract leaves alone"
    got = z[:B][lv]
    assert bool(torch.isfinite(got).all()), "z is not finite: a slot or a history column that is not to be read was read"
    if bool(live.any()):
        st.hold(f"post_{form}", got, (y64 * x64)[lv], bound[lv])
        st["margin"] = float((bound / (x64.abs() * small))[lv].max())          # a lost term moves z by at least |x0| small
    print(st.line(f"{label} post {form} {NAME[T]} B={B}/{Bcap} D={D} Lcap={Lcap} pos={pos} T={Tn} S={S} fan={fan} fb={int(with_fb)}"), flush=True)
    assert st.get("margin", 0.0) < 1.0, ("the bound exceeds the effect of the smallest single term", st["margin"])
    return st, z


# ---- the pre kernels of the variants -----------------------------------------------------------------------------------------------------
def run_pre(_lib, dev, T, form, B, Bcap, D, pos, Tn=1, S=0, Lcap=None, bias=True, seed=0, label=""):
    """one call of hyena_decode_pre_rows / _fan / _block / _block_fan with ldx = 3D + 5 (padding NaN), history and x0 prefilled with SENTINEL, the
    tail NaN where its position is before 0.  x0 and the new history columns within their bounds, the tail exactly the last two of (old tail,
    raw inputs), everything else untouched, pos unchanged.  -> figures"""
    assert form in ("rows", "fan", "block", "block_fan") and (form in ("fan", "block_fan") or S == 0) and (Tn == 1 or form.startswith("block"))
    lib = _lib.lib()
    code, stream = _lib.dtype_code(T), _lib._backend.stream(dev)
    g = torch.Generator().manual_seed(seed)
    tb = [int(p) for p in pos] if form == "rows" else [int(pos)] * B
    Lcap = max(tb) + Tn + 3 if Lcap is None else Lcap                        # (rows: a position outside [0, Lcap) is a parked row)
    live = [_live(form, t, Tn, S, Lcap) for t in tb]
    ldx, ldr = 3 * D + 5, _ceil(Lcap - S, 8)
    w, b_, bin_ = SL._params(3 * D, g, dev, bias)
    X = SL._operand((3 * D, B, 2 + Tn), g, T, dev)                             # row b: positions t_b - 2, t_b - 1, t_b .. t_b + Tn - 1
    tail = torch.full((3 * D, Bcap, 2), SENTINEL, device=dev)
    for b in range(B):
        tail[:, b, 0] = X[:, b, 0].float() if tb[b] >= 2 else NAN
        tail[:, b, 1] = X[:, b, 1].float() if tb[b] >= 1 else NAN
    x = torch.full((B, Tn, ldx), NAN, dtype=T, device=dev)
    x[:, :, :3 * D] = X[:, :, 2:].permute(1, 2, 0)
    vgr = torch.full((Bcap, D, ldr), SENTINEL, dtype=T, device=dev)
    x0 = torch.full((Bcap, Tn, D), SENTINEL, device=dev)
    posb = torch.tensor(tb if form == "rows" else tb[:1], dtype=torch.int32, device=dev)
    ins = [x, w, b_, posb] + ([bin_] if bias else [])
    keep = [t.clone() for t in ins]
    tail0 = tail.clone()
    P = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    with _lib._backend.guard(dev):
        if form == "rows":
            st_ = lib.hyena_decode_pre_rows(P(x), ldx, P(bin_), P(w), P(b_), P(tail), P(vgr), P(x0), P(posb), B, Bcap, D, Lcap, ldr, code, stream)
        elif form == "fan":
            st_ = lib.hyena_decode_pre_fan(P(x), ldx, P(bin_), P(w), P(b_), P(tail), P(vgr), P(x0), P(posb), B, Bcap, D, Lcap, S, ldr, code, stream)
        elif form == "block":
            st_ = lib.hyena_decode_pre_block(P(x), ldx, P(bin_), P(w), P(b_), P(tail), P(vgr), P(x0), P(posb), B, Bcap, D, Lcap, ldr, Tn, code,
                                             stream)
        else:
            st_ = lib.hyena_decode_pre_block_fan(P(x), ldx, P(bin_), P(w), P(b_), P(tail), P(vgr), P(x0), P(posb), B, Bcap, D, Lcap, S, ldr, Tn,
                                                 code, stream)
        _lib.check(st_)
    assert all(same_bits(a, c) for a, c in zip(ins, keep)), "pre wrote one of its inputs (or pos)"
    st = _Stats()
    w64, b64, bin64 = w.double(), b_.double(), None if bin_ is None else bin_.double()
    seq = torch.cat([tail0[:, :B], X[:, :, 2:].float()], dim=2)                # (3D, B, 2 + Tn): old tail, then the raw inputs
    for b in range(B):
        if not live[b]:
            assert same_bits(tail[:, b], tail0[:, b]), "the tail of a row that does not advance was shifted"
            assert bool((vgr[b] == SENTINEL).all()) and bool((x0[b] == SENTINEL).all()), "a row that does not advance was written"
            continue
        off = min(tb[b], 2)                                                    # sc64 pads with zeros before its first column: position 0
        xin = X[:, b:b + 1, 2 - off:].double()
        vg64, Evg = SL.pre_fwd64(xin, bin64, w64, b64, xin.shape[-1])          # (1, D, off + Tn)
        c0 = sc64(xin[:D], None if bin64 is None else bin64[:D], w64[:D], b64[:D])[:, 0, off:]                # (D, Tn)
        e0 = sc_err(xin[:D], None if bin64 is None else bin64[:D], w64[:D], b64[:D])[:, 0, off:]
        st.hold(f"pre_{form}.x0", x0[b].t(), c0, e0)
        ref, E = vg64[0, :, off:], Evg[0, :, off:]
        c = tb[b] - S
        got = vgr[b, :, c:c + Tn]
        assert bool(torch.isfinite(got).all())
        st.hold(f"pre_{form}.vg", got, ref, E + half_ulp_io(ref.abs() + E, T))
        other = torch.ones(ldr, dtype=torch.bool, device=dev)
        other[c:c + Tn] = False
        assert bool((vgr[b][:, other] == SENTINEL).all()), "a history column other than the new ones was written"
        assert same_bits(tail[:, b], seq[:, b, -2:]), "the tail is not exactly the last two raw inputs"
    assert bool((vgr[B:] == SENTINEL).all()) and bool((x0[B:] == SENTINEL).all()) and bool((tail[:, B:] == SENTINEL).all()), "rows b >= B"
    print(st.line(f"{label} pre {form} {NAME[T]} B={B}/{Bcap} D={D} pos={pos} T={Tn} S={S} bin={int(bias)}"), flush=True)
    return st


# ---- the cases: the smallest shapes that reach each path ------------------------------------------------------------------------------------
CONV_SINGLE = [(8200, (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 15, 16)),           # the first vector partial or full, the window base negative, every phase
               (8200, (8183, 8184, 8188, 8189, 8190, 8191, 8192, 8193, 8194, 8195, 8196, 8197, 8198, 8199)),    # chunk 0's jlo crosses 0
               (8195, (8194,)),                                             # the last position of a cache whose pitch exceeds Lcap
               (16400, (16383, 16384, 16390))]                              # two full chunks and the start of a third
CONV_SINGLE_LONG = ((1 << 19) + 5, (1 << 20) - 8192, (1 << 20) - 1)        # Lcap = 2^20: 65 and 128 chunks, B = 1, D = 2
CONV_ROWS = [(8193, -1, 8193, 5, 16390), (16400, 0, 8191, 8192, 8191), (-1, 16400, -5, 20000, 16400)]      # B = 5 of 6, Lcap = 16400; all parked
FAN_S = (0, 8192, 16384)
FAN_DT = (0, 1, 7, 8, 8191, 8192)                                           # t - S, Lcap = S + 8200
BLOCK_T = (1, 3, 4, 5, 12, 13, 16, 17, 29, 60, 63, 64)
BLOCK_LCAP = 8270                                                           # above S; not a multiple of 8


def block_offsets(Tn):
    """t0 - S: the start, one in, the block ending at the chunk edge, straddling it (8185: from T = 8 on; 8191: from T = 2 on), starting on it,
    ending at the cache's end"""
    return sorted({0, 1, CHUNK - Tn, 8185, 8191, CHUNK, BLOCK_LCAP - Tn})


POST_T = (0, 8191, 8192, 16384)                                             # nc = 1, 1, 2, 3 at Lcap = 16400; nc = 128: t = 2^20 - 1 at Lcap = 2^20
POST_ROWS = [(8193, -1, 16384, 5, 16399), (16400, 0, 8191, 8192, 20000)]
PRE_T = (0, 1, 2, 5)
PRE_BLOCK_T = (1, 2, 3, 8, 9, 64)
WIDE = dict(B=4, Bcap=4, D=256, Lcap=16500)                                 # GPU only: the shipped width, a grid of 3 x 256 workgroups
WIDE_POS = 16389


# ---- the suites: what one test function of either test file runs (emulator and GPU share them) ---------------------------------------------
def suite_conv_single(_lib, dev, T, Lcap, ts, label):
    """B = 3 of 4: the LDS parity of the wavefront sums alternates and comes round; the decay family once, at the last position"""
    for t in ts:
        run_conv(_lib, dev, T, "single", 3, 4, 3 if t % 2 else 2, Lcap, t, seed=Lcap + t, label=label)
    run_conv(_lib, dev, T, "single", 3, 4, 2, Lcap, ts[-1], family="decay", seed=Lcap, label=label)
    run_conv(_lib, dev, T, "single", 3, 4, 2, Lcap, Lcap, seed=Lcap, label=label)                         # out of range: nothing is written


def suite_conv_single_long(_lib, dev, T, t, label):
    run_conv(_lib, dev, T, "single", 1, 1, 2, 1 << 20, t, seed=t, ldk_extra=0, label=label)
    if t == (1 << 20) - 1:
        run_conv(_lib, dev, T, "single", 1, 1, 2, 1 << 20, t, family="decay", seed=t, ldk_extra=0, label=label)


def suite_conv_rows(_lib, dev, T, label):
    for i, pos in enumerate(CONV_ROWS):
        run_conv(_lib, dev, T, "rows", 5, 6, 2 + i % 2, 16400, pos, seed=100 + i, label=label)
    run_conv(_lib, dev, T, "rows", 5, 6, 2, 16400, CONV_ROWS[0], family="decay", seed=103, label=label)
    run_conv(_lib, dev, T, "rows", 3, 3, 2, 8200, (8199, 8199, 8199), seed=104, label=label)              # equal positions: the window is kept


def suite_conv_fan(_lib, dev, T, S, label):
    for dt in FAN_DT:
        run_conv(_lib, dev, T, "fan", 6, 7, 2, S + 8200, S + dt, S=S, fan=3, seed=S + dt, label=label)
    run_conv(_lib, dev, T, "fan", 6, 7, 2, S + 8200, S + 8199, S=S, fan=3, family="decay", seed=S + 1, label=label)
    run_conv(_lib, dev, T, "fan", 2, 3, 3, S + 8200, S + 9, S=S, fan=1, seed=S + 2, label=label)          # fan = 1
    if S:
        run_conv(_lib, dev, T, "fan", 6, 7, 2, S + 8200, S - 1, S=S, fan=3, seed=S + 3, label=label)      # below S: nothing is written


def suite_conv_block(_lib, dev, T, Tn, label):
    """the plain kernel and the fan form (S = 8192, G = 2, fan = 2) at the same offsets; every one of the Tn outputs against its own sum"""
    for off in block_offsets(Tn):
        run_conv(_lib, dev, T, "block", 2, 3, 2, BLOCK_LCAP, off, Tn=Tn, seed=off + Tn, label=label)
        run_conv(_lib, dev, T, "block_fan", 4, 5, 2, CHUNK + BLOCK_LCAP, CHUNK + off, Tn=Tn, S=CHUNK, fan=2, seed=off + Tn + 1, label=label)
    run_conv(_lib, dev, T, "block", 2, 3, 2, BLOCK_LCAP, 8185, Tn=Tn, family="decay", seed=Tn, label=label)
    run_conv(_lib, dev, T, "block_fan", 4, 5, 2, CHUNK + BLOCK_LCAP, CHUNK + 8185, Tn=Tn, S=CHUNK, fan=2, family="decay", seed=Tn, label=label)
    run_conv(_lib, dev, T, "block", 2, 3, 2, BLOCK_LCAP, BLOCK_LCAP - Tn + 1, Tn=Tn, seed=Tn, label=label)   # does not fit: nothing is written


def suite_post(_lib, dev, T, form, with_fb, label):
    """nc = 1, 1, 2, 3 at Lcap = 16400 and nc = 128 at 2^20, B = 3 of 4 (fan: G = 2, fan = 2, S = 8192; t = 0 is below S: nothing happens)"""
    kw = dict(S=CHUNK, fan=2) if form in ("fan", "block_fan") else {}
    B, Bcap = (4, 5) if kw else (3, 4)
    if form == "rows":
        for i, pos in enumerate(POST_ROWS):
            run_post(_lib, dev, T, "rows", 5, 6, 3, 16400, pos, with_fb=with_fb, seed=200 + i, label=label)
        run_post(_lib, dev, T, "rows", 3, 4, 2, 1 << 20, ((1 << 20) - 1, 8192, 1 << 20), with_fb=with_fb, seed=202, label=label)
    elif form.startswith("block"):
        for Tn in (1, 17, 64):
            for t0 in (8192 - Tn // 2 - 1, 16384 - Tn // 2, 16400 - Tn, 16400 - Tn + 1):             # across both edges, the end, one too far
                run_post(_lib, dev, T, form, B, Bcap, 3, 16400, t0, Tn=Tn, with_fb=with_fb, seed=t0 + Tn, label=label, **kw)
        run_post(_lib, dev, T, form, B, Bcap, 2, 1 << 20, (1 << 20) - 17, Tn=17, with_fb=with_fb, seed=203, label=label, **kw)
    else:
        for t in POST_T:
            run_post(_lib, dev, T, form, B, Bcap, 3, 16400, t, with_fb=with_fb, seed=300 + t, label=label, **kw)
        run_post(_lib, dev, T, form, B, Bcap, 2, 1 << 20, (1 << 20) - 1, with_fb=with_fb, seed=301, label=label, **kw)
        run_post(_lib, dev, T, form, B, Bcap, 3, 16400, 16400, with_fb=with_fb, seed=302, label=label, **kw)     # out of range: nothing changes
    if form == "single":
        run_post(_lib, dev, T, "single", 5, 6, 256, 8200, 8192, with_fb=with_fb, seed=303, label=label)         # B D > 1024: the stride loop


def suite_pre(_lib, dev, T, form, bias, label):
    """B = 3 of 4 and D = 100: two workgroups, the second partial; ldx = 3D + 5"""
    if form == "rows":
        for i, pos in enumerate([(0, -1, 5), (1, 8, 2), (2, 5, 0), (5, 1, -3)]):
            run_pre(_lib, dev, T, "rows", 3, 4, 100, pos, Lcap=8, bias=bias, seed=400 + i, label=label)
    elif form == "fan":
        for t in PRE_T:
            run_pre(_lib, dev, T, "fan", 3, 4, 100, t, bias=bias, seed=410 + t, label=label)
        for t in (CHUNK, CHUNK + 5, CHUNK - 1):                                                        # column t - S; below S nothing happens
            run_pre(_lib, dev, T, "fan", 3, 4, 100, t, S=CHUNK, Lcap=CHUNK + 8, bias=bias, seed=420 + t, label=label)
    else:
        for Tn in PRE_BLOCK_T:
            for t0 in PRE_T:
                run_pre(_lib, dev, T, "block", 3, 4, 100, t0, Tn=Tn, bias=bias, seed=430 + 10 * Tn + t0, label=label)
            run_pre(_lib, dev, T, "block_fan", 3, 4, 100, CHUNK + (Tn % 3), Tn=Tn, S=CHUNK, bias=bias, seed=440 + Tn, label=label)
        run_pre(_lib, dev, T, "block", 3, 4, 100, 5, Tn=9, Lcap=13, bias=bias, seed=450, label=label)       # t0 + T = Lcap + 1: nothing changes


def suite_wide(_lib, dev, T, kind, form, label):
    """GPU only: the shipped width, D = 256, B = 4, Lcap = 16500, t (t0) = 16389, T = 64; two runs on fresh buffers, bitwise equal"""
    kw = dict(S=CHUNK, fan=2) if form in ("fan", "block_fan") else {}
    Tn = 64 if form.startswith("block") else 1
    pos = (WIDE_POS, 8191, WIDE_POS - 1, 16499) if form == "rows" else WIDE_POS
    run = run_conv if kind == "conv" else run_post
    st, a = run(_lib, dev, T, form, pos=pos, Tn=Tn, seed=500, label=label, **WIDE, **kw)
    _, b = run(_lib, dev, T, form, pos=pos, Tn=Tn, seed=500, label=label, **WIDE, **kw)
    assert same_bits(a, b), "two runs on fresh buffers differ"
    return st
