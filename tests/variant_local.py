"""fp64 references and derived bounds for the edited-window kernels of csrc/variant_kernels.h (hyena_variant_pre, hyena_variant_conv), the
operator route on top (HyenaOperator.forward(u, inference_params=EditWindowParams)) and the model's entry points (HyenaDNALM.forward_edited_windows,
score_variants, saturation_mutagenesis).  Shared by tests/test_variant_emu.py (CPU emulation) and tests/test_gpu_variant.py (gfx950).  Plain torch,
device-agnostic; not a test file.

The operation count n of a result, read off the kernels' own chains (u = 2^-24, gamma_n = n u / (1 - n u), as in tests/decode_local.py):

    conv    output i of a (window, channel) is ONE chain in variant_conv_kernel: acc = fma(k[i - j], delta[j], acc) for j = 0 .. i starting from 0.f
            (i + 1 roundings, the products unrounded), then y = y_ref + acc (one), then y = fma(delta[i], fb, y) (one):
                |y - y64| <= gamma_(i + 3) (|y_ref| + sum_{j <= i} |k delta| + |fb delta_i|)                                      n_conv(i) = i + 3
            z on top of y: DL.post_bound's form (round_io(y), times x0, round_io) with E_y the line above.
    pre     x0 against sc64 of group 0 within sc_err; delta = float(round_io(c1 cv)) - float(vg_ref) against c1 cv - vg_ref within pre_fwd64's bound
            (sc_err propagated, one fp32 rounding of the product) + half_ulp_io of the product + one fp32 rounding of the difference.

Operands are DL's "flat" family (|k|, |delta| in [0.5, 1], y_ref and fb in [1, 2], x0 in [0.5, 1], random signs), so a lost or doubled term moves an
output by more than its bound: the conv runner asserts margin < 1 in fp32, where no output rounding hides a term.  Every case runs as it is and with
y_ref = 0, so that the Toeplitz sum stands alone.  Poison: x0, delta, z NaN before every call, the padding columns of x and of k NaN, a tail value
whose position lies before 0 NaN; where a window is clipped by the sequence's end the rows behind the valid ones hold SENTINEL."""
import torch

from tests import decode_local as DL
from tests import shell_local as SL
from tests.decode_local import NAN, _Stats, _min_nonzero, flat, same_bits
from tests.shell_local import DTYPES, NAME, SENTINEL, U, gamma, half_ulp_io, sc64, sc_err  # noqa: F401  (DTYPES, NAME: the test files' ids)

TMAX = 1024
KERNEL_SHAPES = [(1, 3, 1), (1, 3, 2), (2, 5, 3), (3, 8, 63), (3, 8, 64), (2, 8, 65), (1, 64, 257), (1, 4, 1024)]     # (M, D, T)
KERNEL_SHAPES_GPU = [(2, 256, 1024)]
PRE_POS = (0, 1, 2, 77)
TOL = 1e-5                                                                   # the project's cached-route-versus-forward figure, fp32
TOL_AUTOCAST = 2e-2                                                          # ... under bf16 autocast
OPERATOR_CASES = [(96, 8, 0, 96), (96, 8, 1, 30), (96, 8, 40, 20), (2100, 8, 1500, 64), (2100, 8, 2036, 64), (2100, 8, 2099, 64)]    # (L, D, pos, T)
OPERATOR_CASES_GPU = [(33000, 64, 20000, 128)]                               # the two-level long-convolution plan
VOCAB = 12


def case_id(c):
    return "-".join(str(x) for x in c)


def _P(x):
    return None if x is None else x.data_ptr()


def rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()


def n_conv(i):
    return i + 3


# ---- hyena_variant_conv -----------------------------------------------------------------------------------------------------------------------
def conv_ref(k64, d64, y64, fb64):
    """k64 (D, T), d64 / y64 (M, D, T), fb64 (D,) or None -> (y, A) (M, D, T): the fp64 value of y_ref + the causal product + fb delta and the sum
    of the magnitudes of its terms; at most 2^24 products at a time"""
    M, D, T = d64.shape
    dev = d64.device
    i = torch.arange(T, device=dev)
    lag = i[:, None] - i[None, :]                                              # (i, j): the tap of output i and input j
    ok = (lag >= 0).double()
    lag = lag.clamp_min(0)
    y, A = y64.clone(), y64.abs()
    step = max(1, (1 << 24) // (T * T))
    for d0 in range(0, D, step):
        km = k64[d0:d0 + step][:, lag] * ok                                    # (dd, T, T)
        y[:, d0:d0 + step] += torch.einsum("dij,mdj->mdi", km, d64[:, d0:d0 + step])
        A[:, d0:d0 + step] += torch.einsum("dij,mdj->mdi", km.abs(), d64[:, d0:d0 + step].abs())
    if fb64 is not None:
        y += fb64[None, :, None] * d64
        A += (fb64[None, :, None] * d64).abs()
    return y, A


def conv_operands(M, D, Tn, T, dev, seed, zero_y=False, with_fb=True, zero_delta=False):
    g = torch.Generator().manual_seed(seed)
    kv = flat((D, Tn), g, torch.float32, dev)
    delta = flat((M, D, Tn), g, torch.float32, dev)
    y_ref = flat((M, D, Tn), g, torch.float32, dev, 1.0, 2.0)
    fb = flat((D,), g, torch.float32, dev, 1.0, 2.0) if with_fb else None
    x0 = flat((M, Tn, D), g, torch.float32, dev)
    if zero_y:
        y_ref.zero_()
    if zero_delta:
        delta.zero_()
    k = torch.full((D, Tn + 4), NAN, device=dev)                              # pitched rows: the columns past T are never read
    k[:, :Tn] = kv
    return k, delta, y_ref, fb, x0


def call_conv(_lib, dev, T, k, delta, y_ref, fb, x0):
    M, D, Tn = delta.shape
    z = torch.full((M, Tn, D), NAN, dtype=T, device=dev)
    ins = [k, delta, y_ref, x0] + ([fb] if fb is not None else [])
    keep = [x.clone() for x in ins]
    with _lib._backend.guard(dev):
        _lib.check(_lib.lib().hyena_variant_conv(_P(y_ref), _P(delta), _P(k), k.stride(0), _P(fb), _P(x0), _P(z), M, D, Tn, _lib.dtype_code(T),
                                                 _lib._backend.stream(dev)))
    assert all(same_bits(a, b) for a, b in zip(ins, keep)), "conv wrote one of its inputs"
    return z


def run_conv(_lib, dev, T, M, D, Tn, zero_y=False, with_fb=True, seed=0, label=""):
    """one call of hyena_variant_conv: every z within post_bound of y64 x0 with E_y = gamma_(i + 3) A; fp32: the bound below the smallest term"""
    k, delta, y_ref, fb, x0 = conv_operands(M, D, Tn, T, dev, seed, zero_y, with_fb)
    z = call_conv(_lib, dev, T, k, delta, y_ref, fb, x0)
    assert bool(torch.isfinite(z).all()), "z is not finite: something outside the window's own rows was read"
    y64, A = conv_ref(k[:, :Tn].double(), delta.double(), y_ref.double(), None if fb is None else fb.double())
    nc = (n_conv(torch.arange(Tn, device=dev)) - 1).double()[None, None, :]      # post_bound takes gamma_(nc + 1)
    x64 = x0.double().transpose(1, 2)                                              # (M, D, T)
    bound = DL.post_bound(y64, A, nc, x64, T)
    st = _Stats()
    st.hold("conv", z.transpose(1, 2), y64 * x64, bound)
    small = _min_nonzero(k[:, :Tn]) * _min_nonzero(delta)
    if fb is not None:
        small = min(small, _min_nonzero(fb) * _min_nonzero(delta))
    if not zero_y:
        small = min(small, _min_nonzero(y_ref))
    st["margin"] = float((bound / (x64.abs() * small)).max())                     # a lost term moves z by at least |x0| small
    print(st.line(f"{label} variant_conv {NAME[T]} M={M} D={D} T={Tn} y0={int(zero_y)} fb={int(with_fb)}"), flush=True)
    if T == torch.float32:
        assert st["margin"] < 1.0, ("the bound exceeds the effect of the smallest single term", st["margin"])
    return st, z


def run_conv_zero_delta(_lib, dev, T, M, D, Tn, seed=0):
    """delta == 0: z == round_io(round_io(y_ref) x0) exactly"""
    k, delta, y_ref, fb, x0 = conv_operands(M, D, Tn, T, dev, seed, zero_delta=True)
    z = call_conv(_lib, dev, T, k, delta, y_ref, fb, x0)
    want = (y_ref.to(T).float().transpose(1, 2) * x0).to(T)
    assert torch.equal(z, want), "delta == 0 does not give round(round(y_ref) x0)"


# ---- hyena_variant_pre ------------------------------------------------------------------------------------------------------------------------
def pre_operands(M, D, Tn, T, dev, pos, seed, bias=True):
    """X (3D, M, 2 + Tn): positions pos - 2, pos - 1, then the window; the tail NaN where its position lies before 0"""
    g = torch.Generator().manual_seed(seed)
    w, b_, bin_ = SL._params(3 * D, g, dev, bias)
    X = SL._operand((3 * D, M, 2 + Tn), g, T, dev)
    vg_ref = SL._operand((M, D, Tn), g, T, dev)
    tail = torch.empty(3 * D, M, 2, device=dev)
    for m in range(M):
        tail[:, m, 0] = X[:, m, 0].float() if pos[m] >= 2 else NAN
        tail[:, m, 1] = X[:, m, 1].float() if pos[m] >= 1 else NAN
    ldx = 3 * D + 5
    x = torch.full((M, Tn, ldx), NAN, dtype=T, device=dev)
    x[:, :, :3 * D] = X[:, :, 2:].permute(1, 2, 0)
    posb = torch.tensor(list(pos), dtype=torch.int32, device=dev)
    return X, x, ldx, w, b_, bin_, tail, posb, vg_ref


def call_pre(_lib, dev, T, x, ldx, w, b_, bin_, tail, posb, vg_ref):
    M, D, Tn = vg_ref.shape
    x0 = torch.full((M, Tn, D), NAN, device=dev)
    delta = torch.full((M, D, Tn), NAN, device=dev)
    ins = [x, w, b_, tail, posb, vg_ref] + ([bin_] if bin_ is not None else [])
    keep = [t.clone() for t in ins]
    with _lib._backend.guard(dev):
        _lib.check(_lib.lib().hyena_variant_pre(_P(x), ldx, _P(bin_), _P(w), _P(b_), _P(tail), _P(posb), _P(vg_ref), _P(x0), _P(delta), M, D, Tn,
                                                _lib.dtype_code(T), _lib._backend.stream(dev)))
    assert all(same_bits(a, c) for a, c in zip(ins, keep)), "pre wrote one of its inputs"
    return x0, delta


def run_pre(_lib, dev, T, M, D, Tn, pos, bias=True, seed=0, label=""):
    """one call of hyena_variant_pre with ldx = 3D + 5: x0 and delta within their bounds at every window position, for every row's own pos"""
    X, x, ldx, w, b_, bin_, tail, posb, vg_ref = pre_operands(M, D, Tn, T, dev, pos, seed, bias)
    x0, delta = call_pre(_lib, dev, T, x, ldx, w, b_, bin_, tail, posb, vg_ref)
    assert bool(torch.isfinite(x0).all()) and bool(torch.isfinite(delta).all()), "a value in front of position 0 (or a padding column) was used"
    w64, b64, bin64 = w.double(), b_.double(), None if bin_ is None else bin_.double()
    st = _Stats()
    for m in range(M):
        off = min(int(pos[m]), 2)                                              # sc64 pads with zeros before its first column: position 0
        xin = X[:, m:m + 1, 2 - off:].double()
        vg64, Evg = SL.pre_fwd64(xin, bin64, w64, b64, xin.shape[-1])          # (1, D, off + Tn)
        c0 = sc64(xin[:D], None if bin64 is None else bin64[:D], w64[:D], b64[:D])[:, 0, off:]               # (D, Tn)
        e0 = sc_err(xin[:D], None if bin64 is None else bin64[:D], w64[:D], b64[:D])[:, 0, off:]
        st.hold("pre.x0", x0[m].t(), c0, e0)
        v, E = vg64[0, :, off:], Evg[0, :, off:]
        E = E + half_ulp_io(v.abs() + E, T)                                    # round_io of the product
        ref = v - vg_ref[m].double()
        st.hold("pre.delta", delta[m], ref, E + U * (ref.abs() + E))           # ... and one fp32 rounding of the difference
    print(st.line(f"{label} variant_pre {NAME[T]} M={M} D={D} T={Tn} pos={tuple(pos)} bin={int(bias)}"), flush=True)
    return st


def suite_kernels(_lib, dev, T, M, D, Tn, label):
    """5.1: one (M, D, T) shape -- conv as it is and with y_ref = 0 (with and without fb), pre at every position of PRE_POS"""
    seed = 1000 * M + 10 * D + Tn
    run_conv(_lib, dev, T, M, D, Tn, seed=seed, label=label)
    run_conv(_lib, dev, T, M, D, Tn, zero_y=True, seed=seed + 1, label=label)
    run_conv(_lib, dev, T, M, D, Tn, zero_y=True, with_fb=False, seed=seed + 2, label=label)
    for j, p in enumerate(PRE_POS):
        pos = [PRE_POS[(j + m) % len(PRE_POS)] for m in range(M)]             # the rows of one call stand at different positions
        run_pre(_lib, dev, T, M, D, Tn, pos, bias=j % 2 == 0, seed=seed + 3 + j, label=label)


def run_row_independence(_lib, dev, T, D=6, Tn=37, seed=5):
    """5.2: M = 5 windows at once against each window alone, through the _lib wrappers: x0, delta, z bit for bit"""
    M = 5
    pos = [0, 1, 2, 77, 5]
    X, x, ldx, w, b_, bin_, tail, posb, vg_ref = pre_operands(M, D, Tn, T, dev, pos, seed)
    x3 = x[:, :, :3 * D].contiguous()
    tail = torch.nan_to_num(tail, nan=SENTINEL)                               # (the wrappers take the tail as it is; a value before 0 is never used)
    k, _, y_ref, fb, _ = conv_operands(M, D, Tn, T, dev, seed + 1)
    k = k[:, :Tn]

    def both(sl):
        m = sl.stop - sl.start
        x0 = torch.full((m, Tn, D), NAN, device=dev)
        delta = torch.full((m, D, Tn), NAN, device=dev)
        z = torch.full((m, Tn, D), NAN, dtype=T, device=dev)
        assert _lib.variant_pre(x3[sl].contiguous(), bin_, w, b_, tail[:, sl].contiguous(), posb[sl].contiguous(), vg_ref[sl].contiguous(), x0,
                                delta) == TMAX
        assert _lib.variant_conv(y_ref[sl].contiguous(), delta, k, fb, x0, z) == TMAX
        return x0, delta, z
    all_ = both(slice(0, M))
    for m in range(M):
        one = both(slice(m, m + 1))
        for a, b, name in zip(all_, one, ("x0", "delta", "z")):
            assert torch.equal(a[m:m + 1], b), (name, m)


def check_bad_arguments(_lib, dev):
    L = _lib.lib()
    t = torch.zeros(64, device=dev)
    p = t.data_ptr()
    assert L.hyena_variant_pre(None, 12, None, None, None, None, None, None, None, None, 1, 4, 8, 0, None) == 1
    assert L.hyena_variant_conv(None, None, None, 8, None, None, None, 1, 4, 8, 0, None) == 1
    for M, D, Tn, ldx, ldk, code in ((0, 1, 1, 3, 1, 0), (1, 0, 1, 3, 1, 0), (1, 1, 0, 3, 1, 0), (1, 1, TMAX + 1, 3, TMAX + 1, 0),
                                     (1, 1, 1, 3, 1, 7), (1, 65536, 1, 3 * 65536, 1, 0)):
        assert L.hyena_variant_pre(p, ldx, None, p, p, p, p, p, p, p, M, D, Tn, code, None) == 1, (M, D, Tn, ldx, code)
        assert L.hyena_variant_conv(p, p, p, ldk, None, p, p, M, D, Tn, code, None) == 1, (M, D, Tn, ldk, code)
    assert L.hyena_variant_pre(p, 2, None, p, p, p, p, p, p, p, 1, 1, 1, 0, None) == 1                # ldx < 3D
    assert L.hyena_variant_conv(p, p, p, 3, None, p, p, 1, 1, 4, 0, None) == 1                      # ldk < T


# ---- HyenaOperator --------------------------------------------------------------------------------------------------------------------------
def _layer(l_max, **kw):
    d = dict(l_max=l_max, order=2, filter_order=64, emb_dim=5, short_filter_order=3, modulate=True, w=10, lr=6e-4, wd=0.0, lr_pos_emb=0.0)
    d.update(kw)
    return d


def run_operator(dev, L, D, pos, Tn, label=""):
    """5.4: the window route against the operator's own forward over the edited input (every row from pos on replaced): relative l2 < 1e-5 over
    the window's rows inside the sequence; the reference phase's output is the plain forward's, bit for bit; the rows of a clipped window behind
    the sequence's end hold SENTINEL"""
    from hyena_dna_amd.hyena import HyenaOperator
    from hyena_dna_amd.variants import EditWindowParams
    torch.manual_seed(L + D + pos)
    op = HyenaOperator(d_model=D, **_layer(L + 3)).to(dev)
    u = torch.randn(1, L, D, device=dev)
    ua = u.clone()
    ua[:, pos:] = torch.randn(1, L - pos, D, device=dev)
    n = min(Tn, L - pos)
    win = torch.full((1, Tn, D), SENTINEL, device=dev)
    win[:, :n] = ua[:, pos:pos + n]
    with torch.no_grad():
        full, plain = op(ua), op(u)
        ew = EditWindowParams(torch.tensor([pos], device=dev), None, Tn)
        assert torch.equal(op(u, inference_params=ew), plain), "the reference phase is not the plain forward"
        ew.phase = "window"
        got = op(win, inference_params=ew)
    assert got.shape == (1, Tn, D) and bool(torch.isfinite(got[:, :n]).all())
    r, away = rel(got[:, :n], full[:, pos:pos + n]), rel(plain[:, pos:pos + n], full[:, pos:pos + n])
    print(f"[variant] {label} operator L={L} D={D} pos={pos} T={Tn} rel={r:.3g} reference_is_away_by={away:.3g}", flush=True)
    assert r < TOL, r
    assert away > 50 * TOL, "the edit does not move the operator's output: the case shows nothing"


# ---- HyenaDNALM -----------------------------------------------------------------------------------------------------------------------------
def lm(dev, L, d=64, n_layer=2, seed=0, **kw):
    from hyena_dna_amd.lm import HyenaDNALM
    torch.manual_seed(seed)
    m = HyenaDNALM(d_model=d, n_layer=n_layer, d_inner=4 * d, vocab_size=VOCAB, layer=_layer(L + 2), resid_dropout=0.0, embed_dropout=0.1,
                   pad_vocab_size_multiple=8, fused_dropout_add_ln=True, residual_in_fp32=True, **kw)
    return m.to(dev).eval()


def ref_ids(L, dev, seed=1, G=1):
    return torch.randint(7, 11, (G, L), generator=torch.Generator().manual_seed(seed)).to(dev)


def snvs(ref, positions):
    """all 3 alternative bases at every position of row 0 -> positions (M,), alts (M,)"""
    pos, alts = [], []
    for p in positions:
        for a in range(7, 11):
            if a != int(ref[0, p]):
                pos.append(p)
                alts.append(a)
    return torch.tensor(pos, device=ref.device), torch.tensor(alts, device=ref.device)


def _ctx(autocast_dev):
    return torch.autocast(autocast_dev, dtype=torch.bfloat16) if autocast_dev else torch.autocast("cpu", enabled=False)


def edited_forwards(m, ref, pos, alts, autocast_dev=None, groups=None):
    """the full forwards of the M edited sequences, four at a time -> (M, L, V) fp32"""
    M = pos.shape[0]
    g = torch.zeros_like(pos) if groups is None else groups
    seqs = ref[g].clone()
    seqs[torch.arange(M, device=ref.device), pos] = alts
    with torch.no_grad(), _ctx(autocast_dev):
        return torch.cat([m(seqs[i:i + 4])[0].logits.float() for i in range(0, M, 4)], dim=0)


def run_model_windows(dev, L, positions, Tn, tol, autocast_dev=None, d=64, label=""):
    """5.5: forward_edited_windows over all 3 alternative bases at `positions` against the full forwards of the edited sequences, per variant over
    the window's rows inside the sequence; rows past the end are zeros; ref_logits is the cached prefill's logits bit for bit"""
    from hyena_dna_amd.inference import InferenceParams
    m = lm(dev, L, d=d)
    ref = ref_ids(L, dev)
    pos, alts = snvs(ref, positions)
    M = pos.shape[0]
    idx = (pos[:, None] + torch.arange(Tn, device=dev)[None, :])
    window = ref[0][idx.clamp(max=L - 1)]
    window[:, 0] = alts
    window[idx >= L] = 0                                                     # (any valid id: those rows are dropped)
    with _ctx(autocast_dev):
        ref_logits, logits = m.forward_edited_windows(ref, pos, window)
        with torch.no_grad():
            ip = InferenceParams(max_seqlen=L, max_batch_size=1)
            ip.key_value_memory_dict = m.allocate_inference_cache(1, L)
            prefill = m(ref, inference_params=ip)[0].logits
    assert torch.equal(ref_logits, prefill), "ref_logits is not the cached prefill's logits"
    full = edited_forwards(m, ref, pos, alts, autocast_dev)
    worst = 0.0
    for i in range(M):
        n = min(Tn, L - int(pos[i]))
        worst = max(worst, rel(logits[i, :n], full[i, int(pos[i]):int(pos[i]) + n]))
        assert bool((logits[i, n:] == 0).all()), "a row past the sequence's end is not zero"
    print(f"[variant] {label} model L={L} M={M} T={Tn} worst_rel={worst:.3g}", flush=True)
    assert worst < tol, worst


def run_long_conv_carries(dev, L, p, label=""):
    """5.6: at window offsets [3, 35) the short convolution no longer sees an SNV.  The two full forwards must differ there by more than 50 x the
    tolerance (a condition on the inputs), the window logits must match the edited forward within the tolerance"""
    m = lm(dev, L)
    ref = ref_ids(L, dev)
    pos = torch.tensor([p], device=dev)
    alts = (ref[0, pos] - 7 + 1) % 4 + 7                                      # the next base
    Tn = 35
    window = ref[0][(pos[:, None] + torch.arange(Tn, device=dev)[None, :]).clamp(max=L - 1)]
    window[:, 0] = alts
    ref_logits, logits = m.forward_edited_windows(ref, pos, window)
    full = edited_forwards(m, ref, pos, alts)
    with torch.no_grad():
        base = m(ref)[0].logits.float()
    rows = slice(p + 3, p + 35)
    moved, r = rel(base[0, rows], full[0, rows]), rel(logits[0, 3:35], full[0, rows])
    print(f"[variant] {label} long-conv L={L} pos={p} moved={moved:.3g} rel={r:.3g}", flush=True)
    assert moved > 50 * TOL, ("the edit does not reach offsets [3, 35) through the long convolution: the inputs show nothing", moved)
    assert r < TOL, r


def scores_from_full(ref, base, full, pos, alts, Tn, V):
    """site, downstream, llr, complete and the per-entry bounds from full-forward logits: base (1, L, Vall) of the reference, full (M, L, Vall) of
    the edited sequences.  bound = 2 tol (||alt logit row||_2 + ||ref logit row||_2) per entry, check_greedy_against_forward's form"""
    M, L = pos.shape[0], ref.shape[1]
    dev = ref.device
    idx = pos[:, None] + torch.arange(Tn + 1, device=dev)[None, :]
    tok = ref[0][idx.clamp(max=L - 1)]                                         # ref[p + j]
    rrow = base[0][(idx - 1).clamp(max=L - 1)][..., :V]                        # reference rows p - 1 ... p + T - 1
    arow = full[torch.arange(M, device=dev)[:, None], (idx[:, :Tn]).clamp(max=L - 1)][..., :V]      # edited rows p ... p + T - 1
    lr, la = torch.log_softmax(rrow.double(), -1), torch.log_softmax(arow.double(), -1)
    site = (lr[:, 0].gather(-1, alts[:, None]) - lr[:, 0].gather(-1, tok[:, :1])).squeeze(-1)
    nxt = tok[:, 1:, None]
    live = idx[:, 1:] <= L - 1
    down = (la.gather(-1, nxt) - lr[:, 1:].gather(-1, nxt)).squeeze(-1) * live
    b_site = 2 * 2 * rrow[:, 0].double().norm(dim=-1)
    b_down = 2 * (arow.double().norm(dim=-1) + rrow[:, 1:].double().norm(dim=-1)) * live
    return site, down, site + down.sum(-1), pos + Tn >= L - 1, b_site, b_down


def run_scores(dev, L, positions, Tn, tol, label=""):
    """5.7: score_variants against the same formulas on full-forward logits within the per-entry bound; `complete`; chunking with max_window_tokens
    within the same bound; saturation_mutagenesis' reference entries exactly 0 and its other entries score_variants' bit for bit"""
    m = lm(dev, L)
    ref = ref_ids(L, dev)
    pos, alts = snvs(ref, positions)
    V = VOCAB
    got = m.score_variants(ref, pos, alts, horizon=Tn, vocab_size=V)
    with torch.no_grad():
        base = m(ref)[0].logits.float()
    full = edited_forwards(m, ref, pos, alts)
    site, down, llr, complete, b_site, b_down = scores_from_full(ref, base, full, pos, alts, Tn, V)
    assert got.site.shape == (pos.shape[0],) and got.downstream.shape == (pos.shape[0], Tn) and got.llr.shape == (pos.shape[0],)
    assert torch.equal(got.complete, complete) and got.complete.dtype == torch.bool
    e_site, e_down, e_llr = (got.site - site).abs(), (got.downstream - down).abs(), (got.llr - llr).abs()
    print(f"[variant] {label} scores L={L} T={Tn} site={float((e_site / b_site).max()):.3g} x tol-bound "
          f"down={float((e_down / b_down.clamp_min(1e-30)).max()):.3g} llr_err={float(e_llr.max()):.3g}", flush=True)
    assert bool((e_site <= tol * b_site).all()) and bool((e_down <= tol * b_down).all())
    assert bool((e_llr <= tol * (b_site + b_down.sum(-1))).all())
    assert bool((got.downstream[(pos[:, None] + torch.arange(Tn, device=dev)[None, :] + 1) > L - 1] == 0).all())
    chunked = m.score_variants(ref, pos, alts, horizon=Tn, vocab_size=V, max_window_tokens=5 * Tn)
    assert bool(((chunked.site - site).abs() <= tol * b_site).all()) and bool(((chunked.downstream - down).abs() <= tol * b_down).all())
    assert bool(((chunked.llr - llr).abs() <= tol * (b_site + b_down.sum(-1))).all()) and torch.equal(chunked.complete, complete)
    return m, ref


def run_saturation(dev, L, start, stop, Tn):
    m = lm(dev, L)
    ref = ref_ids(L, dev)
    alphabet = (7, 8, 9, 10)
    sat = m.saturation_mutagenesis(ref[0], start, stop, alphabet=alphabet, horizon=Tn, vocab_size=VOCAB)
    assert sat.shape == (stop - start, 4) and sat.dtype == torch.float32
    pos = torch.arange(start, stop, device=dev).repeat_interleave(4)
    alts = torch.tensor(alphabet, device=dev).repeat(stop - start)
    llr = m.score_variants(ref, pos, alts, horizon=Tn, vocab_size=VOCAB).llr.view(stop - start, 4)
    is_ref = (alts == ref[0][pos]).view(stop - start, 4)
    assert bool((is_ref.sum(-1) == 1).all())
    assert bool((sat[is_ref] == 0).all()), "the reference base's entry is not exactly 0"
    assert torch.equal(sat[~is_ref], llr[~is_ref]), "an entry differs from score_variants'"
    assert bool((sat[~is_ref] != 0).all())


# ---- refusals: (message, call) pairs; every one raises before any allocation -------------------------------------------------------------------
def refusal_cases(dev):
    from hyena_dna_amd.hyena import HyenaOperator
    from hyena_dna_amd.lm import HyenaDNALM
    from hyena_dna_amd.variants import EditWindowParams
    L = 40
    m = lm(dev, L)
    ref = ref_ids(L, dev)
    pos, alts = torch.tensor([5, 9], device=dev), torch.tensor([7, 8], device=dev)
    win = ref[0][pos[:, None] + torch.arange(4, device=dev)[None, :]]

    def lm_with(**layer_kw):
        torch.manual_seed(0)
        return HyenaDNALM(d_model=16, n_layer=1, d_inner=32, vocab_size=VOCAB, layer=_layer(L + 2, **layer_kw), pad_vocab_size_multiple=8,
                          fused_dropout_add_ln=True, residual_in_fp32=True).to(dev).eval()

    def learned_positions():
        torch.manual_seed(0)
        mm = HyenaDNALM(d_model=16, n_layer=1, d_inner=32, vocab_size=VOCAB, layer=_layer(L + 2), max_position_embeddings=L + 2,
                        pad_vocab_size_multiple=8, fused_dropout_add_ln=True, residual_in_fp32=True).to(dev).eval()
        mm.score_variants(ref, pos, alts)

    def window_before_reference():
        op = HyenaOperator(d_model=8, **_layer(64)).to(dev)
        ew = EditWindowParams(pos[:1], None, 4)
        ew.phase = "window"
        with torch.no_grad():
            op(torch.randn(1, 4, 8, device=dev), inference_params=ew)

    def with_grad():
        op = HyenaOperator(d_model=8, **_layer(64)).to(dev)
        op(torch.randn(1, 16, 8, device=dev), inference_params=EditWindowParams(pos[:1], None, 4))

    other = torch.device("meta")
    return [
        ("learned position embeddings", NotImplementedError, learned_positions),
        ("horizon=0", ValueError, lambda: m.score_variants(ref, pos, alts, horizon=0)),
        ("horizon=1025", ValueError, lambda: m.score_variants(ref, pos, alts, horizon=TMAX + 1)),
        ("window_tokens' T=1025", ValueError, lambda: m.forward_edited_windows(ref, pos, ref[:, :1].expand(2, TMAX + 1))),
        ("positions hold entries outside", ValueError, lambda: m.score_variants(ref, torch.tensor([5, L], device=dev), alts)),
        ("positions hold entries outside", ValueError, lambda: m.forward_edited_windows(ref, torch.tensor([-1, 3], device=dev), win)),
        ("position 0 has no context", ValueError, lambda: m.score_variants(ref, torch.tensor([0, 3], device=dev), alts)),
        ("alts hold token ids outside", ValueError, lambda: m.score_variants(ref, pos, torch.tensor([7, VOCAB], device=dev), vocab_size=VOCAB)),
        ("groups hold entries outside", ValueError, lambda: m.score_variants(ref, pos, alts, groups=torch.tensor([0, 1], device=dev))),
        ("groups is required", ValueError, lambda: m.score_variants(ref.expand(2, L), pos, alts)),
        ("vocab_size=99", ValueError, lambda: m.score_variants(ref, pos, alts, vocab_size=99)),
        ("positions has to be", ValueError, lambda: m.score_variants(ref, pos.to(torch.int32), alts)),
        ("alts has to be", ValueError, lambda: m.score_variants(ref, pos, alts.to(torch.int32))),
        ("ref_ids has to be", ValueError, lambda: m.score_variants(ref.to(torch.int32), pos, alts)),
        ("window_tokens has to be", ValueError, lambda: m.forward_edited_windows(ref, pos, win.to(torch.int32))),
        ("positions live on", ValueError, lambda: m.score_variants(ref, pos.to(other), alts)),
        ("groups has to be", ValueError, lambda: m.score_variants(ref, pos, alts, groups=torch.zeros(2, dtype=torch.int64, device=other))),
        ("max_window_tokens=0", ValueError, lambda: m.forward_edited_windows(ref, pos, win, max_window_tokens=0)),
        ("start=0", ValueError, lambda: m.saturation_mutagenesis(ref[0], 0, 4)),
        ("one reference", ValueError, lambda: m.saturation_mutagenesis(ref, 1, 4)),
        ("order-2", NotImplementedError, lambda: lm_with(order=3).score_variants(ref, pos, alts)),
        ("causal", NotImplementedError, lambda: lm_with(bidirectional=True).score_variants(ref, pos, alts)),
        ("fused", NotImplementedError, lambda: lm_with(num_heads=2).score_variants(ref, pos, alts)),
        ("max_seqlen", ValueError, lambda: m.score_variants(ref_ids(L + 3, dev), pos, alts)),
        ("after its reference phase", ValueError, window_before_reference),
        ("inference only", ValueError, with_grad),
        ("an edited window holds", ValueError, lambda: EditWindowParams(pos, None, TMAX + 1)),
    ]


REFUSAL_MESSAGES = ["learned position embeddings", "horizon=0", "horizon=1025", "window_tokens' T=1025", "positions hold entries outside",
                    "positions hold entries outside", "position 0 has no context", "alts hold token ids outside", "groups hold entries outside",
                    "groups is required", "vocab_size=99", "positions has to be", "alts has to be", "ref_ids has to be", "window_tokens has to be",
                    "positions live on", "groups has to be", "max_window_tokens=0", "start=0", "one reference", "order-2", "causal", "fused",
                    "max_seqlen", "after its reference phase", "inference only", "an edited window holds"]          # refusal_cases' messages, in its order
