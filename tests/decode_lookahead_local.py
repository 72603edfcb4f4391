"""fp64 references and derived bounds for the lookahead carry of csrc/decode_kernels.h (hyena_decode_carry, _conv_la, _post_la), the cache that
runs on it (HyenaDecodeState(lookahead=W)) and the model on top.  Shared by tests/test_decode_lookahead_emu.py (CPU emulation) and
tests/test_gpu_decode_lookahead.py (gfx950).  Plain torch, device-agnostic; not a test file.

The operation count n of a result, from the kernels' own chains (u = 2^-24, gamma_n = n u / (1 - n u), as in tests/decode_local.py):

    carry   a chunk's partial is decode_conv_block_kernel's chain, kept as it is: 32 FMAs of a lane (DEC_NV DEC_V, the product unrounded) + 6
            butterfly steps + the two levels of (r0 + r1) + (r2 + r3) = 40 = DL.N_CONV.  decode_carry_reduce_kernel then adds the nc = ceil(t0 /
            8192) partials in chunk order starting from 0.f: the first addition is exact, each further chunk is one rounding.
                |carry - ref64| <= gamma_(40 + max(nc - 1, 0)) sum_{s < t0} |k vg|                                            n_carry(t0)
            History columns at and past t0 enter as exact zeros (the VALUE is selected): they hold SENTINEL here and may hold anything.
    step    decode_conv_la_kernel keeps decode_conv_kernel's chain (40) for each of the nl = t // 8192 - base // 8192 + 1 live chunks (1 or 2).
            decode_post_la_kernel starts from the carry and adds the nl partials in chunk order, then fma(vg_t, fb, y): nl + 1 roundings on top
            of the carry's n_carry(base), and no term has more behind it.
                |y - y64| <= gamma_(n_carry(base) + nl + 1) (sum_{s <= t} |k vg| + |fb vg_t|)                                  n_step(base, t)
            z on top of y: DL.post_bound's form (round_io(y), times x0, round_io), with E_y the line above.
    With base = 0 and a zero carry the step IS decode_conv + decode_post (0.f + p is exact, same lanes, same order): torch.equal.

Operands are DL's "flat" family (|k|, |vg| in [0.5, 1], random signs), so a lost or doubled term moves a carry by more than its bound: the
carry runner asserts margin < 1 (the step runner in fp32, where no output rounding hides a term).  Poison: carry, partials, z (and x0 where it
is not read) NaN before every call; the history at and past t0 SENTINEL for the carry; for a step real values up to t, SENTINEL in (t, t | 7],
NaN beyond; k NaN past the last tap the header allows."""
import torch

from tests import decode_local as DL
from tests.decode_local import CHUNK, NAN, N_CONV, _Stats, _bits, _ceil, _min_nonzero, conv_ref, flat, same_bits
from tests.shell_local import DTYPES, NAME, SENTINEL, gamma  # noqa: F401  (DTYPES, NAME: the test files' ids)

TMAX = 64
LCAP3 = 3 * CHUNK + 64                                                     # the largest cache of the kernel cases


def n_carry(t0):
    return N_CONV + max(-(-t0 // CHUNK) - 1, 0)


def n_step(base, t):
    return n_carry(base) + (t // CHUNK - base // CHUNK + 1) + 1


def _P(x):
    return None if x is None else x.data_ptr()


def _operands(B, D, Lcap, seed, T, dev):
    g = torch.Generator().manual_seed(seed)
    kv = flat((D, Lcap), g, torch.float32, dev)
    h = flat((B, D, Lcap), g, T, dev)
    return g, kv, h


def _k_buffer(kv, last, dev):
    """(D, ldk) with ldk = ceil4(Lcap) + 4: the taps 0 .. last, NaN beyond"""
    D, Lcap = kv.shape
    k = torch.full((D, _ceil(Lcap, 4) + 4), NAN, device=dev)
    k[:, :last + 1] = kv[:, :last + 1]
    return k


def causal_ref(k64, h64, t0, n, lo=0, hi=None):
    """ref, S (B, n, D): the fp64 sums of k[d, t0 + i - s] h[b, d, s] and of their magnitudes over lo <= s < hi (default: all s <= t0 + i), chunk by chunk"""
    B, D, _ = h64.shape
    hi = t0 + n if hi is None else hi
    ref = torch.zeros(B, n, D, dtype=torch.float64, device=h64.device)
    S = torch.zeros_like(ref)
    for s0 in range(lo // CHUNK * CHUNK, hi, CHUNK):
        a, b = max(s0, lo), min(s0 + CHUNK, hi)
        if a < b:
            r, m = conv_ref(k64, h64[:, :, a:b], t0, n, a)
            ref += r
            S += m
    return ref, S


# ---- hyena_decode_carry ----------------------------------------------------------------------------------------------------------------------
def run_carry(_lib, dev, T, B, D, Lcap, t0, W, seed=0, label=""):
    """one call of hyena_decode_carry.  carry[:, j] within gamma_(n_carry) sum|k vg| of the fp64 sum over s < t0 for j < min(W, Lcap - t0), the
    other slots bitwise the NaN they held, exactly 0 at t0 = 0; base = t0 afterwards; k, the history and pos unchanged.  -> (figures, carry)"""
    lib = _lib.lib()
    code, stream = _lib.dtype_code(T), _lib._backend.stream(dev)
    _, kv, h = _operands(B, D, Lcap, seed, T, dev)
    live = 0 <= t0 < Lcap
    Weff = min(W, Lcap - t0) if live else 0
    k = _k_buffer(kv, t0 + Weff - 1 if live else -1, dev)
    lda = _ceil(Lcap, 8)
    vg = torch.full((B, D, lda), SENTINEL, dtype=T, device=dev)            # at and past t0: large, finite, and not to enter the sum
    vg[:, :, :max(min(t0, Lcap), 0)] = h[:, :, :max(min(t0, Lcap), 0)]
    nfl = lib.hyena_decode_carry_partial_floats(B, D, Lcap, W)
    assert nfl == -(-Lcap // CHUNK) * B * W * D
    part = torch.full((nfl,), NAN, device=dev)
    carry = torch.full((B, W, D), NAN, device=dev)
    pos = torch.tensor([t0], dtype=torch.int32, device=dev)
    base = torch.tensor([-7], dtype=torch.int32, device=dev)
    ins = [k, vg, pos]
    keep = [x.clone() for x in ins]
    with _lib._backend.guard(dev):
        _lib.check(lib.hyena_decode_carry(_P(k), k.stride(0), _P(vg), _P(part), _P(carry), _P(pos), _P(base), B, D, Lcap, lda, W, code, stream))
    assert all(same_bits(a, b) for a, b in zip(ins, keep)), "carry wrote one of its inputs (or pos)"
    assert base.item() == (t0 if live else -7), ("base", base.item(), t0)
    st = _Stats()
    assert bool(torch.isnan(carry[:, Weff:]).all()), "a carry slot past the cache's end (or of a parked call) was written"
    if Weff:
        got = carry[:, :Weff]
        assert bool(torch.isfinite(got).all()), "a carry slot the header names is not finite"
        ref, S = causal_ref(k.double(), h.double(), t0, Weff, 0, t0)
        bound = gamma(n_carry(t0)) * S
        st.hold("carry", got, ref, bound)
        if t0 == 0:
            assert bool((_bits(got) == 0).all()), "t0 = 0: the carry is not exactly +0"
            assert bool(torch.isnan(part).all()), "t0 = 0: a partial was written"
        else:
            small = _min_nonzero(kv[:, :t0 + Weff]) * _min_nonzero(h[:, :, :t0])
            st["margin"] = float(bound.max()) / small
    print(st.line(f"{label} carry {NAME[T]} B={B} D={D} Lcap={Lcap} t0={t0} W={W}"), flush=True)
    assert st.get("margin", 0.0) < 1.0, ("the bound exceeds the smallest single term: the case is too large to see a lost term", st["margin"])
    return st, carry


# ---- hyena_decode_conv_la + hyena_decode_post_la on a carry taken by hyena_decode_carry -----------------------------------------------------------
def run_steps(_lib, dev, T, B, D, Lcap, base, W, ts, with_fb=True, seed=0, label=""):
    """the carry at `base` (taken while the history from base on holds SENTINEL), then for every t of ts on its own: the history filled up to t,
    one call of conv_la and of post_la.  A t inside the window: z within DL.post_bound's form of y64 x0 with n_step(base, t), pos = t + 1.  A t
    outside it (t >= base + W, t >= Lcap): z, the partials, the history and pos bitwise as they were.  base never changes.  -> figures"""
    lib = _lib.lib()
    code, stream = _lib.dtype_code(T), _lib._backend.stream(dev)
    g, kv, h = _operands(B, D, Lcap, seed, T, dev)
    x0v = flat((B, D), g, torch.float32, dev)
    fb = flat((D,), g, torch.float32, dev, 1.0, 2.0) if with_fb else None
    lda = _ceil(Lcap, 8)
    k = _k_buffer(kv, Lcap - 1, dev)
    vg = torch.full((B, D, lda), SENTINEL, dtype=T, device=dev)
    vg[:, :, :base] = h[:, :, :base]
    carry = torch.full((B, W, D), NAN, device=dev)
    cpart = torch.full((lib.hyena_decode_carry_partial_floats(B, D, Lcap, W),), NAN, device=dev)
    pos = torch.tensor([base], dtype=torch.int32, device=dev)
    bas = torch.tensor([-7], dtype=torch.int32, device=dev)
    with _lib._backend.guard(dev):
        _lib.check(lib.hyena_decode_carry(_P(k), k.stride(0), _P(vg), _P(cpart), _P(carry), _P(pos), _P(bas), B, D, Lcap, lda, W, code, stream))
    assert bas.item() == base
    carry0 = carry.clone()
    k64, h64 = k.double(), h.double()
    st = _Stats()
    for t in ts:
        inside = 0 <= t < Lcap and 0 <= t - base < W
        vg.fill_(NAN)
        last = min(t, Lcap - 1)
        vg[:, :, :last + 1] = h[:, :, :last + 1]
        vg[:, :, last + 1:(last | 7) + 1] = SENTINEL
        part = torch.full((2, B, D), NAN, device=dev)
        x0 = x0v.clone() if inside else torch.full((B, D), NAN, device=dev)
        z = torch.full((B, D), SENTINEL, dtype=T, device=dev)
        pos.fill_(t)
        ins = [k, vg, x0, carry, bas] + ([fb] if with_fb else [])
        keep = [x.clone() for x in ins]
        with _lib._backend.guard(dev):
            _lib.check(lib.hyena_decode_conv_la(_P(k), k.stride(0), _P(vg), _P(part), _P(pos), _P(bas), B, D, Lcap, lda, W, code, stream))
            assert pos.item() == t, "conv_la moved the position"
            _lib.check(lib.hyena_decode_post_la(_P(part), _P(carry), _P(vg), _P(fb), _P(x0), _P(z), _P(pos), _P(bas), B, D, Lcap, lda, W, code,
                                                stream))
        assert all(same_bits(a, b) for a, b in zip(ins, keep)), "a step wrote one of its inputs (the history, the carry or base among them)"
        assert same_bits(carry, carry0)
        if not inside:
            assert pos.item() == t and bool((z == SENTINEL).all()) and bool(torch.isnan(part).all()), ("a parked step wrote something", t)
            continue
        assert pos.item() == t + 1, ("pos", pos.item(), t)
        nl = t // CHUNK - base // CHUNK + 1
        assert bool(torch.isfinite(part[:nl]).all()) and bool(torch.isnan(part[nl:]).all()), "the live partials, and no other slot"
        y64, A = causal_ref(k64, h64, t, 1)
        y64, A = y64[:, 0], A[:, 0]
        small = _min_nonzero(kv[:, :t + 1]) * _min_nonzero(h[:, :, :t + 1])
        if with_fb:
            f = fb.double()[None] * h64[:, :, t]
            y64, A, small = y64 + f, A + f.abs(), min(small, _min_nonzero(f))
        x64 = x0v.double()
        bound = DL.post_bound(y64, A, n_step(base, t) - 1.0, x64, T)      # (post_bound takes gamma_(its argument + 1))
        assert bool(torch.isfinite(z).all()), "z is not finite: something that is not to be read was read"
        st.hold("z_la", z, y64 * x64, bound)
        if T == torch.float32:
            st["margin"] = max(st.get("margin", 0.0), float((bound / (x64.abs() * small)).max()))
    print(st.line(f"{label} steps {NAME[T]} B={B} D={D} Lcap={Lcap} base={base} W={W} ts={tuple(ts)} fb={int(with_fb)}"), flush=True)
    assert st.get("margin", 0.0) < 1.0, ("the bound exceeds the effect of the smallest single term", st["margin"])
    return st


def run_parked_with_pre(_lib, dev, T, B, D, Lcap, base, W, seed=0):
    """the whole step (decode_pre, conv_la, post_la) at t = Lcap: the history, the tail, x0, z and pos bitwise as they were"""
    g, kv, h = _operands(B, D, Lcap, seed, T, dev)
    k = _k_buffer(kv, Lcap - 1, dev)
    vg = torch.zeros(B, D, _ceil(Lcap, 8), dtype=T, device=dev)
    vg[:, :, :Lcap] = h
    w, b_ = flat((3 * D, 3), g, torch.float32, dev), flat((3 * D,), g, torch.float32, dev)
    tail = flat((3 * D, B, 2), g, torch.float32, dev)
    x2 = flat((B, 3 * D), g, T, dev)
    x0 = torch.full((B, D), SENTINEL, device=dev)
    z = torch.full((B, D), SENTINEL, dtype=T, device=dev)
    part = torch.full((2, B, D), NAN, device=dev)
    carry = torch.zeros(B, W, D, device=dev)
    pos = torch.tensor([Lcap], dtype=torch.int32, device=dev)
    bas = torch.tensor([base], dtype=torch.int32, device=dev)
    state = [vg, tail, x0, z, part, carry, pos, bas]
    keep = [x.clone() for x in state]
    _lib.decode_pre(x2, None, w, b_, tail, vg, x0, pos, Lcap)
    _lib.decode_conv_la(k, vg, part, pos, bas, B, W, Lcap)
    _lib.decode_post_la(part, carry, vg, None, x0, z, pos, bas, B, Lcap)
    assert all(same_bits(a, b) for a, b in zip(state, keep)), "a step at t = Lcap wrote something"


def run_outside_window_with_pre(_lib, dev, T, B, D, Lcap, base, W, seed=0):
    """the whole step (decode_pre, conv_la, post_la) at t = base + W, inside the cache but past the window -- what a graph warm-up may issue.
    conv_la and post_la park: z, the partials, the carry, base and pos bitwise as they were.  decode_pre, used unchanged, knows nothing of
    the window (include/hyena_decode.h says so): of the history it writes column t and nothing else, and it shifts the tail.  With the tail
    put back (as the warm-up does) a refresh at t and the same step then give a live step: pos = t + 1, z finite, column t the same bits."""
    lib = _lib.lib()
    t = base + W
    assert t < Lcap
    g, kv, h = _operands(B, D, Lcap, seed, T, dev)
    k = _k_buffer(kv, Lcap - 1, dev)
    lda = _ceil(Lcap, 8)
    vg = torch.zeros(B, D, lda, dtype=T, device=dev)
    vg[:, :, :t] = h[:, :, :t]
    w, b_ = flat((3 * D, 3), g, torch.float32, dev), flat((3 * D,), g, torch.float32, dev)
    tail = flat((3 * D, B, 2), g, torch.float32, dev)
    x2 = flat((B, 3 * D), g, T, dev)
    x0 = torch.full((B, D), SENTINEL, device=dev)
    z = torch.full((B, D), SENTINEL, dtype=T, device=dev)
    part = torch.full((2, B, D), NAN, device=dev)
    carry = flat((B, W, D), g, torch.float32, dev)
    cpart = torch.full((lib.hyena_decode_carry_partial_floats(B, D, Lcap, W),), NAN, device=dev)
    pos = torch.tensor([t], dtype=torch.int32, device=dev)
    bas = torch.tensor([base], dtype=torch.int32, device=dev)
    parked = [z, part, carry, pos, bas]
    keep, vg0, tail0 = [x.clone() for x in parked], vg.clone(), tail.clone()

    def step():
        _lib.decode_pre(x2, None, w, b_, tail, vg, x0, pos, Lcap)
        _lib.decode_conv_la(k, vg, part, pos, bas, B, W, Lcap)
        _lib.decode_post_la(part, carry, vg, None, x0, z, pos, bas, B, Lcap)

    step()
    assert all(same_bits(a, b) for a, b in zip(parked, keep)), "conv_la / post_la wrote something at t = base + W"
    col = vg[:, :, t].clone()
    vg0[:, :, t] = col
    assert same_bits(vg, vg0), "decode_pre wrote a history column other than t"
    assert not same_bits(tail, tail0) and bool(torch.isfinite(col).all()), "decode_pre is expected to shift the tail and write column t"
    tail.copy_(tail0)
    with _lib._backend.guard(dev):
        _lib.check(lib.hyena_decode_carry(_P(k), k.stride(0), _P(vg), _P(cpart), _P(carry), _P(pos), _P(bas), B, D, Lcap, lda, W,
                                          _lib.dtype_code(T), _lib._backend.stream(dev)))
    step()
    assert bas.item() == t and pos.item() == t + 1 and bool(torch.isfinite(z).all()) and same_bits(vg[:, :, t], col)
    vg0[:, :, t] = vg[:, :, t]
    assert same_bits(vg, vg0)


def run_equals_plain(_lib, dev, T, B, D, Lcap, t, W, seed=0):
    """base = 0 and an all-zero carry: conv_la + post_la give decode_conv + decode_post's z, bit for bit"""
    g, kv, h = _operands(B, D, Lcap, seed, T, dev)
    x0 = flat((B, D), g, torch.float32, dev)
    fb = flat((D,), g, torch.float32, dev, 1.0, 2.0)
    k = _k_buffer(kv, Lcap - 1, dev)
    vg = torch.zeros(B, D, _ceil(Lcap, 8), dtype=T, device=dev)
    vg[:, :, :t + 1] = h[:, :, :t + 1]
    out = []
    for la in (False, True):
        pos = torch.tensor([t], dtype=torch.int32, device=dev)
        z = torch.full((B, D), SENTINEL, dtype=T, device=dev)
        if la:
            bas = torch.zeros(1, dtype=torch.int32, device=dev)
            carry = torch.zeros(B, W, D, device=dev)
            part = torch.full((2, B, D), NAN, device=dev)
            _lib.decode_conv_la(k, vg, part, pos, bas, B, W, Lcap)
            _lib.decode_post_la(part, carry, vg, fb, x0, z, pos, bas, B, Lcap)
        else:
            part = torch.full((_lib.lib().hyena_decode_partial_floats(B, D, Lcap),), NAN, device=dev)
            _lib.decode_conv(k, vg, part, pos, B, Lcap)
            _lib.decode_post(part, vg, fb, x0, z, pos, B, Lcap)
        assert pos.item() == t + 1
        out.append(z)
    assert bool(torch.isfinite(out[0]).all()) and same_bits(out[0], out[1]), (t, W, "the lookahead step at base 0 is not the plain step")


def check_bad_arguments(_lib, dev):
    """W = 0, W = 65, a null pointer: HYENA_ERR_BAD_ARG before anything is launched (every buffer is as it was)"""
    lib = _lib.lib()
    B, D, Lcap, W = 1, 4, 64, 8
    stream = _lib._backend.stream(dev)
    k = torch.ones(D, Lcap, device=dev)
    vg = torch.ones(B, D, Lcap, device=dev)
    part = torch.full((2 * B * W * D,), NAN, device=dev)
    carry = torch.full((B, W, D), NAN, device=dev)
    x0 = torch.ones(B, D, device=dev)
    z = torch.full((B, D), SENTINEL, device=dev)
    pos = torch.tensor([3], dtype=torch.int32, device=dev)
    bas = torch.tensor([2], dtype=torch.int32, device=dev)
    assert lib.hyena_decode_carry_partial_floats(2, 4, 8193, 8) == 2 * 2 * 8 * 4
    assert lib.hyena_decode_carry_partial_floats(2, 4, 8193, 0) == 0 and lib.hyena_decode_carry_partial_floats(2, 4, 8193, 65) == 0
    assert lib.hyena_decode_carry_partial_floats(1, 4, (1 << 20) + 1, 8) == 0
    with _lib._backend.guard(dev):
        for w in (0, 65, -1):
            assert lib.hyena_decode_carry(_P(k), Lcap, _P(vg), _P(part), _P(carry), _P(pos), _P(bas), B, D, Lcap, Lcap, w, 0, stream) == 1
            assert lib.hyena_decode_conv_la(_P(k), Lcap, _P(vg), _P(part), _P(pos), _P(bas), B, D, Lcap, Lcap, w, 0, stream) == 1
            assert lib.hyena_decode_post_la(_P(part), _P(carry), _P(vg), None, _P(x0), _P(z), _P(pos), _P(bas), B, D, Lcap, Lcap, w, 0, stream) == 1
        full = [_P(k), Lcap, _P(vg), _P(part), _P(carry), _P(pos), _P(bas), B, D, Lcap, Lcap, W, 0, stream]
        for i in (0, 2, 3, 4, 5, 6):
            assert lib.hyena_decode_carry(*(full[:i] + [None] + full[i + 1:])) == 1, i
        full = [_P(k), Lcap, _P(vg), _P(part), _P(pos), _P(bas), B, D, Lcap, Lcap, W, 0, stream]
        for i in (0, 2, 3, 4, 5):
            assert lib.hyena_decode_conv_la(*(full[:i] + [None] + full[i + 1:])) == 1, i
        full = [_P(part), _P(carry), _P(vg), None, _P(x0), _P(z), _P(pos), _P(bas), B, D, Lcap, Lcap, W, 0, stream]
        for i in (0, 1, 2, 4, 5, 6, 7):
            assert lib.hyena_decode_post_la(*(full[:i] + [None] + full[i + 1:])) == 1, i
        assert lib.hyena_decode_carry(_P(k), Lcap, _P(vg), _P(part), _P(carry), _P(pos), _P(bas), B, D, Lcap, Lcap, W, 7, stream) == 1   # dtype
    assert bool(torch.isnan(part).all()) and bool(torch.isnan(carry).all()) and bool((z == SENTINEL).all())
    assert pos.item() == 3 and bas.item() == 2


# ---- the kernel cases: (B, D, Lcap, t0, W), the smallest shapes that reach each path -----------------------------------------------------------
CARRY_CASES = [
    (1, 3, 8200, 0, 16),                    # t0 = 0: exact zeros, no history read
    (3, 5, 8200, 1, 17), (1, 3, 8200, 5, 64),                              # taps before position 0
    (3, 3, 16500, 8191, 16), (1, 5, 16500, 8192, 17), (3, 3, 16500, 8193, 64),                 # chunk edge and vector edge
    (1, 5, LCAP3, 2 * CHUNK + 13, 17), (3, 3, LCAP3, 2 * CHUNK + 13, 64),                      # third chunk
    (1, 3, 120, 8, 1), (1, 3, 120, 9, 1), (3, 5, 120, 10, 16), (1, 3, 120, 11, 17),            # t0 mod 4, W = 1
    (3, 3, 8260, 8260 - 16, 16), (1, 5, 8260, 8260 - 64, 64), (1, 3, 8260, 8259, 1),           # t0 + W = Lcap exactly
    (3, 5, 8260, 8250, 17), (1, 3, 8260, 8259, 64), (1, 3, 8200, 8191, 17),                    # t0 + W > Lcap: Lcap - t0 outputs
    (1, 3, 8200, 8200, 16), (1, 3, 8200, -1, 16),                                              # out of range: nothing is written, base stays
    (1, 256, 8200, 5, 17),                                                                     # the shipped width, one workgroup row per channel
]
CARRY_WIDE = [(3, 256, LCAP3, 2 * CHUNK + 13, 64), (1, 256, LCAP3, LCAP3 - 64, 64)]           # GPU only: 3 x 256 workgroups of real work

# (B, D, Lcap, base, W, ts): t = base, t = base + W - 1, a window across a chunk edge; parked: t = base + W, t = Lcap, t = base - 1
STEP_CASES = [
    (3, 3, 8200, 0, 16, (0, 1, 15, 16)),
    (1, 5, 8200, 5, 17, (5, 6, 13, 21, 22, 4)),
    (3, 5, 16500, 8185, 16, (8185, 8191, 8192, 8193, 8200, 8201)),         # the window straddles the chunk edge: two live partials
    (1, 3, 16500, 8192, 64, (8192, 8199, 8200, 8255, 8256)),
    (3, 3, LCAP3, 2 * CHUNK + 13, 17, (2 * CHUNK + 13, 2 * CHUNK + 16, 2 * CHUNK + 29, 2 * CHUNK + 30)),
    (1, 5, 8260, 8260 - 8, 16, (8252, 8259, 8260)),                        # the window runs past the cache: t = Lcap parks
    (1, 3, 120, 10, 1, (10, 11)),
    (1, 256, 8200, 8185, 16, (8185, 8192, 8200)),
]
STEP_WIDE = [(3, 256, LCAP3, 2 * CHUNK - 5, 64, (2 * CHUNK - 5, 2 * CHUNK, 2 * CHUNK + 58, 2 * CHUNK + 59))]
EQUAL_CASES = [(3, 3, 8200, 0, 16), (1, 5, 8200, 5, 17), (3, 5, 200, 63, 64), (1, 256, 100, 9, 64)]          # (B, D, Lcap, t, W)


def case_id(c):
    return "-".join(str(v) if isinstance(v, int) else f"t{v[0]}" for v in c)


# ---- HyenaDecodeState(lookahead=W): prefill P, then 2 W + 3 steps ---------------------------------------------------------------------------------
def _layer(l_max, **kw):
    d = dict(l_max=l_max, order=2, filter_order=64, emb_dim=5, short_filter_order=3, modulate=True, w=10, lr=6e-4, wd=0.0, lr_pos_emb=0.0)
    d.update(kw)
    return d


def run_state(dev, D, P, W=8, B=2, T=torch.float32, seed=0, label=""):
    """one operator's cache with lookahead: store_prefill of P positions (random activations), then 2 W + 3 steps.  Every step's z within the
    derived bound of the fp64 causal convolution of the stored operands (the cache's own k, history, fb, x0), `base` on the device equal to
    the position of the last due refresh after every step, pos = t + 1.  -> figures"""
    from hyena_dna_amd.hyena import HyenaOperator
    N = 2 * W + 3
    torch.manual_seed(seed + D + P)
    op = HyenaOperator(d_model=D, **_layer(P + N + 2)).to(dev)
    g = torch.Generator().manual_seed(seed + P)
    with torch.no_grad():
        st_ = op.allocate_inference_cache(B, P + N, dtype=T, lookahead=W)
        assert st_.W == W and st_.carry.shape == (B, W, D) and st_.base.dtype == torch.int32
        xT = (0.5 * torch.randn(3 * D, B, P, generator=g)).to(T).to(dev)
        vg = torch.randn(B, D, P, generator=g).to(T).to(dev)
        st_.store_prefill(xT, vg, P)
        assert st_.pos.item() == P and st_.base.item() == P and st_.la_used == 0
        k64, fb64 = st_.k.double(), st_.fb.double()
        st = _Stats()
        for i in range(N):
            t = P + i
            x2 = (0.5 * torch.randn(B, 3 * D, generator=g)).to(T).to(dev)
            z = st_.step(x2)
            base = P + (i // W) * W
            assert st_.pos.item() == t + 1 and st_.base.item() == base, (t, st_.pos.item(), st_.base.item(), base)
            h64 = st_.hist[:, :, :t + 1].double()
            y64, A = causal_ref(k64, h64, t, 1)
            f = fb64[None] * h64[:, :, t]
            y64, A = y64[:, 0] + f, A[:, 0] + f.abs()
            x64 = st_.x0.double()
            st.hold("z_state", z, y64 * x64, DL.post_bound(y64, A, n_step(base, t) - 1.0, x64, T))
    print(st.line(f"{label} state {NAME[T]} B={B} D={D} P={P} W={W}"), flush=True)
    return st


# ---- HyenaDNALM ---------------------------------------------------------------------------------------------------------------------------------
def rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()


def lm_teacher_forced(m, ids, P, W, autocast_dev=None):
    """the logits of positions P - 1 .. L - 2 from a lookahead cache (prefill P, then one step per known token) and from one full forward"""
    from hyena_dna_amd.inference import InferenceParams
    B, L = ids.shape
    ctx = torch.autocast(autocast_dev, dtype=torch.bfloat16) if autocast_dev else torch.autocast("cpu", enabled=False)
    with torch.no_grad(), ctx:
        ref = m(ids)[0].logits[:, P - 1:L - 1].float()
        ip = InferenceParams(max_seqlen=L, max_batch_size=B, lookahead=W)
        ip.key_value_memory_dict = m.allocate_inference_cache(B, L, lookahead=W)
        outs = [m(ids[:, :P], inference_params=ip)[0].logits[:, -1:].float()]
        for i in range(P, L - 1):
            ip.seqlen_offset = i
            outs.append(m(ids[:, i:i + 1], inference_params=ip)[0].logits.float())
        states = list(ip.key_value_memory_dict.values())
        assert all(s.W == W and s.base.item() == P + (L - 2 - P) // W * W for s in states) or L - 1 == P
    return torch.cat(outs, dim=1), ref


class watched:
    """``with watched(m) as log:`` -- what generate() does with the lookahead cache inside the block.  Wraps ``m.allocate_inference_cache``
    (log.caches: the {layer key: HyenaDecodeState} of every call, log.kwargs: its keywords) and ``HyenaDecodeState.refresh`` (log.refreshes:
    id(state) -> calls, whoever makes them: store_prefill, an eager step, or GraphedDecodeStep before a replay)."""

    def __enter__(self):
        from hyena_dna_amd.inference import HyenaDecodeState
        self._cls, self._refresh, self._alloc = HyenaDecodeState, HyenaDecodeState.refresh, self.m.allocate_inference_cache
        log = self

        def refresh(state):
            log.refreshes[id(state)] = log.refreshes.get(id(state), 0) + 1
            return log._refresh(state)

        def allocate(*args, **kw):
            caches = log._alloc(*args, **kw)
            log.caches.append(caches)
            log.kwargs.append(kw)
            return caches

        HyenaDecodeState.refresh = refresh
        self.m.allocate_inference_cache = allocate                            # (an instance attribute in front of the method)
        return self

    def __init__(self, m):
        self.m, self.caches, self.kwargs, self.refreshes = m, [], [], {}

    def __exit__(self, *exc):
        self._cls.refresh = self._refresh
        del self.m.allocate_inference_cache
        return False

    def check_schedule(self, W, P, n_new, n_layer=2):
        """ONE cache per layer, built with lookahead=W, and on each the host schedule of n_new tokens from a prompt of P: the refresh that ends
        the prefill, then one before every W-th of the n_new - 1 steps -- 1 + (n_new - 2) // W in all, neither more (a warm-up or a capture
        that counted) nor fewer; the window's use and ``base`` on the device where that leaves them; no cache left in external mode."""
        assert len(self.caches) == 1 and self.kwargs[0].get("lookahead") == W, ("generate did not ask for a lookahead cache", self.kwargs)
        states = list(self.caches[0].values())
        assert len(states) == n_layer
        later = (n_new - 2) // W
        for s in states:
            assert s.W == W and s.carry is not None and s.carry.shape[1] == W, "the cache generate() built has no lookahead window"
            assert self.refreshes.get(id(s), 0) == 1 + later, ("refreshes", self.refreshes.get(id(s), 0), 1 + later)
            assert s.la_used == n_new - 1 - later * W and not s.la_external, (s.la_used, s.la_external)
            assert s.pos.item() == P + n_new - 1 and s.base.item() == P + later * W, (s.pos.item(), s.base.item())


def check_greedy_against_forward(m, seq, P, tol, autocast_dev=None):
    """under the full forward over the produced sequence the logit of every new token lies within 2 tol ||row||_2 of its row's maximum"""
    ctx = torch.autocast(autocast_dev, dtype=torch.bfloat16) if autocast_dev else torch.autocast("cpu", enabled=False)
    with torch.no_grad(), ctx:
        logits = m(seq)[0].logits.float()[:, P - 1:-1]                                         # row i predicts token P + i
    chosen = logits.gather(2, seq[:, P:, None])[:, :, 0]
    gap = logits.max(-1).values - chosen
    assert bool((gap <= 2 * tol * logits.norm(dim=-1)).all()), ("a generated token is not the reference's argmax within the tolerance",
                                                               float((gap / logits.norm(dim=-1)).max()))
