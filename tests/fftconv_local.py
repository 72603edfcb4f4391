"""Element-wise fp64 references, bounds and case tables for the long convolution itself: every kernel branch of csrc/fftconv.hip (two-level
plan: col_fwd / col_inv of all 30 column sizes, the row kernels and the host loop over channel chunks) and of csrc/onchip.hip /
csrc/onchip_dk.hip (workspace-free plan, L <= 32768), reached BY DESIGN -- each case names the route it must take and asserts it from the
library's own host entry points (hyena_fftconv_plan, _fft_size, _default_chunk, _workspace_bytes) and the knobs in force.  Shared by the
emulator tests (tests/test_fftconv_local_emu.py) and the GPU tests (tests/test_gpu_fftconv_local.py).  Plain torch; not a test file.  Figures
of the oracle and of the kernels, run times and the seeded defects: profiles/fftconv_local.md.

Reference (float64, torch on the CPU, operands exactly as the kernel sees them -- 16-bit inputs rounded, then widened):
    out = irfft(rfft(u, 2L) rfft(k, 2L))[:L] + bias u        du = corr(dout, k) + bias dout        dk = sum_b corr(dout, u)
    dbias = sum dout u                                        (pinned to oracle.causal_conv_direct_f64 in the emulator file)
Inputs: u, dout, bias ~ randn; k = randn / sqrt(L), FLAT -- every tap weighs the same, so a mishandled late tap or ragged last tile shows.

Bounds, element-wise, per row, no element left out:
    fp32 out / du / dk     |got - ref64| <= C 2^-24 rms(ref64 row),  C = 4 x the largest figure the fp32 torch oracle (oracle.fftconv_ref and its
                           autograd) reaches on the same inputs, per quantity and size class: C_BOUND below, the measured figures beside it
    16-bit out / du        |got - ref64| <= half_ulp(ref64) + the fp32 bound;  got == round(ref64) except on < 2 % of the elements of a row
    dbias                  |got - sum dout u| < 3e-6 sqrt(B L) + 1e-6
dk and dbias are fp32, out and du have the input's type, everything is finite, and a second call gives the same bits."""
import math
import os

import torch

from tests.shell_local import DTYPES, NAME, half_ulp_io  # noqa: F401  (DTYPES, NAME: the test files' ids)

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
U = 2.0 ** -24
NAN = float("nan")
SENTINEL = 1536.0
SUPPORTED_M1 = (1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 14, 16, 20, 24, 28, 32, 64, 96, 128, 160, 192, 224, 256, 320, 384, 448, 512, 640, 768, 1024)
KNOBS = ("HYENA_FFTCONV_ONCHIP", "HYENA_FFTCONV_SMALL", "HYENA_FFTCONV_DK1", "HYENA_FFTCONV_DUDK")
MISMATCH_CAP = 0.02

# The fp32 torch oracle against the fp64 reference over ALL the case tables below, max |oracle - ref64| / (2^-24 rms(ref64 row)) per size class,
# measured on the CPU by `python -m tests.fftconv_local` (profiles/fftconv_local.md has the figures per table):
#                  out    du    dk
#   L <= 64       12.1   9.5   9.9
#   L <= 2048     41.0  49.2  45.5
#   L <= 32768    53.4  50.5  50.5
#   L <  2^20     46.2  43.0  54.6
#   L == 2^20    253.7 181.5 323.4     NOT used: the oracle's own weakness at the power of two 2L = 2^21 (15 - 21 at L = 65536, 19 - 21 at
#                                      163840).  The kernels' transform at L = 2^20 is the one of L = 2^20 - 3, so it is held to that class.
# C = 4 x the class's largest figure, rounded up to the next integer.
CLASSES = (64, 2048, 32768, (1 << 20) - 1, 1 << 20)
ORACLE_C = {64: (12.1, 9.5, 9.9), 2048: (41.0, 49.2, 45.5), 32768: (53.4, 50.5, 50.5), (1 << 20) - 1: (46.2, 43.0, 54.6)}
C_BOUND = {top: tuple(math.ceil(4 * c) for c in cs) for top, cs in ORACLE_C.items()}


def size_class(L):
    return min(top for top in CLASSES if L <= top)


def c_bound(L):
    """(C_out, C_du, C_dk) of the size class of L"""
    return C_BOUND[min(size_class(L), (1 << 20) - 1)]


def _bits(t):
    return t.view({4: torch.int32, 2: torch.int16}[t.element_size()])


def same_bits(a, b):
    if a is None or b is None:
        return a is None and b is None
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a.contiguous()), _bits(b.contiguous()))


# ---- inputs and the fp64 reference --------------------------------------------------------------------------------------------------------
def inputs(B, D, L, T, seed, bias=True):
    """host tensors: u, dout (B, D, L) of type T, k (D, L) fp32 flat, bias (D,) fp32 or None"""
    g = torch.Generator().manual_seed(seed)
    u = torch.randn(B, D, L, generator=g).to(T)
    k = torch.randn(D, L, generator=g) / math.sqrt(L)
    b = torch.randn(D, generator=g)
    dout = torch.randn(B, D, L, generator=g).to(T)
    return u, k, (b if bias else None), dout


def ref64(u, k, bias, dout):
    """-> out, du (B, D, L), dk (D, L), dbias (D,), all float64, from host tensors of any float type"""
    u, k, dout = u.double(), k.double(), dout.double()
    L = u.shape[-1]
    n = 2 * L
    b = torch.zeros(k.shape[0], dtype=torch.float64) if bias is None else bias.double()
    Uf, Kf, Gf = torch.fft.rfft(u, n=n), torch.fft.rfft(k, n=n), torch.fft.rfft(dout, n=n)
    out = torch.fft.irfft(Uf * Kf, n=n)[..., :L] + u * b[:, None]
    du = torch.fft.irfft(Gf * Kf.conj(), n=n)[..., :L] + dout * b[:, None]
    dk = torch.fft.irfft((Gf * Uf.conj()).sum(0), n=n)[..., :L]
    return out, du, dk, (dout * u).sum(dim=(0, 2))


def oracle32(u, k, bias, dout):
    """the fp32 torch oracle and its autograd on the same operands (16-bit ones widened) -> out, du, dk"""
    from oracle import hyena_oracle as O
    u_ = u.float().clone().requires_grad_(True)
    k_ = k.clone().requires_grad_(True)
    b_ = torch.zeros(k.shape[0]) if bias is None else bias
    out = O.fftconv_ref(u_, k_, b_)
    out.backward(dout.float())
    return out.detach(), u_.grad, k_.grad


def _rms(ref):
    return ref.pow(2).mean(dim=-1, keepdim=True).sqrt()


def figure32(got, ref):
    """max over the elements of |got - ref| / (2^-24 rms of the row); a row whose reference is all zero counts only if got is not"""
    d = (got.double() - ref).abs()
    r = _rms(ref).expand_as(d)
    nz = r > 0
    fig = float((d[nz] / (U * r[nz])).max()) if bool(nz.any()) else 0.0
    return math.inf if bool((d[~nz] > 0).any()) else fig


def mismatch_share(got, ref, T):
    """largest share, over the rows, of elements that are not the reference rounded to T"""
    return float((got != ref.to(T)).double().mean(dim=-1).max())


class Stats(dict):
    def put(self, name, v):
        self[name] = max(self.get(name, 0.0), v)

    def hold32(self, name, got, ref, C, own=0.0):
        """own: the bound is own 2^-24 |ref row|_2 at every element instead (the impulse probes alone, see run_probes)"""
        assert got.dtype == F32 and got.shape == ref.shape, (name, got.dtype, got.shape)
        assert bool(torch.isfinite(got).all()), (name, "not finite")
        if own:
            d, bound = (got.double() - ref).abs(), (own * U * ref.norm(dim=-1, keepdim=True)).expand_as(ref)
            self.put(name + "/bound", float((d / bound).max()))
            assert bool((d <= bound).all()), (name, float((d / bound).max()), int((d > bound).sum()))
            return
        fig = figure32(got, ref)
        self.put(name, fig)
        assert fig <= C, (name, fig, C, int(((got.double() - ref).abs() > C * U * _rms(ref)).sum()))

    def hold16(self, name, got, ref, C, T, flips=True, own=0.0):
        assert got.dtype == T and got.shape == ref.shape, (name, got.dtype, got.shape)
        assert bool(torch.isfinite(got).all()), (name, "not finite")
        d = (got.double() - ref).abs()
        bound = half_ulp_io(ref.abs(), T) + (own * U * ref.norm(dim=-1, keepdim=True) if own else C * U * _rms(ref))
        self.put(name + "/bound", float((d / bound.clamp_min(1e-300)).max()))
        assert bool((d <= bound).all()), (name, float((d / bound.clamp_min(1e-300)).max()), int((d > bound).sum()))
        if not flips:
            return
        share = mismatch_share(got, ref, T)
        self.put(name + "_flips", share)
        assert share < MISMATCH_CAP, (name, "share of elements that are not the rounded reference", share)

    def hold(self, name, got, ref, C, T, flips=True, own=0.0):
        if T == F32:
            self.hold32(name, got, ref, C, own)
        else:
            self.hold16(name, got, ref, C, T, flips, own)

    def line(self, label):
        return f"[fftconv-local] {label} " + " ".join(f"{k}={v:.3g}" for k, v in self.items())


# ---- which kernels a call reaches: the dispatch of csrc/fftconv.hip, onchip.hip and onchip_dk.hip, from the library's host entry points ---
def _off(name):
    return os.environ.get(name, "")[:1] == "0"


def route(_lib, B, D, L, need_du=True, need_dk=True, saved=False, chunk=0):
    """The kernels forward + backward of this call run, as one string.  Plan, transform size, chunking, the number of dk slices and the dk
    form at B = 1 are READ from the library (so a dispatch change shows); the rest mirrors the conditions of the host code on the knobs."""
    lib = _lib.lib()
    plan, M = lib.hyena_fftconv_plan(L), lib.hyena_fftconv_fft_size(L)
    assert plan in (_lib.PLAN_ONCHIP, _lib.PLAN_TWO_LEVEL) and M % 1024 == 0 and M >= L
    if plan == _lib.PLAN_TWO_LEVEL:
        M1 = M // 1024
        assert M1 in SUPPORTED_M1 and (M1 == 1 or SUPPORTED_M1[SUPPORTED_M1.index(M1) - 1] * 1024 < L)
        pairs = (M1 - 1) // 2
        parts = [f"two col<{M1}>", "side" if pairs else "noside"]
        if need_dk:
            du = "du" if need_du else "nodu"
            parts.append(f"row0_bwd<{du}>" + ("" if not pairs else f"+row_bwd<{du}>" if B == 1 else "+row_dk+corr" if need_du else "+row_dk"))
        else:
            parts.append("row0_corr" + ("+corr" if pairs else ""))
        for bwd in (0, 1):
            c = min(chunk or lib.hyena_fftconv_default_chunk(B, D, L, bwd), D)
            assert lib.hyena_fftconv_workspace_bytes(B, D, L, bwd, chunk) == ((2 * B + 2 if bwd else B + 1) * c * M + bwd * B * c * 2048) * 8
            parts.append(f"chunks={D // c}x{c}" + (f"+{D % c}" if D % c else ""))
        return " ".join(parts + (["saved"] if saved else []))
    R = M // 1024
    assert R in (1, 2, 4, 8, 16, 32) and (R == 1 or 512 * R < L)
    spec = D * M * 8
    assert lib.hyena_fftconv_workspace_bytes(B, D, L, 0, 0) == spec
    extra = lib.hyena_fftconv_workspace_bytes(B, D, L, 1, 0) - spec
    dk1 = B == 1 and R == 32 and not _off("HYENA_FFTCONV_DK1")
    if dk1:
        extra -= spec                                        # the spectrum of u behind the partial rows
    assert extra >= 0 and extra % (D * L * 4) == 0, "HYENA_FFTCONV_DK1 is not what the library reads, or the partial rows changed"
    S = extra // (D * L * 4) or 1
    groups = 1 if R == 32 else min(16, 512 // (32 * R))      # dk_row_groups: batch rows one step of dk_kernel takes
    if S > 1:
        nb = -(-(-(-B // S)) // groups) * groups
        assert -(-B // nb) == S
    if R <= 2 and not _off("HYENA_FFTCONV_SMALL") and B <= 2 * (256 // (32 * R)):
        return f"oc small_fwd<{R}> small_bwd<{R}>" + (" saved" if saved else "")
    parts = [f"oc spec<{R}>+conv<{R}>"]
    e = os.environ.get("HYENA_FFTCONV_DUDK", "")[:1]
    if need_du and need_dk and B >= 2 and R <= 16 and e != "0" and (e == "1" or R == 16):
        parts.append(f"dk<{R},1,DU> S={S}" + ("" if S == 1 else f" ragged={B % nb}"))
    else:
        if need_du:
            parts.append(f"corr<{R}>")
        if need_dk:
            parts.append("conv<32,f32out>" if dk1 else ("dk<16,2>" if R == 32 else f"dk<{R},1>") + f" S={S}" + ("" if S == 1 else f" ragged={B % nb}"))
    return " ".join(parts + (["saved"] if saved else []))


class knobs:
    """the environment knobs of one case (read by the library on every call), through pytest's monkeypatch"""

    def __init__(self, mp, env):
        self.mp, self.env = mp, env or {}

    def __enter__(self):
        for name in KNOBS:
            self.mp.delenv(name, raising=False)
        for name, v in self.env.items():
            assert "HYENA_FFTCONV_" + name in KNOBS
            self.mp.setenv("HYENA_FFTCONV_" + name, str(v))

    def __exit__(self, *exc):
        for name in KNOBS:
            self.mp.delenv(name, raising=False)


# ---- one case ----------------------------------------------------------------------------------------------------------------------------
def _call(_lib, dev, u, k, bias, dout, need, saved, chunk, place=None):
    """forward (+ the spectra when saved) and backward on the device -> out, du, dk, dbias on the host.  place(tensor, "x" | "k"): how u / dout and k
    reach the device (default: packed); a pitched view makes the wrappers hand its pitch on, and out / du / dk come back at that pitch"""
    put = place or (lambda t, kind: t.to(dev))
    ud, kd, gd = put(u, "x"), put(k, "k"), put(dout, "x")
    bd = None if bias is None else bias.to(dev)
    if saved:
        out, sp = _lib.fftconv_fwd(ud, kd, bd, chunk=chunk, save=True)
    else:
        out, sp = _lib.fftconv_fwd(ud, kd, bd, chunk=chunk), None
    du, dk, db = _lib.fftconv_bwd(gd, ud, kd, bd, need_du=bool(need[0]), need_dk=bool(need[1]), chunk=chunk, saved=sp)
    return tuple(None if t is None else t.cpu() for t in (out, du, dk, db))


def run_case(_lib, dev, mp, T, B, D, L, want, need=(1, 1), saved=False, chunk=0, bias=True, env=None, seed=None, label="", place=None):
    """forward + backward of one shape under one setting of the knobs: the route is `want`, every output within its bound of the fp64
    reference at every element, types as promised, a second call the same bits.  -> (figures, outputs)
    place: see _call (tests/limits_local.py: the inputs on rows gigabytes apart)."""
    seed = 7 * L + 3 * B + D if seed is None else seed
    u, k, b, dout = inputs(B, D, L, T, seed, bias)
    with knobs(mp, env):
        got_route = route(_lib, B, D, L, bool(need[0]), bool(need[1]), saved, chunk)
        assert got_route == want, ("the case no longer reaches the code it was written for", got_route, want)
        got = _call(_lib, dev, u, k, b, dout, need, saved, chunk, place)
        again = _call(_lib, dev, u, k, b, dout, need, saved, chunk, place)
    assert all(same_bits(a, c) for a, c in zip(got, again)), "a second call gives other bits"
    out, du, dk, db = got
    r_out, r_du, r_dk, r_db = ref64(u, k, b, dout)
    Co, Cu, Ck = c_bound(L)
    st = Stats()
    st.hold("out", out, r_out, Co, T)
    assert (du is None) == (not need[0]) and (dk is None) == (not need[1]) and (db is None) == (not need[1])
    if need[0]:
        st.hold("du", du, r_du, Cu, T)
    if need[1]:
        st.hold32("dk", dk, r_dk, Ck)
        assert db.dtype == F32 and db.shape == (D,) and bool(torch.isfinite(db).all())
        e = float((db.double() - r_db).abs().max())
        st.put("dbias/bound", e / (3e-6 * math.sqrt(B * L) + 1e-6))
        assert e < 3e-6 * math.sqrt(B * L) + 1e-6, ("dbias", e)
    print(st.line(f"{label} {NAME[T]} B={B} D={D} L={L} need={need} saved={int(saved)} chunk={chunk} bias={int(bias)} env={env or {}} | {want} |"),
          flush=True)
    return st, got


def run_probes(_lib, dev, mp, T, L, env, want, D=2, label=""):
    """exact structural probes, B = 1, no bias: u = e_0, k = e_(L-1) -> out = e_(L-1), and the mirrored pair; dout = e_(L-1) -> dk[j] = u[L-1-j]
    (dk[0] = u[L-1]) and du[s] = k[L-1-s].  The expected values are exact; the bounds of dk and du are those of every other case.  The impulse
    pairs' output row is zero but for one element, and its spectrum is a pure tone: the rounding errors of the twiddles are then coherent, not
    noise, and gather in a few elements (the one itself: 4 units in its last place; zeros at offsets that are multiples of M / 8 from it: up to
    1 such unit, 250 2^-24 rms of the row at L = 65533) -- the statistics behind C rms do not hold.  What holds for any input is the norm-wise
    bound of the transform (Higham, Accuracy and Stability of Numerical Algorithms, Theorem 24.2: log2(N) roundings' worth of the vector's
    2-norm per transform): every element within 3 log2(2M) 2^-24 |row|_2 for the three transforms of 2M real points (33 ... 63 units of the
    one element's last place; a misplaced, doubled or mis-scaled element is off by its whole size, 2^24 such units).  No transform returns
    the zeros bit for bit, so the share of 16-bit elements off the rounded reference is taken where the reference is dense."""
    Co, Cu, Ck = c_bound(L)
    own = 3 * math.log2(2 * _lib.lib().hyena_fftconv_fft_size(L))
    e0, e1 = torch.zeros(L, dtype=torch.float64), torch.zeros(L, dtype=torch.float64)
    e0[0], e1[L - 1] = 1.0, 1.0
    u, k, _, dout = inputs(1, D, L, T, 11 * L + 1, bias=False)
    st = Stats()
    with knobs(mp, env):
        assert route(_lib, 1, D, L) == want, (route(_lib, 1, D, L), want)
        for name, a, b in (("impulse", e0, e1), ("mirrored", e1, e0)):
            ua = a.to(T)[None, None].expand(1, D, L).contiguous()
            out = _lib.fftconv_fwd(ua.to(dev), b.float()[None].expand(D, L).contiguous().to(dev), None).cpu()
            st.hold(name, out, e1[None, None].expand(1, D, L), Co, T, flips=False, own=own)
        g = e1.to(T)[None, None].expand(1, D, L).contiguous()
        du, dk, db = _lib.fftconv_bwd(g.to(dev), u.to(dev), k.to(dev), None)
        du, dk, db = du.cpu(), dk.cpu(), db.cpu()
    r_dk, r_du = u[0].double().flip(-1), k.double().flip(-1)[None]
    st.hold32("probe_dk", dk, r_dk, Ck)
    st.hold("probe_du", du, r_du, Cu, T)
    bound0 = Ck * U * _rms(r_dk)[:, 0]
    assert bool(((dk[:, 0].double() - u[0, :, L - 1].double()).abs() <= bound0).all()), "dk[0] is not u[L - 1]"
    assert bool(((db.double() - u[0, :, L - 1].double()).abs() < 3e-6 * math.sqrt(L) + 1e-6).all())
    print(st.line(f"{label} probes {NAME[T]} L={L} env={env or {}} | {want} |"), flush=True)
    return st


# ---- A: the two-level column kernels, every M1 x every type ---------------------------------------------------------------------------------
A_EXTRA_M1 = (1, 2, 3, 64, 160, 1024)                 # also at L = 1024 M1 exactly and at the shortest L that selects M1; fp32 and bf16
A_ENV = {"ONCHIP": 0}                                 # for M1 <= 32 (L <= 32768 runs on the workspace-free plan otherwise)


def a_route(M1):
    return f"two col<{M1}> " + ("side" if M1 >= 3 else "noside") + " row0_bwd<du>" + ("+row_bwd<du>" if M1 >= 3 else "") + " chunks=1x2 chunks=1x2"


def a_lengths(M1):
    """L = 1024 M1 - 3; for the M1 of A_EXTRA_M1 also 1024 M1 and the shortest L that selects M1"""
    Ls = [1024 * M1 - 3]
    if M1 in A_EXTRA_M1:
        Ls += [1024 * M1, 1 if M1 == 1 else 1024 * SUPPORTED_M1[SUPPORTED_M1.index(M1) - 1] + 1]
    return Ls


A_KINDS = ("ragged", "full", "shortest", "probes")
A_PARAMS = [(M1, kind) for M1 in SUPPORTED_M1 for kind in (A_KINDS if M1 in A_EXTRA_M1 else A_KINDS[:1])]


def suite_columns(_lib, dev, mp, T, M1, kind, label):
    """B = 1, D = 2, forward + full backward at one of a_lengths(M1) (the two extra lengths in fp32 and bf16), or the probes at the ragged length"""
    env = A_ENV if M1 <= 32 else None
    assert T != F16 or kind == "ragged"
    if kind == "probes":
        return run_probes(_lib, dev, mp, T, 1024 * M1 - 3, env, a_route(M1), label=label)
    return run_case(_lib, dev, mp, T, 1, 2, a_lengths(M1)[A_KINDS.index(kind)], a_route(M1), env=env, label=label)[0]


# ---- B: the two-level row kernels and the host loop: a pairwise-covering selection --------------------------------------------------------
# (M1, B, chunk, (need_du, need_dk), saved, bias, type, route); D = 3, L = 1024 M1 - 3, HYENA_FFTCONV_ONCHIP=0 for M1 <= 7.  chunk 0 = the
# default (all three channels at once); chunk 2 leaves a tail chunk of one channel.  Every pair of values of two factors occurs.
B_CASES = [
    (1, 1, 0, (1, 0), 1, 0, BF16, "two col<1> noside row0_corr chunks=1x3 chunks=1x3 saved"),
    (1, 1, 2, (0, 1), 1, 0, F32, "two col<1> noside row0_bwd<nodu> chunks=1x2+1 chunks=1x2+1 saved"),
    (1, 1, 2, (1, 1), 0, 1, F32, "two col<1> noside row0_bwd<du> chunks=1x2+1 chunks=1x2+1"),
    (1, 2, 0, (0, 1), 0, 1, BF16, "two col<1> noside row0_bwd<nodu> chunks=1x3 chunks=1x3"),
    (1, 2, 0, (1, 1), 1, 1, BF16, "two col<1> noside row0_bwd<du> chunks=1x3 chunks=1x3 saved"),
    (1, 3, 2, (1, 0), 0, 1, F32, "two col<1> noside row0_corr chunks=1x2+1 chunks=1x2+1"),
    (2, 1, 0, (1, 0), 1, 0, BF16, "two col<2> noside row0_corr chunks=1x3 chunks=1x3 saved"),
    (2, 1, 2, (0, 1), 1, 0, F32, "two col<2> noside row0_bwd<nodu> chunks=1x2+1 chunks=1x2+1 saved"),
    (2, 1, 2, (1, 1), 0, 1, F32, "two col<2> noside row0_bwd<du> chunks=1x2+1 chunks=1x2+1"),
    (2, 2, 0, (0, 1), 0, 1, F32, "two col<2> noside row0_bwd<nodu> chunks=1x3 chunks=1x3"),
    (2, 2, 0, (1, 0), 0, 1, F32, "two col<2> noside row0_corr chunks=1x3 chunks=1x3"),
    (2, 3, 0, (0, 1), 1, 1, BF16, "two col<2> noside row0_bwd<nodu> chunks=1x3 chunks=1x3 saved"),
    (2, 3, 2, (1, 1), 1, 0, BF16, "two col<2> noside row0_bwd<du> chunks=1x2+1 chunks=1x2+1 saved"),
    (3, 1, 0, (1, 0), 0, 1, F32, "two col<3> side row0_corr+corr chunks=1x3 chunks=1x3"),
    (3, 1, 0, (1, 1), 0, 1, F32, "two col<3> side row0_bwd<du>+row_bwd<du> chunks=1x3 chunks=1x3"),
    (3, 1, 2, (0, 1), 0, 0, BF16, "two col<3> side row0_bwd<nodu>+row_bwd<nodu> chunks=1x2+1 chunks=1x2+1"),
    (3, 2, 0, (1, 1), 1, 0, BF16, "two col<3> side row0_bwd<du>+row_dk+corr chunks=1x3 chunks=1x3 saved"),
    (3, 2, 2, (0, 1), 1, 0, BF16, "two col<3> side row0_bwd<nodu>+row_dk chunks=1x2+1 chunks=1x2+1 saved"),
    (3, 3, 2, (1, 0), 0, 1, F32, "two col<3> side row0_corr+corr chunks=1x2+1 chunks=1x2+1"),
    (7, 1, 0, (1, 1), 1, 1, F32, "two col<7> side row0_bwd<du>+row_bwd<du> chunks=1x3 chunks=1x3 saved"),
    (7, 1, 2, (0, 1), 1, 0, F32, "two col<7> side row0_bwd<nodu>+row_bwd<nodu> chunks=1x2+1 chunks=1x2+1 saved"),
    (7, 1, 2, (1, 0), 0, 1, F32, "two col<7> side row0_corr+corr chunks=1x2+1 chunks=1x2+1"),
    (7, 2, 0, (1, 0), 1, 1, F32, "two col<7> side row0_corr+corr chunks=1x3 chunks=1x3 saved"),
    (7, 2, 2, (0, 1), 0, 0, BF16, "two col<7> side row0_bwd<nodu>+row_dk chunks=1x2+1 chunks=1x2+1"),
    (7, 3, 0, (1, 1), 0, 0, BF16, "two col<7> side row0_bwd<du>+row_dk+corr chunks=1x3 chunks=1x3"),
    (7, 3, 2, (1, 1), 1, 1, F32, "two col<7> side row0_bwd<du>+row_dk+corr chunks=1x2+1 chunks=1x2+1 saved"),
    (64, 1, 0, (1, 0), 0, 0, BF16, "two col<64> side row0_corr+corr chunks=1x3 chunks=1x3"),
    (64, 1, 0, (1, 1), 0, 1, F32, "two col<64> side row0_bwd<du>+row_bwd<du> chunks=1x3 chunks=1x3"),
    (64, 1, 2, (0, 1), 0, 1, F32, "two col<64> side row0_bwd<nodu>+row_bwd<nodu> chunks=1x2+1 chunks=1x2+1"),
    (64, 2, 0, (1, 1), 0, 1, BF16, "two col<64> side row0_bwd<du>+row_dk+corr chunks=1x3 chunks=1x3"),
    (64, 2, 2, (0, 1), 1, 1, F32, "two col<64> side row0_bwd<nodu>+row_dk chunks=1x2+1 chunks=1x2+1 saved"),
    (64, 2, 2, (1, 0), 1, 1, F32, "two col<64> side row0_corr+corr chunks=1x2+1 chunks=1x2+1 saved"),
    (64, 3, 0, (1, 1), 1, 0, BF16, "two col<64> side row0_bwd<du>+row_dk+corr chunks=1x3 chunks=1x3 saved"),
    (96, 1, 0, (1, 1), 1, 1, F32, "two col<96> side row0_bwd<du>+row_bwd<du> chunks=1x3 chunks=1x3 saved"),
    (96, 1, 2, (0, 1), 1, 1, BF16, "two col<96> side row0_bwd<nodu>+row_bwd<nodu> chunks=1x2+1 chunks=1x2+1 saved"),
    (96, 1, 2, (1, 0), 1, 1, BF16, "two col<96> side row0_corr+corr chunks=1x2+1 chunks=1x2+1 saved"),
    (96, 2, 0, (1, 0), 0, 1, BF16, "two col<96> side row0_corr+corr chunks=1x3 chunks=1x3"),
    (96, 2, 2, (1, 1), 1, 0, F32, "two col<96> side row0_bwd<du>+row_dk+corr chunks=1x2+1 chunks=1x2+1 saved"),
    (96, 3, 0, (1, 1), 0, 1, F32, "two col<96> side row0_bwd<du>+row_dk+corr chunks=1x3 chunks=1x3"),
    (96, 3, 2, (0, 1), 0, 0, BF16, "two col<96> side row0_bwd<nodu>+row_dk chunks=1x2+1 chunks=1x2+1"),
]


def suite_rows(_lib, dev, mp, i, label):
    M1, B, chunk, need, saved, bias, T, want = B_CASES[i]
    return run_case(_lib, dev, mp, T, B, 3, 1024 * M1 - 3, want, need=need, saved=bool(saved), chunk=chunk, bias=bool(bias),
                    env=A_ENV if M1 <= 32 else None, seed=1000 + i, label=label)[0]


# ---- C: the workspace-free plan -----------------------------------------------------------------------------------------------------------
# (R, B, D, L, (need_du, need_dk), saved, knobs, types, route)
ALL, F32_BF16, F32_F16 = (F32, BF16, F16), (F32, BF16), (F32, F16)
C_CASES = [
    # the default knobs.  R <= 2 with a small batch: the one-launch pair; one batch row past its limit 2 (256 / 32 R): the general kernels, two
    # dk slices, the last one ragged
    (1, 1, 3, 1021, (1, 1), 0, None, ALL, "oc small_fwd<1> small_bwd<1>"),
    (1, 2, 3, 1021, (1, 1), 1, None, ALL, "oc small_fwd<1> small_bwd<1> saved"),
    (1, 2, 3, 1, (1, 1), 0, None, ALL, "oc small_fwd<1> small_bwd<1>"),
    (1, 2, 3, 37, (1, 1), 0, None, ALL, "oc small_fwd<1> small_bwd<1>"),
    (1, 17, 3, 1021, (1, 1), 0, None, ALL, "oc spec<1>+conv<1> corr<1> dk<1,1> S=2 ragged=1"),
    (2, 1, 3, 2045, (1, 1), 0, None, ALL, "oc small_fwd<2> small_bwd<2>"),
    (2, 2, 3, 2045, (1, 1), 1, None, ALL, "oc small_fwd<2> small_bwd<2> saved"),
    (2, 9, 3, 2045, (1, 1), 0, None, ALL, "oc spec<2>+conv<2> corr<2> dk<2,1> S=2 ragged=1"),
    (4, 1, 3, 4093, (1, 1), 0, None, ALL, "oc spec<4>+conv<4> corr<4> dk<4,1> S=1"),
    (4, 2, 3, 4093, (1, 1), 1, None, ALL, "oc spec<4>+conv<4> corr<4> dk<4,1> S=1 saved"),
    (4, 9, 3, 4093, (1, 1), 0, None, ALL, "oc spec<4>+conv<4> corr<4> dk<4,1> S=3 ragged=1"),
    (4, 2, 264, 4093, (1, 1), 0, None, ALL, "oc spec<4>+conv<4> corr<4> dk<4,1> S=1"),          # D % 8 == 0: the XCD-aware row mapping, no slices
    (4, 2, 7, 4093, (1, 1), 0, None, ALL, "oc spec<4>+conv<4> corr<4> dk<4,1> S=1"),            # the plain row mapping
    (8, 1, 3, 8189, (1, 1), 0, None, ALL, "oc spec<8>+conv<8> corr<8> dk<8,1> S=1"),
    (8, 2, 3, 8189, (1, 1), 1, None, ALL, "oc spec<8>+conv<8> corr<8> dk<8,1> S=1 saved"),
    (16, 1, 3, 16381, (1, 1), 0, None, ALL, "oc spec<16>+conv<16> corr<16> dk<16,1> S=1"),       # dk_kernel<16, 1> at B = 1
    (16, 2, 3, 16381, (1, 1), 0, None, ALL, "oc spec<16>+conv<16> dk<16,1,DU> S=2 ragged=0"),
    (32, 1, 3, 32765, (1, 1), 0, None, ALL, "oc spec<32>+conv<32> corr<32> conv<32,f32out>"),    # dk at B = 1: conv_kernel<32, ., true>
    (32, 2, 3, 32765, (1, 1), 1, None, ALL, "oc spec<32>+conv<32> corr<32> dk<16,2> S=2 ragged=0 saved"),
    # HYENA_FFTCONV_SMALL=0 at R <= 2: the general kernels; at R = 1 they take two rows per workgroup: 3, 21 and 14 rows
    (1, 1, 3, 1021, (1, 1), 0, {"SMALL": 0}, F32_BF16, "oc spec<1>+conv<1> corr<1> dk<1,1> S=1"),
    (1, 2, 3, 1021, (1, 1), 1, {"SMALL": 0}, F32_F16, "oc spec<1>+conv<1> corr<1> dk<1,1> S=1 saved"),
    (1, 3, 7, 1021, (1, 1), 0, {"SMALL": 0}, F32_BF16, "oc spec<1>+conv<1> corr<1> dk<1,1> S=1"),
    (1, 2, 7, 1021, (1, 1), 0, {"SMALL": 0}, F32_F16, "oc spec<1>+conv<1> corr<1> dk<1,1> S=1"),
    (2, 1, 3, 2045, (1, 1), 0, {"SMALL": 0}, F32_F16, "oc spec<2>+conv<2> corr<2> dk<2,1> S=1"),
    (2, 2, 3, 2045, (1, 1), 1, {"SMALL": 0}, F32_BF16, "oc spec<2>+conv<2> corr<2> dk<2,1> S=1 saved"),
    (2, 2, 264, 2045, (1, 1), 0, {"SMALL": 0}, F32_BF16, "oc spec<2>+conv<2> corr<2> dk<2,1> S=1"),
    # HYENA_FFTCONV_DK1=0 at R = 32, B = 1: dk_kernel<16, 2> with nothing to accumulate over
    (32, 1, 3, 32765, (1, 1), 0, {"DK1": 0}, F32_BF16, "oc spec<32>+conv<32> corr<32> dk<16,2> S=1"),
    # HYENA_FFTCONV_DUDK=1 below M = 16384: du from dk's transform of dout, dk_kernel<R, 1, ., 0, true> for R <= 8
    (1, 2, 3, 1021, (1, 1), 0, {"SMALL": 0, "DUDK": 1}, F32_BF16, "oc spec<1>+conv<1> dk<1,1,DU> S=1"),
    (2, 2, 3, 2045, (1, 1), 1, {"SMALL": 0, "DUDK": 1}, F32_F16, "oc spec<2>+conv<2> dk<2,1,DU> S=1 saved"),
    (4, 2, 3, 4093, (1, 1), 0, {"DUDK": 1}, F32_BF16, "oc spec<4>+conv<4> dk<4,1,DU> S=1"),
    (4, 9, 3, 4093, (1, 1), 1, {"DUDK": 1}, F32_F16, "oc spec<4>+conv<4> dk<4,1,DU> S=3 ragged=1 saved"),
    (8, 2, 3, 8189, (1, 1), 0, {"DUDK": 1}, F32_BF16, "oc spec<8>+conv<8> dk<8,1,DU> S=1"),
    # HYENA_FFTCONV_DUDK=0 at R = 16, B >= 2: dk_kernel<16, 1, ., 0, false> beside a separate du
    (16, 2, 3, 16381, (1, 1), 0, {"DUDK": 0}, F32_F16, "oc spec<16>+conv<16> corr<16> dk<16,1> S=2 ragged=0"),
    # du only and dk only at R > 2, with the forward's spectrum and without
    (4, 2, 3, 4093, (1, 0), 0, None, F32_BF16, "oc spec<4>+conv<4> corr<4>"),
    (4, 2, 3, 4093, (1, 0), 1, None, F32_BF16, "oc spec<4>+conv<4> corr<4> saved"),
    (4, 2, 3, 4093, (0, 1), 0, None, F32_BF16, "oc spec<4>+conv<4> dk<4,1> S=1"),
    (4, 2, 3, 4093, (0, 1), 1, None, F32_BF16, "oc spec<4>+conv<4> dk<4,1> S=1 saved"),
    (16, 2, 3, 16381, (1, 0), 0, None, F32_BF16, "oc spec<16>+conv<16> corr<16>"),
    (16, 2, 3, 16381, (1, 0), 1, None, F32_BF16, "oc spec<16>+conv<16> corr<16> saved"),
    (16, 2, 3, 16381, (0, 1), 0, None, F32_BF16, "oc spec<16>+conv<16> dk<16,1> S=2 ragged=0"),
    (16, 2, 3, 16381, (0, 1), 1, None, F32_BF16, "oc spec<16>+conv<16> dk<16,1> S=2 ragged=0 saved"),
    (32, 2, 3, 32765, (1, 0), 0, None, F32_BF16, "oc spec<32>+conv<32> corr<32>"),
    (32, 2, 3, 32765, (1, 0), 1, None, F32_BF16, "oc spec<32>+conv<32> corr<32> saved"),
    (32, 2, 3, 32765, (0, 1), 0, None, F32_BF16, "oc spec<32>+conv<32> dk<16,2> S=2 ragged=0"),
    (32, 2, 3, 32765, (0, 1), 1, None, F32_BF16, "oc spec<32>+conv<32> dk<16,2> S=2 ragged=0 saved"),
    (32, 1, 3, 32765, (0, 1), 0, None, F32_F16, "oc spec<32>+conv<32> conv<32,f32out>"),
]


def suite_onchip(_lib, dev, mp, i, T, label):
    R, B, D, L, need, saved, env, types, want = C_CASES[i]
    assert T in types and _lib.lib().hyena_fftconv_fft_size(L) == 1024 * R
    return run_case(_lib, dev, mp, T, B, D, L, want, need=need, saved=bool(saved), env=env, seed=2000 + i, label=label)[0]


C_PROBES = [(1, 1021, None, "oc small_fwd<1> small_bwd<1>"), (1, 1021, {"SMALL": 0}, "oc spec<1>+conv<1> corr<1> dk<1,1> S=1"),
            (2, 2045, {"SMALL": 0}, "oc spec<2>+conv<2> corr<2> dk<2,1> S=1"), (4, 4093, None, "oc spec<4>+conv<4> corr<4> dk<4,1> S=1"),
            (8, 8189, None, "oc spec<8>+conv<8> corr<8> dk<8,1> S=1"), (16, 16381, None, "oc spec<16>+conv<16> corr<16> dk<16,1> S=1"),
            (32, 32765, None, "oc spec<32>+conv<32> corr<32> conv<32,f32out>"), (32, 32765, {"DK1": 0}, "oc spec<32>+conv<32> corr<32> dk<16,2> S=1")]


def suite_onchip_probes(_lib, dev, mp, i, T, label):
    R, L, env, want = C_PROBES[i]
    return run_probes(_lib, dev, mp, T, L, env, want, label=label)


# ---- D: pitched rows with guards ------------------------------------------------------------------------------------------------------------
D_CASES = [(2, 2, 65533, None, "two col<64> side row0_bwd<du>+row_dk+corr chunks=1x2 chunks=1x2"),
           (3, 2, 4093, None, "oc spec<4>+conv<4> corr<4> dk<4,1> S=1")]


def suite_pitched(_lib, dev, mp, i, T, label):
    """inputs on empty_rows pitches with NaN between the rows, outputs handed to the C ABI with a sentinel between the rows: nothing
    between the rows is read (everything stays finite) or written, and the results are bitwise those of the packed call, which is itself held
    to the reference; with the forward's spectra and without"""
    B, D, L, env, want = D_CASES[i]
    st, ref = run_case(_lib, dev, mp, T, B, D, L, want, env=env, seed=3000 + i, label=label)
    u, k, b, dout = inputs(B, D, L, T, 3000 + i)
    ld = _lib.row_pitch(L)
    assert ld % 64 == 0 and 0 < ld - L < 64

    def pitched(t, fill):
        buf = torch.full(t.shape[:-1] + (ld,), fill, dtype=t.dtype, device=dev)
        buf[..., :L] = t.to(dev)
        return buf[..., :L], buf

    (up, ubuf), (kp, kbuf), (gp, gbuf) = pitched(u, NAN), pitched(k, NAN), pitched(dout, NAN)
    assert _lib.ld_of(up) == ld and _lib.ld_of(kp) == ld and _lib.ld_of(gp) == ld
    keep = [x.clone() for x in (ubuf, kbuf, gbuf)]
    bd = b.to(dev)
    lib = _lib.lib()
    code = _lib.dtype_code(T)
    with knobs(mp, env):
        tables = _lib.tables_for(dev, L)
        ws, stream = _lib.workspace_for(dev, lib.hyena_fftconv_workspace_bytes(B, D, L, 1, 0))
        for with_saved in (False, True):
            sp = torch.empty(_lib.saved_bytes(B, D, L), dtype=torch.uint8, device=dev) if with_saved else None
            outp, outbuf = pitched(torch.zeros_like(u), SENTINEL)
            dup, dubuf = pitched(torch.zeros_like(u), SENTINEL)
            dkp, dkbuf = pitched(torch.zeros_like(k), SENTINEL)
            db = torch.full((D,), SENTINEL, device=dev)
            with _lib._backend.guard(dev):
                _lib.check(lib.hyena_fftconv_fwd_ld(up.data_ptr(), kp.data_ptr(), bd.data_ptr(), outp.data_ptr(), B, D, L, ld, ld, code,
                                                    tables.data_ptr(), ws.data_ptr(), ws.numel(), 0, sp.data_ptr() if with_saved else None,
                                                    sp.numel() if with_saved else 0, stream))
                _lib.check(lib.hyena_fftconv_bwd_ld(gp.data_ptr(), up.data_ptr(), None if with_saved else kp.data_ptr(), bd.data_ptr(),
                                                    dup.data_ptr(), dkp.data_ptr(), db.data_ptr(), B, D, L, ld, ld, code, tables.data_ptr(),
                                                    ws.data_ptr(), ws.numel(), 0, sp.data_ptr() if with_saved else None,
                                                    sp.numel() if with_saved else 0, stream))
            for name, a, r in (("out", outp, ref[0]), ("du", dup, ref[1]), ("dk", dkp, ref[2]), ("dbias", db, ref[3])):
                assert same_bits(a.cpu(), r), (name, "pitched rows give other bits than packed ones", with_saved)
            for name, buf in (("out", outbuf), ("du", dubuf), ("dk", dkbuf)):
                assert bool((buf[..., L:] == SENTINEL).all()), (name, "written between the rows", with_saved)
    assert all(same_bits(a, c) for a, c in zip((ubuf, kbuf, gbuf), keep)), "an input was written"
    return st


# ---- E: the side stream off (a fresh process: the knob is read once per process) -----------------------------------------------------------
E_CASE = (2, 2, 65533, "two col<64> side row0_bwd<du>+row_dk+corr chunks=1x2 chunks=1x2")
E_TYPES = (F32, BF16)
E_SEED = 4000


def side_case_outputs(_lib, dev, T):
    """what both the parent and the child of the side-stream test compute: forward + full backward of E_CASE, on the host"""
    B, D, L, _ = E_CASE
    u, k, b, dout = inputs(B, D, L, T, E_SEED)
    return _call(_lib, dev, u, k, b, dout, (1, 1), False, 0)


# ---- the oracle's own figures over the case tables: `python -m tests.fftconv_local` (CPU only) ------------------------------------------------
def _all_shapes():
    for M1 in SUPPORTED_M1:
        for T in DTYPES:
            for i, L in enumerate(a_lengths(M1)):
                if not (i and T == F16):
                    yield "A", T, 1, 2, L, True, 7 * L + 3 + 2
    for i, (M1, B, chunk, need, saved, bias, T, want) in enumerate(B_CASES):
        yield "B", T, B, 3, 1024 * M1 - 3, bool(bias), 1000 + i
    for i, (R, B, D, L, need, saved, env, types, want) in enumerate(C_CASES):
        for T in types:
            yield "C", T, B, D, L, True, 2000 + i
    for i, (B, D, L, env, want) in enumerate(D_CASES):
        for T in (F32, BF16):
            yield "D", T, B, D, L, True, 3000 + i


def oracle_figures():
    """per table and size class: the fp32 oracle's figure per quantity, and for the 16-bit types the largest per-row share of elements of
    the oracle's rounded out / du that are not the rounded reference"""
    worst, flips, seen = {}, {}, set()
    for tab, T, B, D, L, bias, seed in _all_shapes():
        if (T, B, D, L, bias, seed) in seen:
            continue
        seen.add((T, B, D, L, bias, seed))
        u, k, b, dout = inputs(B, D, L, T, seed, bias)
        refs = ref64(u, k, b, dout)
        orc = oracle32(u, k, b, dout)
        figs = tuple(figure32(o, r) for o, r in zip(orc, refs))
        cls = size_class(L)
        worst[tab, cls] = tuple(max(a, c) for a, c in zip(worst.get((tab, cls), (0, 0, 0)), figs))
        if T != F32:
            sh = max(mismatch_share(orc[0].to(T), refs[0], T), mismatch_share(orc[1].to(T), refs[1], T))
            flips[tab, cls, NAME[T]] = max(flips.get((tab, cls, NAME[T]), 0.0), sh)
            if sh >= MISMATCH_CAP:
                print(f"  oracle above the cap: {tab} {NAME[T]} B={B} D={D} L={L} seed={seed} share={sh:.4f}", flush=True)
    for key in sorted(worst):
        print("oracle C (out, du, dk)", key, " ".join(f"{v:.1f}" for v in worst[key]), flush=True)
    for key in sorted(flips):
        print("oracle rounded: largest share of a row off the rounded reference", key, f"{flips[key]:.4f}", flush=True)
    return worst, flips


if __name__ == "__main__":
    oracle_figures()
