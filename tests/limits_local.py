"""The pitched entry points at their 32-bit offset limits: rows that lie gigabytes apart inside ONE allocation, so that a wrapped offset lands in
the same allocation -- on a poisoned band or on another row -- and shows as a wrong value, never as a fault.  Shared by tests/test_limits_emu.py
(address space reserved, not committed: only the touched pages cost memory) and tests/test_gpu_limits.py.  Plain torch; not a test file.  The table
of limits, the figures and the seeded defects: profiles/limits_local.md.

Every value is held to the fp64 reference and the derived bound of the module that owns the kernel (tests/fftconv_local.py, tests/shell_local.py,
tests/proj_local.py): no tolerance is made here.  The second check of a far-apart call -- bitwise the rows the same call gives at the package's
own pitch, _lib.row_pitch(L) -- is sharper but not independent.

Layout of a far-apart tensor (class Rows): row r starts at element r ld of an allocation whose first byte is the base pointer the kernel gets.
Nothing between the rows is filled.  A band of BAND bytes on either side of every row, and around the image of every row start modulo 2^32 bytes
and modulo 2^32 elements, is poisoned -- NaN for tensors the kernel reads, SENTINEL for tensors it writes -- and compared bit for bit afterwards.
No offset in the table is formed in a signed type, so nothing can wrap below the base: the allocations have no front padding."""
import math
import mmap

import numpy
import torch

from tests import fftconv_local as FL
from tests import proj_local as PL
from tests import shell_local as SL
from tests.shell_local import SENTINEL, half_ulp_io

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
NAN = float("nan")
BAND = 4096
G32 = 1 << 32
BAD_ARG = 1                                   # HYENA_ERR_BAD_ARG
ALIGN = 64                                    # _lib.ROW_ALIGN (asserted by the callers)
_INT = {4: torch.int32, 2: torch.int16}
_MAP_NORESERVE = getattr(mmap, "MAP_NORESERVE", 0x4000)
CAP_BYTES = 20 << 30                          # device memory one case may hold


def es_of(T):
    return torch.empty((), dtype=T).element_size()


def below(limit, step=ALIGN):
    """the largest multiple of `step` that is < limit"""
    return (limit - 1) // step * step


# ---- one allocation, a few rows far apart -------------------------------------------------------------------------------------------------
def _union(iv):
    out = []
    for a, b in sorted(iv):
        if out and a <= out[-1][1]:
            out[-1][1] = max(out[-1][1], b)
        elif b > a:
            out.append([a, b])
    return out


def _minus(iv, holes):
    for ha, hb in holes:
        nxt = []
        for a, b in iv:
            if hb <= a or ha >= b:
                nxt.append([a, b])
                continue
            if a < ha:
                nxt.append([a, ha])
            if hb < b:
                nxt.append([hb, b])
        iv = nxt
    return iv


class Rows:
    """`nrows` rows of L elements of type T, `ld` elements apart, in one allocation of ((nrows - 1) ld + L) es + BAND bytes; `fill` poisons the
    bands, and the rows until they get their values (NaN: an input; SENTINEL: an output).  values: (nrows, L) on the host, or None."""
    held = 0                                  # device bytes held by live instances (the cap is a condition of the cases, asserted here)

    def __init__(self, dev, T, nrows, L, ld, fill, values=None, starts=None):
        """starts: the rows' first elements where they are not r ld (FarBuf: rows of a strided tensor), ascending"""
        self.T, self.nrows, self.L, self.ld, self.es, self.fill, self.dev = T, nrows, L, ld, es_of(T), fill, dev
        assert ld >= L and nrows >= 1
        self.starts = [r * ld * self.es for r in range(nrows)] if starts is None else [x * self.es for x in starts]
        assert len(self.starts) == nrows and all(b - a >= L * self.es for a, b in zip(self.starts, self.starts[1:]))
        self.nbytes = self.starts[-1] + L * self.es + BAND
        if dev.type == "cpu":                  # reserved, not committed
            self._map = mmap.mmap(-1, self.nbytes, flags=mmap.MAP_PRIVATE | mmap.MAP_ANONYMOUS | _MAP_NORESERVE)
            self.bytes = torch.from_numpy(numpy.frombuffer(self._map, dtype=numpy.uint8))
        else:
            Rows.held += self.nbytes
            assert Rows.held <= CAP_BYTES, ("the case holds more device memory than its cap", Rows.held)
            self._map = None
            self.bytes = torch.empty(self.nbytes, dtype=torch.uint8, device=dev)
        self.ptr = self.bytes.data_ptr()
        rb = L * self.es
        starts = self.starts
        iv = []
        for s in starts:
            for m in {s, s % G32, (s // self.es) % G32 * self.es}:
                iv.append((max(m - BAND, 0), min(m + rb + BAND, self.nbytes)))
        self.bands = _minus(_union(iv), [(s, s + rb) for s in starts])
        self.touched = sum(b - a for a, b in self.bands) + nrows * rb
        for a, b in self.bands:
            self.bytes[a:b].view(T).fill_(fill)
        for r in range(nrows):
            if values is not None:
                self.row(r).copy_(values[r])
            else:
                self.row(r).fill_(fill)

    def row(self, r):
        s = self.starts[r]
        return self.bytes[s:s + self.L * self.es].view(self.T)

    def get(self):
        """the rows on the host, (nrows, L)"""
        return torch.stack([self.row(r).cpu() for r in range(self.nrows)])

    def bands_intact(self):
        """every poisoned band still holds its fill, bit for bit"""
        pat = torch.full((1,), self.fill, dtype=self.T).view(_INT[self.es])
        for a, b in self.bands:
            if not bool((self.bytes[a:b].view(_INT[self.es]).cpu() == pat).all()):
                return False
        return True

    def free(self):
        if self._map is None and self.bytes is not None:
            Rows.held -= self.nbytes
        self.bytes = None
        self._map = None


class FarBuf(SL.Buf):
    """tests/shell_local.py's Buf -- a storage the test owns and a strided logical view of it -- on a Rows allocation: nothing between the rows is
    filled, the bands around them are poisoned with `fill`.  What Buf checks on every element of its storage is checked here on every row and
    every band."""

    def __init__(self, shape, strides, dtype, dev, fill):
        import itertools
        self.shape, self.strides = tuple(shape), tuple(strides)
        assert self.strides[-1] == 1
        dev = torch.device(dev)
        starts = sorted(sum(i * st for i, st in zip(idx, self.strides[:-1])) for idx in itertools.product(*[range(n) for n in self.shape[:-1]]))
        self.rows = Rows(dev, dtype, len(starts), self.shape[-1], self.shape[-1], fill, starts=starts)
        n = starts[-1] + self.shape[-1]
        self.flat = self.rows.bytes[:n * self.rows.es].view(dtype)
        self.view = torch.as_strided(self.flat, self.shape, self.strides)

    def untouched(self, index):
        own = torch.zeros(self.shape, dtype=torch.bool, device=self.flat.device)
        own[index] = True
        return self.rows.bands_intact() and bool((self.view[~own] == SENTINEL).all())

    def same(self, other):
        return torch.equal(self.view, other.view) and self.rows.bands_intact() and other.rows.bands_intact()

    def __del__(self):
        self.flat = self.view = None
        self.rows.free()


def free_all(*rows):
    for r in rows:
        if r is not None:
            r.free()
    if torch.cuda.is_available():
        torch.cuda.empty_cache()


def _sync(dev):
    if dev.type == "cuda":
        torch.cuda.synchronize(dev)


def line(label, **figs):
    return f"[limits-local] {label} " + " ".join(f"{k}={v:.3g}" if isinstance(v, float) else f"{k}={v}" for k, v in figs.items())


# ---- the long convolution -----------------------------------------------------------------------------------------------------------------
# The limits of hyena_fftconv_fwd_ld / _bwd_ld by plan family (profiles/limits_local.md, rows F1 - F6), as functions of the shape: the first pitch
# that is refused (or, for the one-launch pair, handed to the general kernels), in elements.
def lim_rowoff(B, D, L, es):
    """B D ldx es < 2^32: the whole-tensor descriptors of small_fwd / small_bwd and of dk_kernel at T = 32"""
    return -(-G32 // (B * D * es))


def lim_small_ldk(D):
    """D ldk 4 < 2^32: small_fwd's descriptor over k"""
    return -(-G32 // (D * 4))


def lim_pair(L, es):
    """(ld + L) es < 2^32: the two-row window of spec_kernel / conv_kernel at R = 1"""
    return -(-G32 // es) - L


def cross(nrows, es):
    """no 32-bit offset: a pitch that puts the last of `nrows` rows just past 2^32 bytes (= 2^31 16-bit elements, 2^30 fp32 ones)"""
    return -(-(G32 // es) // ((nrows - 1) * ALIGN)) * ALIGN + ALIGN


# (name, type, B, D, L, knobs, route, which pitch is stretched, its limit (None: none short of INT_MAX -> cross()), what the call one ALIGN past the
#  limit does to (forward, backward): "refuse", "run" (another kernel takes it: held to the reference), None (not called), backward?, GPU shape)
# GPU shape: (B, D) to use on the device where B = D = 2 would hold more than CAP_BYTES (the forward's limit at R = 1 puts rows 4 GiB apart).
FFT_CASES = [
    ("small-ldx", BF16, 2, 2, 1021, None, "oc small_fwd<1> small_bwd<1>", "ldx", lambda B, D, L, es: lim_rowoff(B, D, L, es), ("run", "refuse"), True, None),
    ("small-ldk", BF16, 2, 2, 1021, None, "oc small_fwd<1> small_bwd<1>", "ldk", lambda B, D, L, es: lim_small_ldk(D), ("run", "run"), True, None),
    ("r1-fwd-ldx", BF16, 2, 2, 1021, {"SMALL": 0}, "oc spec<1>+conv<1> corr<1> dk<1,1> S=1", "ldx", lambda B, D, L, es: lim_pair(L, es), ("refuse", "refuse"), False, (1, 3)),
    ("r1-bwd-ldx", F32, 2, 2, 1021, {"SMALL": 0}, "oc spec<1>+conv<1> corr<1> dk<1,1> S=1", "ldx", lambda B, D, L, es: lim_rowoff(B, D, L, es), ("run", "refuse"), True, None),
    ("r1-ldk", BF16, 2, 2, 1021, {"SMALL": 0}, "oc spec<1>+conv<1> corr<1> dk<1,1> S=1", "ldk", lambda B, D, L, es: lim_pair(L, 4), ("refuse", "refuse"), True, None),
    ("r4-ldx", BF16, 2, 2, 4093, None, "oc spec<4>+conv<4> corr<4> dk<4,1> S=1", "ldx", None, None, True, None),
    ("r4-ldk", BF16, 2, 2, 4093, None, "oc spec<4>+conv<4> corr<4> dk<4,1> S=1", "ldk", None, None, True, None),
    ("dk1-ldx", F32, 1, 2, 32765, None, "oc spec<32>+conv<32> corr<32> conv<32,f32out>", "ldx", None, None, True, None),
    ("sliced-ldx", BF16, 5, 2, 4093, None, "oc spec<4>+conv<4> corr<4> dk<4,1> S=2 ragged=1", "ldx", None, None, True, None),
    ("two-ldx", BF16, 2, 2, 32771, None, "two col<64> side row0_bwd<du>+row_dk+corr chunks=1x2 chunks=1x2", "ldx", None, None, True, None),
    ("two-ldk", BF16, 2, 2, 32771, None, "two col<64> side row0_bwd<du>+row_dk+corr chunks=1x2 chunks=1x2", "ldk", None, None, True, None),
]
FFT_IDS = [c[0] for c in FFT_CASES]


def _fft_call(_lib, dev, T, B, D, L, ldx, ldk, data, bwd):
    """forward (and backward) through the C ABI on Rows at the given pitches -> (status fwd, status bwd, (out, du, dk, dbias) on the host, intact)"""
    u, k, b, dout = data
    lib, code = _lib.lib(), _lib.dtype_code(T)
    tables = _lib.tables_for(dev, L)
    ws, stream = _lib.workspace_for(dev, lib.hyena_fftconv_workspace_bytes(B, D, L, 1, 0))
    bd = b.to(dev)
    U_ = Rows(dev, T, B * D, L, ldx, NAN, u.reshape(B * D, L))
    K_ = Rows(dev, F32, D, L, ldk, NAN, k)
    O_ = Rows(dev, T, B * D, L, ldx, SENTINEL)
    G_ = DU_ = DK_ = None
    db = torch.full((D,), SENTINEL, device=dev)
    try:
        with _lib._backend.guard(dev):
            s1 = lib.hyena_fftconv_fwd_ld(U_.ptr, K_.ptr, bd.data_ptr(), O_.ptr, B, D, L, ldx, ldk, code, tables.data_ptr(), ws.data_ptr(), ws.numel(),
                                          0, None, 0, stream)
            s2 = None
            if bwd:
                G_ = Rows(dev, T, B * D, L, ldx, NAN, dout.reshape(B * D, L))
                DU_ = Rows(dev, T, B * D, L, ldx, SENTINEL)
                DK_ = Rows(dev, F32, D, L, ldk, SENTINEL)
                s2 = lib.hyena_fftconv_bwd_ld(G_.ptr, U_.ptr, K_.ptr, bd.data_ptr(), DU_.ptr, DK_.ptr, db.data_ptr(), B, D, L, ldx, ldk, code,
                                              tables.data_ptr(), ws.data_ptr(), ws.numel(), 0, None, 0, stream)
        _sync(dev)
        got = (O_.get().view(B, D, L), None if DU_ is None else DU_.get().view(B, D, L), None if DK_ is None else DK_.get(), db.cpu())
        intact = {n: r.bands_intact() for n, r in (("u", U_), ("k", K_), ("out", O_), ("dout", G_), ("du", DU_), ("dk", DK_)) if r is not None}
        touched = sum(r.touched for r in (U_, K_, O_, G_, DU_, DK_) if r is not None)
    finally:
        free_all(U_, K_, O_, G_, DU_, DK_)
    return s1, s2, got, intact, touched


def _fft_refused(_lib, dev, T, B, D, L, ldx, ldk, fwd, bwd):
    """the call one alignment unit past the limit, on buffers of a few elements: HYENA_ERR_BAD_ARG before anything is dereferenced or launched"""
    lib, code = _lib.lib(), _lib.dtype_code(T)
    tables = _lib.tables_for(dev, L)
    ws, stream = _lib.workspace_for(dev, lib.hyena_fftconv_workspace_bytes(B, D, L, 1, 0))
    mk = lambda dt: torch.full((64,), SENTINEL, dtype=dt, device=dev)      # noqa: E731
    x, o, g, du, kk, dk, db, bias = mk(T), mk(T), mk(T), mk(T), mk(F32), mk(F32), mk(F32), mk(F32)
    with _lib._backend.guard(dev):
        if fwd:
            assert lib.hyena_fftconv_fwd_ld(x.data_ptr(), kk.data_ptr(), bias.data_ptr(), o.data_ptr(), B, D, L, ldx, ldk, code, tables.data_ptr(),
                                            ws.data_ptr(), ws.numel(), 0, None, 0, stream) == BAD_ARG, "the forward takes a pitch past its limit"
        if bwd:
            assert lib.hyena_fftconv_bwd_ld(g.data_ptr(), x.data_ptr(), kk.data_ptr(), bias.data_ptr(), du.data_ptr(), dk.data_ptr(), db.data_ptr(), B, D,
                                            L, ldx, ldk, code, tables.data_ptr(), ws.data_ptr(), ws.numel(), 0, None, 0, stream) == BAD_ARG, \
                "the backward takes a pitch past its limit"
    _sync(dev)
    for t in (x, o, g, du, kk, dk, db, bias):
        assert bool((t == SENTINEL).all()), "a refused call wrote"


def _fft_hold(name, T, L, B, got, ref, bwd):
    out, du, dk, db = got
    r_out, r_du, r_dk, r_db = ref
    Co, Cu, Ck = FL.c_bound(L)
    st = FL.Stats()
    st.hold("out", out, r_out, Co, T)
    if bwd:
        st.hold("du", du, r_du, Cu, T)
        st.hold32("dk", dk, r_dk, Ck)
        e = float((db.double() - r_db).abs().max())
        st.put("dbias/bound", e / (3e-6 * math.sqrt(B * L) + 1e-6))
        assert e < 3e-6 * math.sqrt(B * L) + 1e-6, (name, "dbias", e)
    return st


def fft_case(_lib, dev, mp, i, label=""):
    name, T, B, D, L, env, want, which, limit, past, bwd, gpu_shape = FFT_CASES[i]
    assert _lib.ROW_ALIGN == ALIGN
    if dev.type == "cuda" and gpu_shape is not None:
        B, D = gpu_shape
        want = None                                   # (the route string names the emulator's shape)
    es = es_of(T)
    ld0 = _lib.row_pitch(L)
    rows = B * D if which == "ldx" else D
    first_bad = None if limit is None else limit(B, D, L, es)
    far = cross(rows, es if which == "ldx" else 4) if limit is None else below(first_bad)
    assert far < 2 ** 31 and far % ALIGN == 0
    ldx, ldk = (far, ld0) if which == "ldx" else (ld0, far)
    data = FL.inputs(B, D, L, T, 9000 + i)
    ref = FL.ref64(*data)
    with FL.knobs(mp, env):
        if want is not None:
            got_route = FL.route(_lib, B, D, L)
            assert got_route == want, ("the case no longer reaches the code it was written for", got_route, want)
        s1, s2, base, intact0, _ = _fft_call(_lib, dev, T, B, D, L, ld0, ld0, data, bwd)
        assert s1 == 0 and (not bwd or s2 == 0) and all(intact0.values()), (name, "at the package's own pitch", s1, s2, intact0)
        _fft_hold(name, T, L, B, base, ref, bwd)
        # just inside the limit (or, where there is none, across 2^32 bytes)
        s1, s2, got, intact, touched = _fft_call(_lib, dev, T, B, D, L, ldx, ldk, data, bwd)
        assert s1 == 0 and (not bwd or s2 == 0), (name, "refused inside its limit", s1, s2)
        st = _fft_hold(name, T, L, B, got, ref, bwd)
        assert all(intact.values()), (name, "a poisoned band was touched", intact)
        for n, a, c in zip(("out", "du", "dk", "dbias"), got, base):
            assert FL.same_bits(a, c), (name, n, "far-apart rows give other bits than the package's pitch")
    # the module's own runner on the same far-apart inputs, through the Python wrappers (which hand the inputs' pitch on and make out / du / dk at
    # it): route, every bound, types, a second call the same bits -- and the bits of the calls above
    if bwd:
        def place(t, kind):
            ld = ldx if kind == "x" else ldk
            return FarBuf.input(t.to(dev), (D * ld, ld, 1) if t.dim() == 3 else (ld, 1)).view
        _, again = FL.run_case(_lib, dev, mp, T, B, D, L, want, env=env, seed=9000 + i, label=f"{label} limits {name}", place=place)
        for n, a, c in zip(("out", "du", "dk", "dbias"), again, got):
            assert FL.same_bits(a, c), (name, n, "the wrappers on far-apart rows give other bits than the C ABI")
        import gc
        gc.collect()
        free_all()
    with FL.knobs(mp, env):
        # one alignment unit past it
        if first_bad is not None:
            bad = below(first_bad) + ALIGN
            assert bad >= first_bad
            bx, bk = (bad, ld0) if which == "ldx" else (ld0, bad)
            # first on whole far-apart tensors: a call that is NOT refused then runs on memory it owns and shows by value, not by a fault
            s1, s2, got2, intact2, _ = _fft_call(_lib, dev, T, B, D, L, bx, bk, data, bwd)
            assert all(intact2.values()), (name, "past the limit: a poisoned band was touched", intact2)
            untouched = lambda t: bool((t == SENTINEL).all())      # noqa: E731
            if past[0] == "refuse":
                assert s1 == BAD_ARG and untouched(got2[0]), (name, "the forward takes a pitch past its limit", s1)
            else:                                      # another kernel takes the call: the same reference and bound
                assert s1 == 0, (name, "forward past the one-launch limit", s1)
                _fft_hold(name, T, L, B, got2, ref, False)
            if bwd and past[1] == "refuse":
                assert s2 == BAD_ARG and all(untouched(t) for t in got2[1:]), (name, "the backward takes a pitch past its limit", s2)
            elif bwd:
                assert s1 == 0 and s2 == 0, (name, "backward past the one-launch limit", s1, s2)
                _fft_hold(name, T, L, B, got2, ref, True)
            # then on buffers of a few elements: the refusal comes before anything is dereferenced
            _fft_refused(_lib, dev, T, B, D, L, bx, bk, past[0] == "refuse", bwd and past[1] == "refuse")
    print(line(f"{label} fftconv {name} {SL.NAME[T]} B={B} D={D} L={L} {which}={far} first_refused={first_bad} touched_KiB={touched >> 10} | {want} |",
               **dict(st)), flush=True)
    return st, touched


# ---- in_proj + the front of the shell: ldv ------------------------------------------------------------------------------------------------
def lim_ldv(D):
    """(D - 9) ldv + 56 < 2^32 ELEMENTS: inproj_pre_fwd_kernel's voff0 (generation 1)"""
    return -(-(G32 - 56) // (D - 9))


INPROJ_SHAPE = (2, 201, 197, 128)             # B, Lx, Lc, D: one channel group of 64 x 2, whole + ragged tiles, tiles inside and across the sequences


def inproj_case(_lib, dev, T, label=""):
    B, Lx, Lc, D = INPROJ_SHAPE
    lib, rp = _lib.lib(), _lib.row_pitch
    code, stream = _lib.dtype_code(T), _lib._backend.stream(dev)
    assert _lib.proj_kernel_generation(1) == 1 and _lib.proj_supported(B, Lx, D, T)
    g = torch.Generator().manual_seed(77)
    w, b, bin_ = SL._params(3 * D, g, dev, True)
    u, W = PL._op((B, Lx, D), g, T, dev), PL._op((3 * D, D), g, T, dev, PL.W_SCALE)
    xs, csx, bsx = SL.x_strides(3 * D, B, Lx, "cm", rp)
    first_bad = lim_ldv(D)
    step = 8                                          # 16-byte stores: the alignment unit of ldv
    far = below(first_bad, ALIGN)
    assert (D - 9) * far + 56 < G32 <= (D - 9) * (far + ALIGN) + 56

    def call(ldv):
        xT = SL.Buf((3 * D, B, Lx), xs, T, dev, SENTINEL)
        vg = Rows(dev, T, B * D, Lc, ldv, SENTINEL)
        with _lib._backend.guard(dev):
            s = lib.hyena_inproj_pre_fwd_ld(u.data_ptr(), W.data_ptr(), SL._ptr(bin_), w.data_ptr(), b.data_ptr(), xT.flat.data_ptr(), vg.ptr, B, Lx, Lc, D,
                                            csx, bsx, ldv, code, stream)
        _sync(dev)
        got, ok, touched = vg.get().view(B, D, Lc), vg.bands_intact(), vg.touched
        free_all(vg)
        return s, xT, got, ok, touched
    s, xT0, vg0, ok0, _ = call(rp(Lc))
    assert s == 0 and ok0
    s, xT, vg, ok, touched = call(far)
    assert s == 0, "refused inside its limit"
    st = PL._Stats()
    ref, E32 = PL.product64(W.double(), u.double().reshape(B * Lx, D))
    PL._hold16(st, "xT", xT, (slice(None),) * 3, ref.view(3 * D, B, Lx), E32.view(3 * D, B, Lx), T)
    rv, Ev = SL.pre_fwd64(xT.view.double().cpu(), SL._d(bin_).cpu(), w.double().cpu(), b.double().cpu(), Lc)
    assert bool(torch.isfinite(vg).all()), "vg: not finite (a row was not written)"
    st.hold("vg", vg, rv, Ev + half_ulp_io(rv.abs() + Ev, T))
    assert ok, "vg: a poisoned band was written"
    assert torch.equal(xT.flat, xT0.flat) and FL.same_bits(vg, vg0), "far-apart vg rows give other bits than the package's pitch"
    # one alignment unit past the limit: first on whole far-apart tensors (a call that is NOT refused then shows by value), then on buffers of a few
    # elements (the refusal comes before anything is dereferenced)
    s, xTb, vgb, okb, _ = call(far + ALIGN)
    assert s == BAD_ARG and okb and bool((vgb == SENTINEL).all()) and bool((xTb.flat == SENTINEL).all()), ("a vg pitch past the limit is taken", s, okb)
    small = [torch.full((64,), SENTINEL, dtype=T, device=dev) for _ in range(4)]
    f32s = [torch.full((64,), SENTINEL, device=dev) for _ in range(3)]
    bad = below(first_bad, step) + step
    assert bad >= first_bad
    for ldv in (bad, far + ALIGN):
        with _lib._backend.guard(dev):
            assert lib.hyena_inproj_pre_fwd_ld(small[0].data_ptr(), small[1].data_ptr(), f32s[0].data_ptr(), f32s[1].data_ptr(), f32s[2].data_ptr(),
                                               small[2].data_ptr(), small[3].data_ptr(), B, Lx, Lc, D, csx, bsx, ldv, code, stream) == BAD_ARG, ldv
        # the channel stride of xT: csx < 2^31 (stricter than the kernel text needs -- the offsets are 64-bit -- but the contract of the header)
        for bad_csx in (1 << 31, (1 << 31) + 8):
            with _lib._backend.guard(dev):
                assert lib.hyena_inproj_pre_fwd_ld(small[0].data_ptr(), small[1].data_ptr(), f32s[0].data_ptr(), f32s[1].data_ptr(), f32s[2].data_ptr(),
                                                   small[2].data_ptr(), small[3].data_ptr(), B, Lx, Lc, D, bad_csx, bsx, rp(Lc), code, stream) == BAD_ARG, bad_csx
    _sync(dev)
    assert all(bool((t == SENTINEL).all()) for t in small + f32s), "a refused call wrote"
    # generation 2 forms the vg offsets in 64 bits: it takes the pitch generation 1 refuses, and is held to the same reference there
    prev = PL._generation(_lib, 1, 2)
    try:
        s, xT2, vg2, ok2, _ = call(far + ALIGN)
    finally:
        _lib.proj_kernel_generation(1, prev)
    assert s == 0 and ok2, ("generation 2 past generation 1's limit", s, ok2)
    PL._hold16(st, "xT.gen2", xT2, (slice(None),) * 3, ref.view(3 * D, B, Lx), E32.view(3 * D, B, Lx), T)
    rv2, Ev2 = SL.pre_fwd64(xT2.view.double().cpu(), SL._d(bin_).cpu(), w.double().cpu(), b.double().cpu(), Lc)
    assert bool(torch.isfinite(vg2).all()), "vg (generation 2): a row was not written"
    st.hold("vg.gen2", vg2, rv2, Ev2 + half_ulp_io(rv2.abs() + Ev2, T))
    print(line(f"{label} inproj_pre_fwd {SL.NAME[T]} B={B} Lx={Lx} Lc={Lc} D={D} ldv={far} first_refused={first_bad} touched_KiB={touched >> 10}", **dict(st)),
          flush=True)
    return st, touched


# ---- the channel-major shell: every offset is 64-bit, rows across 2^32 bytes ---------------------------------------------------------------
CM_SHAPE = (2, 1021, 1023, 2)                 # B, L, Lx, D: odd lengths, a ragged vector at the end, two rows per workgroup


def cm_case(_lib, dev, T, which, label=""):
    """tests/shell_local.py's run_cm -- cm_pre_fwd, cm_post_fwd, cm_post_bwd, cm_pre_bwd, every reference, bound, sentinel and repeat of it -- with
    the (B, D, L) tensors (which = "lda") or xT / dxT (which = "csx") on rows whose last one starts just past 2^32 bytes"""
    B, L, Lx, D = CM_SHAPE
    es = es_of(T)
    if which == "lda":
        far = cross(B * D, es)
        st = SL.run_cm(_lib, dev, T, B, L, Lx, D, xlayout="cm", rows=True, seed=78, label=label + " limits lda=%d" % far, lda=far, rowbuf=FarBuf)
    else:
        far = cross(3 * D, es)
        st = SL.run_cm(_lib, dev, T, B, L, Lx, D, xlayout="cm", rows=True, seed=79, label=label + " limits csx=%d" % far, csx=far, xbuf=FarBuf)
    import gc
    gc.collect()
    free_all()
    print(line(f"{label} cm_pre_fwd+post_fwd+post_bwd+pre_bwd {SL.NAME[T]} B={B} L={L} Lx={Lx} D={D} {which}={far}", **{k: float(v) for k, v in st.items()}),
          flush=True)
    return st


# ---- packed tensors past 2^32 bytes, at real size (device only) -----------------------------------------------------------------------------
# The packed entry points have no pitch to stretch.  Inputs are filled on the device from a seeded generator; the fp64 reference is computed for a
# fixed sample of rows -- the first, the last, and the rows on either side of each 2^31-element / 2^32-byte crossing -- within the bounds of the
# module that owns the kernel.
def crossing_rows(nrows, rowlen, es):
    """first, last, and the two rows around every multiple of 2^31 bytes inside a packed (nrows, rowlen) tensor of es-byte elements (2^31 bytes:
    a signed byte offset; 2^32 bytes = 2^31 16-bit elements; 2^33 bytes = 2^31 fp32 elements ...)"""
    rows = {0, nrows - 1}
    m = 1
    while m * (1 << 31) < nrows * rowlen * es:
        r = m * (1 << 31) // (rowlen * es)           # the row that holds the crossing (or starts at it)
        rows.update(x for x in (r - 1, r, r + 1) if 0 <= x < nrows)
        m += 1
    return sorted(rows)


def packed_add_norm(_lib, dev, label=""):
    """add_norm_fwd on (rows, 256) bf16, rows D just past 2^31 elements (no residual input, no dropout: 4 + 4 + 8 GiB)"""
    from tests import block_local as BL
    D, T = 256, BF16
    rows = (1 << 23) + 64
    assert rows * D > 1 << 31
    g = torch.Generator(device=dev).manual_seed(501)
    x0 = torch.randn((rows, D), generator=g, device=dev, dtype=T)
    w, b = BL.draw_params(D, torch.Generator().manual_seed(502), dev)
    out, ro, mean, rstd = _lib.add_norm_fwd(x0, None, w, b, BL.EPS, T)
    _sync(dev)
    sample = sorted(set(crossing_rows(rows, D, 2)) | set(crossing_rows(rows, D, 4)))
    idx = torch.tensor(sample, device=dev)
    R = BL.fwd64(x0[idx].double(), None, w.double(), b.double(), None, 1.0)
    st = BL._Stats()
    st.hold("res_out", ro[idx], R["r"], R["e_r"])
    st.hold("mean", mean[idx], R["mean"], R["e_m"])
    st.hold("rstd", rstd[idx], R["rstd"], R["e_s"])
    st.hold("out", out[idx], R["out"], R["E_out"] + half_ulp_io(R["out"].abs() + R["E_out"], T))
    print(line(f"{label} add_norm_fwd bf16 rows={rows} D={D} elements=2^31+{rows * D - (1 << 31)} sampled_rows={len(sample)}", **dict(st)), flush=True)
    return st


def packed_cm(_lib, dev, label=""):
    """cm_pre_fwd + cm_post_fwd, packed, B L just past 2^23 at D = 256, bf16: xT is 3 x 2^32 bytes, vg / y / zT 2^32 bytes each.  xT + y + zT would
    hold 85 KiB more than CAP_BYTES: cm_post_fwd gets the channel rows [0, D) of xT alone, the only ones it reads."""
    B, L, D, T = 9, 932077, 256, BF16
    assert B * L > 1 << 23
    lib, code, stream = _lib.lib(), _lib.dtype_code(T), _lib._backend.stream(dev)
    gd = torch.Generator(device=dev).manual_seed(503)
    w, b, bin_ = SL._params(3 * D, torch.Generator().manual_seed(504), dev, True)
    xT = torch.randn((3 * D, B, L), generator=gd, device=dev, dtype=T)
    vg = torch.empty((B, D, L), device=dev, dtype=T)
    with _lib._backend.guard(dev):
        _lib.check(lib.hyena_cm_pre_fwd(xT.data_ptr(), bin_.data_ptr(), w.data_ptr(), b.data_ptr(), vg.data_ptr(), B, L, L, D, code, stream))
    _sync(dev)
    st = SL._Stats()
    # (b, d): flat xT rows 2304 = (256, 0) and 4608 = (512, 0) start just past 2^31 / 2^32 elements, 4607 = (511, 8) and 6911 = (767, 8) hold a crossing
    pre_rows = [(0, 0), (8, 255), (4, 100)]
    for bi, d in pre_rows:
        ch = [d, D + d, 2 * D + d]
        ref, E = SL.pre_fwd64(xT[ch, bi:bi + 1].double().cpu(), bin_[ch].double().cpu(), w[ch].double().cpu(), b[ch].double().cpu(), L)
        st.hold("pre_fwd", vg[bi, d].cpu()[None, None], ref, E + half_ulp_io(ref.abs() + E, T))
    x0 = xT[:D].clone()                                                  # channel rows [0, D): what cm_post_fwd reads
    del xT
    torch.cuda.empty_cache()
    zT = torch.empty((D, B, L), device=dev, dtype=T)
    with _lib._backend.guard(dev):
        _lib.check(lib.hyena_cm_post_fwd(vg.data_ptr(), x0.data_ptr(), bin_.data_ptr(), w.data_ptr(), b.data_ptr(), zT.data_ptr(), B, L, L, D, code, stream))
    _sync(dev)
    # (d, b): flat rows 0, 2303 = (255, 8) -- it holds the 2^31-element crossing of xT, y and zT alike -- and one in between
    for d, bi in [(0, 0), (255, 8), (100, 4)]:
        ch = [d, d, d]                                                   # (post_fwd64 reads the first third of its x)
        ref, E = SL.post_fwd64(x0[ch, bi:bi + 1].double().cpu(), bin_[ch].double().cpu(), w[ch].double().cpu(), b[ch].double().cpu(),
                               vg[bi:bi + 1, d:d + 1].double().cpu(), L)
        st.hold("post_fwd", zT[d, bi].cpu()[None, None], ref, E + half_ulp_io(ref.abs() + E, T))
    print(line(f"{label} cm_pre_fwd+cm_post_fwd packed bf16 B={B} L={L} D={D} B*L=2^23+{B * L - (1 << 23)}", **dict(st)), flush=True)
    return st


def packed_fftconv(_lib, dev, mp, label=""):
    """fftconv_fwd on the two-level plan, D = 256, bf16, L just past 32768, the smallest B with B D L es > 2^32"""
    D, L, T = 256, 33789, BF16
    B = (1 << 32) // (D * L * 2) + 1
    assert (B - 1) * D * L * 2 <= 1 << 32 < B * D * L * 2 and B == 249
    with FL.knobs(mp, None):
        assert _lib.lib().hyena_fftconv_plan(L) == _lib.PLAN_TWO_LEVEL and _lib.lib().hyena_fftconv_fft_size(L) == 65536
        gd = torch.Generator(device=dev).manual_seed(505)
        u = torch.randn((B, D, L), generator=gd, device=dev, dtype=T)
        gh = torch.Generator().manual_seed(506)
        k = (torch.randn(D, L, generator=gh) / math.sqrt(L)).to(dev)
        bias = torch.randn(D, generator=gh).to(dev)
        out = _lib.fftconv_fwd(u, k, bias, grad=False)
        _sync(dev)
    st = FL.Stats()
    sample = crossing_rows(B * D, L, 2)
    for r in sample:
        bi, d = divmod(r, D)
        ref = FL.ref64(u[bi:bi + 1, d:d + 1].cpu(), k[d:d + 1].cpu(), bias[d:d + 1].cpu(), u[bi:bi + 1, d:d + 1].cpu())[0]
        st.hold("out", out[bi:bi + 1, d:d + 1].cpu(), ref, FL.c_bound(L)[0], T)
    print(line(f"{label} fftconv_fwd two-level bf16 B={B} D={D} L={L} bytes=2^32+{B * D * L * 2 - (1 << 32)} sampled_rows={len(sample)}", **dict(st)),
          flush=True)
    return st


# ---- the implicit filter: D ldk 4 <= 2^31 ----------------------------------------------------------------------------------------------------
FILTER_SHAPE = (64, 133, 5)                   # D, L, E: three workgroups of positions, the last one ragged


def filter_case(_lib, dev, label=""):
    """hyena_filter_fwd_ld / _bwd_ld (fp32) with k and dk on far-apart rows at the largest pitch flt_pitch_ok admits; the references and bounds of
    tests/filter_local.py.  (The refusal on buffers of a few floats: tests/test_filter_local_emu.py::test_row_pitch_beyond_32_bit_offsets_is_rejected.)"""
    import ctypes
    from tests import filter_local as FLoc
    D, L, E = FILTER_SHAPE
    shift, modulate = 0.0, True
    args = FLoc.make_case(D, L, E, seed=3, device=dev)
    lib, stream = _lib.lib(), _lib._backend.stream(dev)
    P = int(lib.hyena_filter_row_pitch(L))
    eps_m = FLoc.eps_m_for(_lib, dev)
    first_bad = (1 << 29) // D + 1
    far = below(first_bad)
    assert D * far * 4 <= 1 << 31 < D * (far + ALIGN) * 4
    dk = torch.randn(D, L, generator=torch.Generator().manual_seed(5))
    names = ("dw0", "db0", "dw1", "db1", "dw2", "db2", "dw3", "dfreq")

    def call(ldk):
        p = FLoc._params(_lib, args, shift, modulate)
        K, G = Rows(dev, F32, D, L, ldk, SENTINEL), Rows(dev, F32, D, L, ldk, NAN, dk)
        saved = FLoc.poison((3, 64, P), dev)
        outs = {n: FLoc.poison(tuple(args[i].shape), dev) for n, i in zip(names, range(2, 10))}
        outs["dz"] = FLoc.poison((E, L), dev)
        g = _lib.FilterGrads()
        for n, ten in outs.items():
            setattr(g, n, ten.data_ptr())
        nbytes = int(lib.hyena_filter_workspace_bytes(L, D))
        ws = FLoc.poison((nbytes // 4,), dev)
        with _lib._backend.guard(dev):
            s1 = lib.hyena_filter_fwd_ld(ctypes.byref(p), K.ptr, ldk, saved.data_ptr(), stream)
            s2 = lib.hyena_filter_bwd_ld(ctypes.byref(p), G.ptr, ldk, saved.data_ptr(), ctypes.byref(g), ws.data_ptr(), nbytes, stream)
        _sync(dev)
        r = (s1, s2, K.get(), saved, outs, ws, K.bands_intact() and G.bands_intact(), K.touched + G.touched)
        free_all(K, G)
        return r
    s1, s2, k0, saved0, outs0, _, ok0, _ = call(_lib.row_pitch(L))
    assert s1 == 0 and s2 == 0 and ok0
    s1, s2, k, saved, outs, ws, ok, touched = call(far)
    assert s1 == 0 and s2 == 0, ("refused inside its limit", s1, s2)
    acts = [saved[s][:, :L] for s in range(3)]
    fw, max_arg = FLoc.forward_check(k.to(dev), acts, args, shift, modulate, eps_m)
    bw = FLoc.backward_check(outs, ws, dk.to(dev), acts, args, shift, modulate, eps_m, True)
    assert max_arg <= FLoc.SINCOS_RANGE
    for name, v in list(fw.worst.items()) + list(bw.worst.items()):
        assert v <= 1.0, (name, v)
    assert ok, "a poisoned band was touched"
    assert FL.same_bits(k, k0) and all(torch.equal(outs[n], outs0[n]) for n in outs), "far-apart rows give other bits than the package's pitch"
    # one alignment unit past the limit, on whole tensors: refused, nothing written
    s1, s2, kb, savedb, outsb, _, okb, _ = call(far + ALIGN)
    assert s1 == BAD_ARG and s2 == BAD_ARG and okb and bool((kb == SENTINEL).all()) and FLoc.is_poison(savedb) and all(FLoc.is_poison(t) for t in outsb.values())
    print(line(f"{label} filter_fwd+filter_bwd fp32 D={D} L={L} E={E} ldk={far} first_refused={first_bad} touched_KiB={touched >> 10} fwd: {fw.line()} | bwd: {bw.line()}"),
          flush=True)
    return touched


def filter16_case(_lib, dev, T, label=""):
    """hyena_filter16_fwd_ld / _bwd_ld (the graph under autocast of type T; k and dk are fp32, the limit is K1's) with k and dk on far-apart rows at
    the largest pitch flt_pitch_ok admits: the statistics and conditions of tests/filter16_local.py's check_local, bitwise the call at the package's
    own pitch, and the refusal one alignment unit further on whole tensors"""
    import ctypes
    from tests import filter16_local as F16
    from tests import filter_local as FLoc
    D, L, E = FILTER_SHAPE
    shift, modulate = 0.0, True
    args = FLoc.make_case(D, L, E, seed=3, device=dev)
    lib, stream, code = _lib.lib(), _lib._backend.stream(dev), _lib.dtype_code(T)
    P = int(lib.hyena_filter_row_pitch(L))
    first_bad = (1 << 29) // D + 1
    far = below(first_bad)
    dk = torch.randn(D, L, generator=torch.Generator().manual_seed(6))
    names = ("dw0", "db0", "dw1", "db1", "dw2", "db2", "dw3", "dfreq")

    def call(ldk):
        p = _lib._filter_params(*args, shift, modulate)
        K, G = Rows(dev, F32, D, L, ldk, SENTINEL), Rows(dev, F32, D, L, ldk, NAN, dk)
        saved = torch.full((3, 32, P), F16.S_SENTINEL, dtype=torch.int32, device=dev)
        outs = {n: FLoc.poison(tuple(args[i].shape), dev) for n, i in zip(names, range(2, 10))}
        dzt = FLoc.poison((E, L), dev)
        g = _lib.FilterGrads()
        for n, ten in outs.items():
            setattr(g, n, ten.data_ptr())
        g.dz = dzt.data_ptr()
        nbytes = int(lib.hyena_filter_workspace_bytes(L, D))
        ws = FLoc.poison((nbytes // 4,), dev)
        with _lib._backend.guard(dev):
            s1 = lib.hyena_filter16_fwd_ld(ctypes.byref(p), code, K.ptr, ldk, saved.data_ptr(), stream)
            s2 = lib.hyena_filter16_bwd_ld(ctypes.byref(p), code, G.ptr, ldk, saved.data_ptr(), ctypes.byref(g), ws.data_ptr(), nbytes, stream)
        _sync(dev)
        r = (s1, s2, K.get(), saved, [outs[n] for n in names] + [dzt], K.bands_intact() and G.bands_intact(), K.touched + G.touched)
        free_all(K, G)
        return r
    s1, s2, k0, saved0, g0, ok0, _ = call(_lib.row_pitch(L))
    assert s1 == 0 and s2 == 0 and ok0
    s1, s2, k, saved, grads, ok, touched = call(far)
    assert s1 == 0 and s2 == 0, ("refused inside its limit", s1, s2)
    assert bool(torch.isfinite(k).all()) and bool((saved[:, :, L:] == F16.S_SENTINEL).all())
    acts = F16.decode_saved(saved, L, T)
    fwd = F16.forward_stats(k.to(dev), acts, args, shift, modulate, T)
    assert fwd["max_arg"] <= F16.SINCOS_RANGE and fwd["viol_a"] == [0, 0, 0] and fwd["viol_k"] == 0, fwd
    assert all(x <= (1e-2 if T == BF16 else 2e-2) for x in fwd["ambiguous"]) and all(x < 1e-2 for x in fwd["inexact"]), fwd      # conditions on the input
    got = [x if i < 8 else x.t().contiguous() for i, x in enumerate(grads)]           # dz arrives as (E, L)
    bwd = F16.backward_stats(got, dk.to(dev), acts, args, shift, modulate, T)
    for n, (e, nn) in bwd.items():
        assert e < nn / 4, (n, e, nn)
    assert ok, "a poisoned band was touched"
    assert FL.same_bits(k, k0) and torch.equal(saved[:, :, :L], saved0[:, :, :L]) and all(torch.equal(a, c) for a, c in zip(grads, g0)), \
        "far-apart rows give other bits than the package's pitch"
    s1, s2, kb, savedb, gb, okb, _ = call(far + ALIGN)
    assert s1 == BAD_ARG and s2 == BAD_ARG and okb and bool((kb == SENTINEL).all()) and bool((savedb == F16.S_SENTINEL).all()) and \
        all(FLoc.is_poison(t) for t in gb), ("a pitch past the limit is taken", s1, s2)
    print(line(f"{label} filter16_fwd+filter16_bwd {SL.NAME[T]} D={D} L={L} E={E} ldk={far} first_refused={first_bad} touched_KiB={touched >> 10} "
               f"viol_a={fwd['viol_a']} viol_k={fwd['viol_k']} " + " ".join(f"{n}:E={e:.3g},N={nn:.3g}" for n, (e, nn) in bwd.items())), flush=True)
    return touched


# ---- out_proj: the row pitch of y (forward, both generations) and of y / dyc (input gradient) ------------------------------------------------
OUTPROJ_SHAPE = (2, 201, 203, 128)            # B, L, Lx, D: whole tiles, a pulled-back last tile, the truncated operator (Lx > L)


def outproj_case(_lib, dev, T, which, label=""):
    """tests/proj_local.py's run_outproj (generation 1 or 2, with the LayerNorm epilogue) / run_dgrad (exact operands) with the (B, D, L) tensors on
    rows whose last one starts just past 2^32 bytes: every offset of them is 64-bit (table row P3), so there is nothing to refuse"""
    B, L, Lx, D = OUTPROJ_SHAPE
    far = cross(B * D, es_of(T))
    if which == "dgrad":
        st = PL.run_dgrad(_lib, dev, T, B, L, Lx, D, True, seed=81, label=label + " limits lda=%d" % far, path="far rows", lda=far, rowbuf=FarBuf)
    else:
        st = PL.run_outproj(_lib, dev, T, B, L, Lx, D, int(which[-1]), norm=True, seed=80, label=label + " limits lda=%d" % far, path="far rows", lda=far,
                            rowbuf=FarBuf)
    import gc
    gc.collect()
    free_all()
    print(line(f"{label} outproj {which} {SL.NAME[T]} B={B} L={L} Lx={Lx} D={D} lda={far}", **{k: float(v) for k, v in st.items()}), flush=True)
    return st


# ---- the decode step's convolution: the pitch of k and of the row history (every offset 64-bit: table row D1) ---------------------------------
DECODE_SHAPE = (2, 2, 2, 100, 57)             # B, Bcap, D, Lcap, position: one ragged chunk


def decode_conv_case(_lib, dev, T, form, label=""):
    """tests/decode_local.py's run_conv with k and the row history on rows whose last one starts just past 2^32 bytes"""
    from tests import decode_local as DL
    B, Bcap, D, Lcap, pos = DECODE_SHAPE
    made = []

    def alloc(shape, fill, dtype, dev_, pitch):
        strides = (pitch, 1) if len(shape) == 2 else (shape[1] * pitch, pitch, 1)
        made.append(FarBuf(shape, strides, dtype, dev_, fill))
        return made[-1].view
    kp, rp_ = cross(D, 4), cross(Bcap * D, es_of(T))
    Tn = 3 if form == "block" else 1
    st, _ = DL.run_conv(_lib, dev, T, form, B, Bcap, D, Lcap, [pos, pos - 9] if form == "rows" else pos, Tn=Tn, seed=82,
                        label=label + f" limits ldk={kp} lda={rp_}", kpitch=kp, rpitch=rp_, alloc=alloc)
    assert len(made) == 2 and all(fb.rows.bands_intact() for fb in made), "a poisoned band was touched"
    made.clear()
    import gc
    gc.collect()
    free_all()
    print(line(f"{label} decode_conv {form} {SL.NAME[T]} B={B} D={D} Lcap={Lcap} ldk={kp} lda={rp_}", **{k: float(v) for k, v in st.items()}), flush=True)
    return st
