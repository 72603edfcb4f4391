"""Layer-local element-wise fp64 references for the fp32 implicit-filter kernels (csrc/filter_kernels.h), shared by the emulator tests
(tests/test_filter_local_emu.py) and the GPU tests (tests/test_gpu_filter_local.py).  Plain torch, device-agnostic; not a test file.
The 16-bit twin is tests/filter16_local.py; derivations, depth counts and measured figures are in profiles/filter_local.md.

The forward saves its pre-activations, so every layer is predicted from the KERNEL'S OWN previous one: the sin(10 a) amplification is gone
and what is left follows from fp32 arithmetic.  u = 2^-24, x = fl32(freq a_(s-1)) as the kernel forms it, h_(s-1) = sin(x) in fp64:

    e_0 = W0 z + b0                   |a_0 - e_0| <= (E + 2) u (|W0||z| + |b0|)
    e_s = W_s h_(s-1) + b_s, s = 1, 2 |a_s - e_s| <= 66 u (|W_s||h| + |b_s|) + sigma |W_s| 1
    y   = W3 h_2                      |y' - y|    <= 66 u |W3||h_2| + sigma |W3| 1
    k_ref = y m,  m = exp(-t|delta|) + shift
    |k - k_ref| <= |y' - y| |m| + |y| (|m - shift| (eps_m + 2 u |t delta|) + u |m|) + u |k_ref|

(K + 2) u covers K exact products and a bias summed in fp32 in ANY order.  sigma = 2 x the measured largest absolute error of hy_sincos over
|x| <= SINCOS_RANGE; eps_m = 2 x the measured relative error of the kernels' exp2 beyond the rounding of its argument (`modulation_probe`),
at least 2^-23.

The backward is linear in dk at fixed saved pre-activations: `backward_ref` evaluates the graph in fp64 at the kernel's a_0, a_1, a_2 with cos(x)
in fp64, and next to it the same graph on magnitudes, which carries the error recursion

    E(delta_3)     = |dk| (|m - shift| (eps_m + 2 u |t delta|) + u |m|) + u |delta_3|
    E(delta_(s-1)) = [ |W_s|^T E(delta_s) + (NO + 2) u |W_s|^T |delta_s| ] |f||cos x| + |W_s^T delta_s| |f| sigma + 3 u |delta_(s-1)|
    E(dW_s) = sum_l [ E(delta_s) |h| + |delta_s| sigma ] + n_W u sum_l |delta_s||h|          (db, dfreq, dz likewise)

n_W, n_b, n_f: the depths of the sums as the code performs them (`depths`), never L."""
import ctypes
import time

import torch

from tests.filter16_local import SINCOS_RANGE, _modulation, module_args, with_emb_dim  # noqa: F401  (re-exported for the test files)

U = 2.0 ** -24
SIGMA_MEASURED = 9.24e-8          # hy_sincos over |x| <= SINCOS_RANGE on the CPU build (hipemu_probe_sincos; re-measured by the emulator tests)
SIGMA = 2 * SIGMA_MEASURED
EPS_M_FLOOR = 2.0 ** -23
EPS_M_CAP = 4 * U                 # relative error of an exp2 that is 2 ulp off at the bottom of a binade: the most the probe may report
POISON_BITS = 0x7FC0BEEF          # a quiet NaN with a payload: what every pad, scratch and output buffer holds before a call
GRADS = ("dw0", "db0", "dw1", "db1", "dw2", "db2", "dw3", "dfreq", "dz")

# csrc/filter_kernels.h: FLT_WAVES, FLT_TP, FLT_WG_POS, FLT_MAX_WG, FLT_RED_S and FltBwdCfg<NO, NI>::KS
WAVES, TP, WG_POS, MAX_WG, RED_S = 8, 32, 256, 256, 16


def KS(NO, NI):
    nib = (NI + 31) // 32
    blocks = (NO // 32) * nib
    bpw = blocks // WAVES if blocks >= WAVES else 1
    return WAVES // (blocks // bpw)


def grid_of(L):
    return min((L + WG_POS - 1) // WG_POS, MAX_WG)


def reduction_counts(D, L):
    """`count` of every reduction of one backward call (launch_filter_layer_bwd): partial rows summed per output"""
    g = grid_of(L)
    k3, k, k0 = KS(D, 64), KS(64, 64), KS(64, 8)
    return {"dw3": g * k3, "dw2": g * k, "dw1": g * k, "dw0": g * k0, "db2": 2 * g * k, "db1": 2 * g * k, "db0": 2 * g * k0, "dfreq": WAVES * g}


def reduce_loops(count):
    """which loops of the reduction kernels run for `count` partial rows: (thread rows that enter the unrolled loop, its largest trip
    count, thread rows that enter the tail loop)"""
    rows_unrolled = trips = rows_tail = 0
    for cs in range(RED_S):
        c, n = cs, 0
        while c + 7 * RED_S < count:
            c, n = c + 8 * RED_S, n + 1
        rows_unrolled += n > 0
        trips = max(trips, n)
        rows_tail += c < count
    return rows_unrolled, trips, rows_tail


def depths(D, L):
    """depth (number of fp32 additions behind one output) of every sum over positions, recounted from filter_layer_bwd_kernel and the
    reduce kernels; profiles/filter_local.md gives the lines"""
    g = grid_of(L)
    iters = -(-((L + WG_POS - 1) // WG_POS) // g)               # workgroup iterations of the busiest workgroup
    cnt = reduction_counts(D, L)
    red = lambda c: -(-c // RED_S) + RED_S                      # a thread row's share of the partial rows, then the 16 thread rows
    d = {}
    for name, no, ni in (("dw3", D, 64), ("dw2", 64, 64), ("dw1", 64, 64), ("dw0", 64, 8)):
        pt_per = WAVES // KS(no, ni)
        d[name] = 32 * pt_per * iters + red(cnt[name])          # 16 MFMAs of k = 2 per tile, pt_per tiles per iteration
        if name != "dw3":
            d["db" + name[2]] = 16 * pt_per * iters + red(cnt["db" + name[2]])    # 16 adds per tile into accb, the two half-wave slots are partial rows
    d["dfreq"] = iters + TP + red(cnt["dfreq"]) + 3             # accf per iteration, the 32-lane sum, the reduction, one add per accumulating launch
    return d


def poison(shape, device, dtype=torch.float32):
    return torch.full(shape, POISON_BITS, dtype=torch.int32, device=device).view(dtype)


def is_poison(x):
    return bool((x.contiguous().view(torch.int32) == POISON_BITS).all())


def make_case(D, L, E, seed, shift=0.0, z_stride=None, device="cpu"):
    """kernel arguments as tests/test_filter_emu.py::_make_filter builds them (random weights, biases N(0, 0.3)), the first E columns of a wider
    embedding where HyenaFilter cannot build E itself, deltas of BOTH signs; z_stride > E: z is columns [:E] of an (L, z_stride) tensor of NaN"""
    from tests.test_filter_emu import _make_filter
    f = _make_filter(D, L, emb_dim=max(3, E | 1), seed=seed, shift=shift)
    args, sh, modulate = module_args(f, L)
    args = with_emb_dim(args, E)
    sign = torch.where(torch.arange(D) % 3 == 1, 1.0, -1.0)                 # the module's deltas are all negative
    args[10] = (args[10].abs() * sign).contiguous()
    args = [a.to(device) for a in args]
    if z_stride is not None:
        wide = poison((L, z_stride), device)
        wide[:, :E] = args[0]
        args[0] = wide[:, :E]
    assert sh == shift and modulate
    return args


def _params(_lib, args, shift, modulate):
    z = args[0]
    assert z.dim() == 2 and (z.shape[1] == 1 or z.stride(1) == 1)
    p = _lib.FilterParams()
    for name, ten in zip(("z", "t", "w0", "b0", "w1", "b1", "w2", "b2", "w3", "freq", "deltas"), args):
        _lib._require_gpu(ten, name)
        assert ten.dtype == torch.float32 and (name == "z" or ten.is_contiguous()), name
        setattr(p, name, ten.data_ptr())
    zs = z.shape[1] if z.is_contiguous() else z.stride(0)
    p.shift, p.modulate, p.z_stride, p.L, p.E, p.D = float(shift), int(bool(modulate)), zs, z.shape[0], z.shape[1], args[8].shape[0]
    return p


def filter_fwd_into(_lib, k_buf, saved, args, shift, modulate):
    """hyena_filter_fwd_ld on CALLER-owned buffers: k_buf (D, ldk) fp32 with ldk >= L -- the filter goes to k_buf[:, :L] -- and saved
    (3, 64, P) fp32 or None, P = hyena_filter_row_pitch(L)"""
    p = _params(_lib, args, shift, modulate)
    P = int(_lib.lib().hyena_filter_row_pitch(p.L))
    assert k_buf.dim() == 2 and k_buf.shape[0] == p.D and k_buf.shape[1] >= p.L and k_buf.dtype == torch.float32 and k_buf.is_contiguous()
    assert saved is None or (saved.shape == (3, 64, P) and saved.dtype == torch.float32 and saved.is_contiguous())
    dev = args[1].device
    with _lib._backend.guard(dev):
        _lib.check(_lib.lib().hyena_filter_fwd_ld(ctypes.byref(p), k_buf.data_ptr(), k_buf.shape[1], None if saved is None else saved.data_ptr(),
                                                  _lib._backend.stream(dev)))
    return k_buf[:, :p.L]


def filter_bwd_into(_lib, dk_buf, saved, args, shift, modulate, need_dz=True):
    """hyena_filter_bwd_ld on caller-owned buffers, every one of them poisoned first: dk_buf (D, ldk) with the gradient in [:, :L] -> (grads
    dict, dz as (E, L) or None, workspace as (floats,)); the first two (64, P) blocks of the workspace hold delta_0 and delta_1 afterwards"""
    p = _params(_lib, args, shift, modulate)
    P = int(_lib.lib().hyena_filter_row_pitch(p.L))
    assert dk_buf.dim() == 2 and dk_buf.shape[0] == p.D and dk_buf.shape[1] >= p.L and dk_buf.dtype == torch.float32 and dk_buf.is_contiguous()
    assert saved.shape == (3, 64, P) and saved.dtype == torch.float32 and saved.is_contiguous()
    dev = args[1].device
    outs = {n: poison(tuple(args[i].shape), dev) for n, i in (("dw0", 2), ("db0", 3), ("dw1", 4), ("db1", 5), ("dw2", 6), ("db2", 7), ("dw3", 8), ("dfreq", 9))}
    outs["dz"] = poison((p.E, p.L), dev) if need_dz else None
    g = _lib.FilterGrads()
    for n, ten in outs.items():
        setattr(g, n, None if ten is None else ten.data_ptr())
    nbytes = int(_lib.lib().hyena_filter_workspace_bytes(p.L, p.D))
    assert nbytes % 4 == 0 and nbytes >= 2 * 64 * P * 4
    ws = poison((nbytes // 4,), dev)
    with _lib._backend.guard(dev):
        _lib.check(_lib.lib().hyena_filter_bwd_ld(ctypes.byref(p), dk_buf.data_ptr(), dk_buf.shape[1], saved.data_ptr(), ctypes.byref(g), ws.data_ptr(),
                                                  nbytes, _lib._backend.stream(dev)))
    return outs, ws


# ---- the modulation probe ------------------------------------------------------------------------------------------------------------
_EPS_M = {}


def modulation_probe(_lib, device, L=2048, D=256):
    """Relative error of the kernels' modulation, measured through the ABI.  W2 = 0, W3 = ones in column 0, freq[0] b2[0] ~ pi/2: y is the same
    constant y0 at every (d, l); one call with modulate = 0 returns y0, one with modulate = 1 (shift 0) returns k = fl(y0 m'), so m' = k / y0 to
    one rounding.  t = linspace(0, 1, L) as the module builds it, |delta| log-spaced over the module's range x [0.1, 10], signs alternating.
    -> (eps, info): eps = max over samples with exp(-t|delta|) >= 2^-120 of |m' - m| / m - 2 u |t delta| - u (argument rounding, the rounding of k)."""
    import math
    g = torch.Generator().manual_seed(0)
    z = torch.randn(L, 5, generator=g)
    t = torch.linspace(0, 1, L)
    w = lambda *s: torch.randn(*s, generator=g) * 0.1
    w0, b0, w1, b1, w2, b2 = w(64, 5), w(64), w(64, 64), w(64), torch.zeros(64, 64), torch.zeros(64)
    freq = torch.full((64,), 10.0)
    b2[0] = math.pi / 20
    w3 = torch.zeros(D, 64)
    w3[:, 0] = 1.0
    lo, hi = abs(math.log(1e-2) / 1.5), abs(math.log(1e-2) / 0.3)                  # ExponentialModulation's range of |deltas|
    mag = torch.logspace(math.log10(0.1 * lo), math.log10(10 * hi), D, dtype=torch.float64).float()
    deltas = mag * torch.where(torch.arange(D) % 2 == 0, -1.0, 1.0)
    args = [x.to(device).contiguous() for x in (z, t, w0, b0, w1, b1, w2, b2, w3, freq, deltas)]
    y0 = filter_fwd_into(_lib, poison((D, L), device), None, args, 0.0, False).double()
    k = filter_fwd_into(_lib, poison((D, L), device), None, args, 0.0, True).double()
    assert bool((y0 == y0[0, 0]).all()) and 0.99 < float(y0[0, 0]) <= 1.0, "the probe's y is not one constant"
    td = args[1].double()[None, :] * args[10].double().abs()[:, None]
    m = torch.exp(-td)
    ok = m >= 2.0 ** -120
    raw = ((k / y0 - m).abs() / m)
    eps = (raw - 2 * U * td - U)[ok].clamp_min(0).max().item()
    info = {"samples": int(ok.sum()), "raw_max": raw[ok].max().item(), "max_t_delta": td[ok].max().item(), "y0": float(y0[0, 0])}
    return eps, info


def eps_m_for(_lib, device):
    """the eps_m the bounds use on this backend: 2 x the probe's figure, at least 2^-23 (measured once per backend and process) -- and never
    more than 2 x what a 2 ulp exp2 explains (EPS_M_CAP): the figure comes from the code under test, and a broken modulation must fail the
    cases' bounds, not widen them"""
    key = (_lib._backend.name, str(device))
    if key not in _EPS_M:
        eps, info = modulation_probe(_lib, device)
        print(f"[filter-local] modulation probe on {key[0]}: eps_m measured {eps:.3g} = {eps / U:.2f} u ({info})", flush=True)
        _EPS_M[key] = (eps, min(max(2 * eps, EPS_M_FLOOR), 2 * EPS_M_CAP))
    return _EPS_M[key][1]


# ---- references ------------------------------------------------------------------------------------------------------------------------
def _sincos64(a, freq):
    """a (64, n) fp32, freq (64,) fp32 -> x = fl32(freq a) as fp64, sin x, cos x"""
    x = (freq[:, None] * a).to(torch.float64)
    return x, torch.sin(x), torch.cos(x)


def _mod_terms(t, deltas, shift, modulate, D, eps_m):
    """m (D, n) and the bound on |m' - m| of the kernels' m' = fl(exp2'(fl(-t fl(|delta| log2 e))) + shift)"""
    m = _modulation(t, deltas, shift, modulate, D)
    if not modulate:
        return m, torch.zeros_like(m)
    td = t.to(torch.float64)[None, :] * deltas.to(torch.float64).abs()[:, None]
    return m, (m - shift).abs() * (eps_m + 2 * U * td) + U * m.abs()


class _Worst:
    """largest |err| / bound per name, and the share of elements beyond half their bound"""

    def __init__(self):
        self.worst, self.near, self.n = {}, {}, {}

    def add(self, name, got, ref, bound):
        err = (got.to(torch.float64) - ref).abs()
        assert bool(torch.isfinite(err).all()), f"{name}: not finite"
        ratio = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300))
        self.worst[name] = max(self.worst.get(name, 0.0), float(ratio.max()))
        self.near[name] = self.near.get(name, 0) + int((ratio > 0.5).sum())
        self.n[name] = self.n.get(name, 0) + ratio.numel()

    def line(self):
        return " ".join(f"{k}={v:.3g}" for k, v in self.worst.items())

    def near_share(self):
        return sum(self.near.values()) / max(1, sum(self.n.values()))


def forward_check(k, acts, args, shift, modulate, eps_m, chunk=1 << 14):
    """k (D, L) and the saved pre-activations acts = (a0, a1, a2), each (64, L) fp32, of one forward call against the stage references of the
    module docstring -> (_Worst over a0, a1, a2, k; max |freq a|)"""
    z, t, w0, b0, w1, b1, w2, b2, w3, freq, deltas = args
    L, E, D = z.shape[0], z.shape[1], w3.shape[0]
    W = [w.to(torch.float64) for w in (w0, w1, w2, w3)]
    b = [x.to(torch.float64)[:, None] for x in (b0, b1, b2)]
    out, max_arg = _Worst(), 0.0
    for l0 in range(0, L, chunk):
        l1 = min(L, l0 + chunk)
        h = z[l0:l1].to(torch.float64).t()
        for s in range(3):
            e = W[s] @ h + b[s]
            bound = ((E if s == 0 else 64) + 2) * U * (W[s].abs() @ h.abs() + b[s].abs())
            if s > 0:
                bound = bound + SIGMA * W[s].abs().sum(1, keepdim=True)
            a = acts[s][:, l0:l1]
            out.add(f"a{s}", a, e, bound)
            x, h, _ = _sincos64(a, freq)
            max_arg = max(max_arg, float(x.abs().max()))
        y = W[3] @ h
        ey = 66 * U * (W[3].abs() @ h.abs()) + SIGMA * W[3].abs().sum(1, keepdim=True)
        m, em = _mod_terms(t[l0:l1], deltas, shift, modulate, D, eps_m)
        kref = y * m
        out.add("k", k[:, l0:l1], kref, ey * m.abs() + y.abs() * em + U * kref.abs())
    return out, max_arg


def backward_ref(dk, acts, args, shift, modulate, eps_m=EPS_M_FLOOR, need_dz=True, chunk=1 << 14, on_delta=None):
    """The backward of the five lines of the module docstring in fp64 at the pre-activations `acts`, and the same graph on magnitudes.
    -> (grads, bounds): dicts of fp64 tensors dw0 .. dw3, db0 .. db2, dfreq, dz (L, E) or None; `bounds` holds E(.) of the module docstring with
    the depths of `depths`.  on_delta(s, l0, l1, delta_s, E(delta_s)) is called per position slice for s = 1, 0 (the caller compares its own rows:
    nothing of size (64, L) is kept in fp64)."""
    z, t, w0, b0, w1, b1, w2, b2, w3, freq, deltas = args
    L, D = z.shape[0], w3.shape[0]
    assert dk.shape == (D, L)
    W = [w.to(torch.float64) for w in (w0, w1, w2, w3)]
    f64 = freq.to(torch.float64)[:, None]
    nd = depths(D, L)
    g = {n: 0.0 for n in GRADS[:-1]}
    Eg = {n: 0.0 for n in GRADS[:-1]}          # propagated error
    Mg = {n: 0.0 for n in GRADS[:-1]}          # sum of the magnitudes of the terms (x depth x u: the summation's own error)
    dz, Edz = [], []
    for l0 in range(0, L, chunk):
        l1 = min(L, l0 + chunk)
        a = [acts[s][:, l0:l1] for s in range(3)]
        sc = [_sincos64(a[s], freq) for s in range(3)]
        hin = [z[l0:l1].to(torch.float64).t(), sc[0][1], sc[1][1], sc[2][1]]
        m, em = _mod_terms(t[l0:l1], deltas, shift, modulate, D, eps_m)
        dk64 = dk[:, l0:l1].to(torch.float64)
        d = dk64 * m
        Ed = dk64.abs() * em + (U * d.abs() if modulate else 0.0)
        for s in (3, 2, 1):
            no = D if s == 3 else 64
            g[f"dw{s}"] = g[f"dw{s}"] + d @ hin[s].t()
            Eg[f"dw{s}"] = Eg[f"dw{s}"] + Ed @ hin[s].abs().t() + SIGMA * d.abs().sum(1, keepdim=True)
            Mg[f"dw{s}"] = Mg[f"dw{s}"] + d.abs() @ hin[s].abs().t()
            if s < 3:
                g[f"db{s}"], Eg[f"db{s}"], Mg[f"db{s}"] = g[f"db{s}"] + d.sum(1), Eg[f"db{s}"] + Ed.sum(1), Mg[f"db{s}"] + d.abs().sum(1)
            x, _, c = sc[s - 1]
            dh = W[s].t() @ d
            Edh = W[s].abs().t() @ Ed + (no + 2) * U * (W[s].abs().t() @ d.abs())
            gi = dh * c
            term = gi * a[s - 1].to(torch.float64)
            g["dfreq"] = g["dfreq"] + term.sum(1)
            Eg["dfreq"] = Eg["dfreq"] + ((Edh * c.abs() + dh.abs() * SIGMA) * a[s - 1].to(torch.float64).abs() + 2 * U * term.abs()).sum(1)
            Mg["dfreq"] = Mg["dfreq"] + term.abs().sum(1)
            d = gi * f64
            Ed = Edh * (f64.abs() * c.abs()) + dh.abs() * f64.abs() * SIGMA + 3 * U * d.abs()
            if on_delta is not None:
                on_delta(s - 1, l0, l1, d, Ed)
        g["dw0"], Eg["dw0"], Mg["dw0"] = g["dw0"] + d @ hin[0].t(), Eg["dw0"] + Ed @ hin[0].abs().t(), Mg["dw0"] + d.abs() @ hin[0].abs().t()
        g["db0"], Eg["db0"], Mg["db0"] = g["db0"] + d.sum(1), Eg["db0"] + Ed.sum(1), Mg["db0"] + d.abs().sum(1)
        if need_dz:
            dz.append((W[0].t() @ d).t())
            Edz.append((W[0].abs().t() @ Ed + 66 * U * (W[0].abs().t() @ d.abs())).t())
    bounds = {n: Eg[n] + nd[n] * U * Mg[n] for n in GRADS[:-1]}
    g["dz"], bounds["dz"] = (torch.cat(dz, 0), torch.cat(Edz, 0)) if need_dz else (None, None)
    return g, bounds


def backward_check(outs, ws, dk, acts, args, shift, modulate, eps_m, need_dz=True, chunk=1 << 14):
    """the gradients `outs` and the workspace `ws` of filter_bwd_into against backward_ref: every element of delta_1, delta_0, dz, dw0 .. dw3,
    db0 .. db2 and dfreq against its own bound -> _Worst"""
    L = args[0].shape[0]
    P = ws_pitch(L)
    blocks = ws[:2 * 64 * P].view(2, 64, P)                        # dA = delta_0 (written last), dB = delta_1
    out = _Worst()

    def on_delta(s, l0, l1, d, Ed):
        if s <= 1:                                                 # delta_2 lived in dA until delta_0 replaced it
            out.add(f"delta{s}", blocks[s][:, l0:l1], d, Ed)
    g, bounds = backward_ref(dk, acts, args, shift, modulate, eps_m, need_dz, chunk, on_delta)
    for n in GRADS:
        if n == "dz":
            if need_dz:
                out.add(n, outs[n].t(), g[n], bounds[n])
            else:
                assert outs[n] is None
        else:
            out.add(n, outs[n], g[n].reshape(outs[n].shape), bounds[n].reshape(outs[n].shape))
    return out


def ws_pitch(L):
    return (L + 63) & ~63


def check_local(_lib, args, shift, modulate, dk, ldk=None, need_dz=True, chunk=1 << 14, label=""):
    """Every forward, backward and structural condition of this module on one input, through the C ABI of whatever backend `_lib` is routed
    to; prints the figures before it asserts and returns them.  ldk: row pitch of k and dk (default: packed, ldk = L)."""
    t0 = time.time()
    z, w3 = args[0], args[8]
    L, E, D, dev = z.shape[0], z.shape[1], w3.shape[0], args[1].device
    ldk = L if ldk is None else ldk
    P = int(_lib.lib().hyena_filter_row_pitch(L))
    assert P == ws_pitch(L)
    eps_m = eps_m_for(_lib, dev)
    # ---- forward
    k_buf, saved = poison((D, ldk), dev), poison((3, 64, P), dev)
    k = filter_fwd_into(_lib, k_buf, saved, args, shift, modulate)
    k_plain = filter_fwd_into(_lib, poison((D, ldk), dev), None, args, shift, modulate)
    cargs = [args[0].contiguous()] + list(args[1:])
    k_prod = _lib.filter_fwd(*cargs, shift, modulate, save=False)
    fwd_pads = is_poison(k_buf[:, L:]) and is_poison(saved[:, :, L:])
    same_k = torch.equal(k, k_plain) and torch.equal(k, k_prod)
    acts = [saved[s][:, :L] for s in range(3)]
    fwd_finite = bool(torch.isfinite(k).all()) and all(bool(torch.isfinite(a).all()) for a in acts)
    print(f"[filter-local] {label} D={D} L={L} E={E} ldk={ldk} zs={_params(_lib, args, shift, modulate).z_stride} modulate={int(modulate)} shift={shift} "
          f"dz={int(need_dz)}: fwd pads_ok={fwd_pads} same_k={same_k} finite={fwd_finite}", flush=True)
    assert fwd_finite, "a pad's NaN reached the forward's output"
    fw, max_arg = forward_check(k, acts, args, shift, modulate, eps_m, chunk)
    # ---- backward on the forward's own `saved`
    dk_buf = poison((D, ldk), dev)
    dk_buf[:, :L] = dk
    outs, ws = filter_bwd_into(_lib, dk_buf, saved, args, shift, modulate, need_dz)
    outs2, ws2 = filter_bwd_into(_lib, dk_buf, saved, args, shift, modulate, need_dz)
    names = [n for n in GRADS if outs[n] is not None]
    deterministic = all(torch.equal(outs[n], outs2[n]) for n in names) and torch.equal(ws[:128 * P].view(128, P)[:, :L], ws2[:128 * P].view(128, P)[:, :L])
    if need_dz:                                                     # the same call without dz: every other gradient keeps its bits
        outs3, _ = filter_bwd_into(_lib, dk_buf, saved, args, shift, modulate, False)
        same_without_dz = all(torch.equal(outs[n], outs3[n]) for n in names if n != "dz")
    else:
        same_without_dz = True
    bwd_pads = is_poison(ws[:128 * P].view(128, P)[:, L:]) and is_poison(saved[:, :, L:]) and is_poison(dk_buf[:, L:])
    bwd_finite = all(bool(torch.isfinite(outs[n]).all()) for n in names) and bool(torch.isfinite(ws[:128 * P].view(128, P)[:, :L]).all())
    print(f"[filter-local] {label} bwd pads_ok={bwd_pads} deterministic={deterministic} same_without_dz={same_without_dz} finite={bwd_finite}", flush=True)
    assert bwd_finite, "a pad's NaN, or what an output buffer held before the call, reached a gradient"
    bw = backward_check(outs, ws, dk, acts, args, shift, modulate, eps_m, need_dz, chunk)
    dt = time.time() - t0
    print(f"[filter-local] {label} max|f a|={max_arg:.3g} worst fwd: {fw.line()} | bwd: {bw.line()} | within 2x of bound: fwd {fw.near_share():.3g} "
          f"bwd {bw.near_share():.3g} | {dt:.2f} s", flush=True)
    assert fwd_pads, "columns [L, ldk) of k or [L, P) of saved were written"
    assert same_k, "SAVE = true, SAVE = false and _lib.filter_fwd do not give the same bits"
    assert max_arg <= SINCOS_RANGE, max_arg
    assert bwd_pads, "columns [L, P) of dA / dB / saved or [L, ldk) of dk were written"
    assert deterministic and same_without_dz
    for name, w in list(fw.worst.items()) + list(bw.worst.items()):
        assert w <= 1.0, (label, name, w)
    return {"fwd": fw, "bwd": bw, "k": k, "grads": outs, "seconds": dt}
