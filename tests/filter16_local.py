"""Layer-local fp64 references for the 16-bit implicit-filter kernels (csrc/filter16_kernels.h), shared by the emulator tests
(tests/test_filter16_emu.py) and the GPU tests (tests/test_gpu_filter.py).  Plain torch, device-agnostic; not a test file.

An end-to-end comparison of the filter under 16-bit autocast cannot be tight: one flipped 16-bit rounding in front of sin(10 a) moves
everything downstream of that position by percent, so two correct implementations differ at 1e-2.  The amplification disappears when
every layer is predicted from the KERNEL'S OWN previous pre-activation, which the forward saves anyway: given a_(s-1), the next layer
is one small matrix product and one rounding, and a restatement in fp64 with the roundings of filter16_kernels.h:8-16 predicts it
element by element to half a 16-bit ulp plus a derivable fp32 accumulation bound.  With R() = round-to-nearest-even to T (`.to(T)`):

    h_(-1) = R(z_l)       h_(s-1) = R(sin(x)),  x = the FP32 product freq * a_(s-1) (graph and kernel both round it to fp32)
    e_s = R(W_s) h_(s-1) + R(b_s)      s = 0, 1, 2            y = R(W_3) h_2            k_ref = R(y) m,  m = exp(-t_l |delta_d|) + shift

    acc_s = (K + 2) 2^-24 (|R(W_s)| |h_(s-1)| + |R(b_s)|)     K = 64 (16 for s = 0): K + 1 exact products / bias summed in fp32 in ANY order
    amb_s = |R(W_s)| (ulp_T(h_(s-1)) [h_(s-1) ambiguous])     an h is ambiguous when its fp64 sine lies within tau of a rounding boundary
                                                              of T: there the device's sine may land on the other neighbour

    |a_s - e_s| <= 1/2 ulp_T(e_s) + acc_s + amb_s             |k - k_ref| <= (1/2 ulp_T(y) + acc_3 + amb_3) |m| + 2^-20 |k_ref|

The filter condition as written compares two ROUNDED values: where the fp64 y lies within acc_3 + amb_3 of a rounding boundary of T, the
device's fp32 y may lie on the other side of it, R() of the two differs by a whole ulp, and no correct implementation can meet 1/2 ulp
(measured on the emulator: 1 - 2 elements of 1e5 in bf16, ~1e-3 in fp16, each at 1.6 - 2.0 x the bound).  So every element is held to the
same bound round the UNROUNDED y m -- exactly how the pre-activations are held to e_s -- and, wherever y is not within acc_3 + amb_3 of
a boundary, to the condition as written as well (`viol_k`); the count of elements outside the condition as written is reported next to
it (`viol_k_literal`).

(ulp_T of the binade of the largest magnitude the bound allows, so the larger neighbour at a binade edge; subnormal spacing below the
smallest normal.)  The backward takes the saved pre-activations as an input, so `backward_ref` evaluates autograd's graph of
filter16_kernels.h:13-16 in fp64 at the kernel's own a_0, a_1, a_2, with (`roundings=True`) or without the R() on the deltas: the distance
between the two is what ignoring the 16-bit roundings costs, the yardstick the kernel's own distance is held to."""
import ctypes

import torch

TAU = 2.0 ** -20            # half-width of the band round a rounding boundary of T inside which the device's sine may round either way;
                            # >= 4 x the measured error of hy_sincos over |x| <= SINCOS_RANGE (test_hy_sincos_error_is_covered_by_tau)
SINCOS_RANGE = 256.0        # every test input keeps max |freq a| below this (asserted where the forward is checked)
_FMT = {torch.bfloat16: (7, -126), torch.float16: (10, -14)}     # explicit mantissa bits, exponent of the smallest normal
GRADS = ("dw0", "db0", "dw1", "db1", "dw2", "db2", "dw3", "dfreq", "dz")


def R(x, T):
    """x rounded to nearest even in T, as fp64"""
    return x.to(T).to(torch.float64)


def ulp(x, T):
    """spacing of T in the binade of |x| (fp64 in, fp64 out); the subnormal spacing below T's smallest normal"""
    mb, emin = _FMT[T]
    x = x.abs()
    e = torch.frexp(x)[1] - 1                                   # floor(log2 x)
    e = torch.where(x == 0, torch.full_like(e, emin), e).clamp_min(emin)
    return torch.ldexp(torch.ones_like(x), e - mb)


def decode_saved(saved, L, T, dtype=torch.float64):
    """saved (3, 32, P) int32 as hyena_filter16_fwd fills it -- word p of a layer's row block holds feature 2 p in its low half and
    feature 2 p + 1 in its high half -- -> a0, a1, a2 as (64, L) `dtype` (every T value is exact in fp32 and fp64)"""
    assert saved.dtype == torch.int32 and saved.dim() == 3 and saved.shape[:2] == (3, 32) and saved.shape[2] >= L
    P = saved.shape[2]
    halves = saved.contiguous().view(torch.int16).view(3, 32, P, 2).view(T)          # little endian: [..., 0] is the low half
    a = halves.permute(0, 1, 3, 2).reshape(3, 64, P)[:, :, :L].to(dtype)
    return a[0], a[1], a[2]


def module_args(f, L):
    """the arguments HyenaFilter.filter_dl hands the kernels, detached fp32: ([z (L, E), t, w0, b0, w1, b1, w2, b2, w3, freq, deltas], shift, modulate)"""
    z, t = f.pos_emb(L)
    lin = [f.implicit_filter[i] for i in (0, 2, 4, 6)]
    args = [z[0], t.reshape(-1), lin[0].weight, lin[0].bias, lin[1].weight, lin[1].bias, lin[2].weight, lin[2].bias, lin[3].weight,
            f.implicit_filter[1].freq.reshape(-1), f.modulation.deltas.reshape(-1)]
    return [x.detach().to(torch.float32).contiguous() for x in args], float(f.modulation.shift), bool(f.modulate)


def boundary_distance(x, T):
    """distance of |x| (fp64) to the nearest rounding boundary of T: the midpoint between two neighbouring values of T"""
    u = ulp(x, T)
    frac = x.abs() / u
    return (frac - torch.floor(frac) - 0.5).abs() * u


def with_emb_dim(args, E):
    """the same arguments with the first E columns of the embedding only (HyenaFilter itself builds E >= 3; the kernels take E >= 1)"""
    args = list(args)
    args[0], args[2] = args[0][:, :E].contiguous(), args[2][:, :E].contiguous()
    return args


def sine_layer(a, freq, T, tau=TAU):
    """a (64, n) values of T (any float dtype), freq (64,) fp32 -> h = R(sin(x)), cos(x), ulp_T(h) where h is ambiguous else 0, max |x|;
    x = freq * a rounded to fp32 as the graph and the kernel round it, everything after that in fp64"""
    x = (freq.to(torch.float32)[:, None] * a.to(torch.float32)).to(torch.float64)
    s = torch.sin(x)
    ambw = torch.where(boundary_distance(s, T) <= tau, ulp(s.abs() + tau, T), torch.zeros_like(s))
    return R(s, T), torch.cos(x), ambw, x.abs().max()


def _modulation(t, deltas, shift, modulate, D):
    if not modulate:
        return torch.ones(D, t.shape[0], dtype=torch.float64, device=t.device)
    return torch.exp(-t.to(torch.float64)[None, :] * deltas.to(torch.float64).abs()[:, None]) + shift


def forward_stats(k, acts, args, shift, modulate, T, tau=TAU, chunk=1 << 16):
    """k (D, L) fp32 and the decoded pre-activations `acts` = (a0, a1, a2) of one forward call against the stage references above,
    evaluated in fp64 on the tensors' device in position slices.  Returns, reduced to numbers: per stage s = 0..2 the count of elements
    outside the bound (`viol_a`), the largest |a_s - e_s| / bound (`worst_a`), the share of elements with a_s != R(e_s) (`inexact`) and
    the share of ambiguous h_s (`ambiguous`); `viol_k` / `worst_k` for the filter (see the module docstring; `viol_k_literal`: elements outside the condition with k_ref = R(y) m,
    `y_ambiguous`: share of y within acc_3 + amb_3 of a rounding boundary); `max_arg` = max |freq a|."""
    z, t, w0, b0, w1, b1, w2, b2, w3, freq, deltas = args
    L, D = z.shape[0], w3.shape[0]
    assert k.shape == (D, L) and all(a.shape == (64, L) for a in acts)
    Ws = [R(w, T) for w in (w0, w1, w2, w3)]
    bs = [R(b, T) for b in (b0, b1, b2)]
    u24 = 2.0 ** -24
    out = {"viol_a": [0, 0, 0], "worst_a": [0.0, 0.0, 0.0], "inexact": [0, 0, 0], "ambiguous": [0, 0, 0], "viol_k": 0, "worst_k": 0.0,
           "viol_k_literal": 0, "y_ambiguous": 0, "max_arg": 0.0}
    for l0 in range(0, L, chunk):
        l1 = min(L, l0 + chunk)
        h = R(z[l0:l1].t(), T)                                     # (E, n): exact, never ambiguous
        ambw = torch.zeros_like(h)
        for s in range(3):
            a = acts[s][:, l0:l1].to(torch.float64)
            W, b = Ws[s], bs[s][:, None]
            e = W @ h + b
            acc = ((16 if s == 0 else 64) + 2) * u24 * (W.abs() @ h.abs() + b.abs())
            amb = W.abs() @ ambw
            bound = 0.5 * ulp(e.abs() + acc + amb, T) + acc + amb
            diff = (a - e).abs()
            out["viol_a"][s] += int((diff > bound).sum())
            out["worst_a"][s] = max(out["worst_a"][s], float((diff / bound).max()))
            out["inexact"][s] += int((a != R(e, T)).sum())
            h, _, ambw, xmax = sine_layer(a, freq, T, tau)           # from the KERNEL'S a_s
            out["ambiguous"][s] += int((ambw > 0).sum())
            out["max_arg"] = max(out["max_arg"], float(xmax))
        W = Ws[3]
        y = W @ h
        acc = (64 + 2) * u24 * (W.abs() @ h.abs())
        amb = W.abs() @ ambw
        m = _modulation(t[l0:l1], deltas, shift, modulate, D)
        kref = R(y, T) * m
        bound = (0.5 * ulp(y.abs() + acc + amb, T) + acc + amb) * m.abs() + 2.0 ** -20 * kref.abs()
        kk = k[:, l0:l1].to(torch.float64)
        literal = (kk - kref).abs() > bound                        # the condition with k_ref = R(y) m
        unrounded = (kk - y * m).abs() > bound                     # the same bound round y m, as the pre-activations are held to e_s
        y_amb = boundary_distance(y, T) <= acc + amb               # R() of the device's fp32 y may land on the other neighbour: a whole ulp
        out["viol_k_literal"] += int(literal.sum())
        out["viol_k"] += int((unrounded | (literal & ~y_amb)).sum())
        out["y_ambiguous"] += int(y_amb.sum())
        out["worst_k"] = max(out["worst_k"], float(((kk - y * m).abs() / bound.clamp_min(1e-300)).max()))
    for key in ("inexact", "ambiguous"):
        out[key] = [c / (64.0 * L) for c in out[key]]
    out["y_ambiguous"] /= float(D * L)
    return out


def backward_ref(dk, acts, args, shift, modulate, T, roundings=True, need_dz=True, chunk=1 << 16):
    """autograd's backward of the autocast graph (filter16_kernels.h:13-16) in fp64, evaluated at the pre-activations `acts` = (a0, a1, a2):
        d3 = R(dk m)    dh2 = R(R(W3)^T d3)    g2 = dh2 cos(f a2)    dfreq += sum_l g2 a2    d2 = R(g2 f)    ... down to d0,  dz = R(R(W0)^T d0)
        dW_i = sum_l d_i h_(i-1)^T    db_i = sum_l d_i        (h_(-1) = R(z); the sums stay fp64: the kernels keep them in fp32)
    `roundings=False` drops the R() on d3, dh2, d2, dh1, d1, dh0, d0 and dz (the forward quantities R(W), h, R(z) stay as they are).
    -> dict of fp64 tensors dw0 .. dw3, db0 .. db2, dfreq, dz (L, E) or None."""
    z, t, w0, b0, w1, b1, w2, b2, w3, freq, deltas = args
    L, D = z.shape[0], w3.shape[0]
    assert dk.shape == (D, L)
    rnd = (lambda x: R(x, T)) if roundings else (lambda x: x)
    Ws = [R(w, T) for w in (w0, w1, w2, w3)]
    f64 = freq.to(torch.float64)[:, None]
    g = {n: 0.0 for n in GRADS[:-1]}
    dz = []
    for l0 in range(0, L, chunk):
        l1 = min(L, l0 + chunk)
        a = [acts[s][:, l0:l1].to(torch.float64) for s in range(3)]
        hc = [sine_layer(a[s], freq, T)[:2] for s in range(3)]      # (h_s, cos(f a_s))
        hin = [R(z[l0:l1].t(), T), hc[0][0], hc[1][0], hc[2][0]]   # the input of layer i
        d = rnd(dk[:, l0:l1].to(torch.float64) * _modulation(t[l0:l1], deltas, shift, modulate, D))
        for i in (3, 2, 1):
            g[f"dw{i}"] = g[f"dw{i}"] + d @ hin[i].t()
            if i < 3:
                g[f"db{i}"] = g[f"db{i}"] + d.sum(1)
            gi = rnd(Ws[i].t() @ d) * hc[i - 1][1]
            g["dfreq"] = g["dfreq"] + (gi * a[i - 1]).sum(1)
            d = rnd(gi * f64)
        g["dw0"] = g["dw0"] + d @ hin[0].t()
        g["db0"] = g["db0"] + d.sum(1)
        if need_dz:
            dz.append(rnd(Ws[0].t() @ d).t())
    g["dz"] = torch.cat(dz, 0) if need_dz else None
    return g


def rel(a, b):
    a, b = a.to(torch.float64), b.to(torch.float64)
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()


def backward_stats(got, dk, acts, args, shift, modulate, T, need_dz=True, chunk=1 << 16):
    """got: the kernel's (dw0, db0, dw1, db1, dw2, db2, dw3, dfreq, dz) -> {name: (E_g, N_g)}: E_g = rel-L2(kernel, G_R), N_g = rel-L2(G_noR, G_R)"""
    gr = backward_ref(dk, acts, args, shift, modulate, T, True, need_dz, chunk)
    gn = backward_ref(dk, acts, args, shift, modulate, T, False, need_dz, chunk)
    out = {}
    for name, x in zip(GRADS, got):
        if name == "dz" and not need_dz:
            assert x is None
            continue
        assert x is not None and x.shape == gr[name].shape, name
        out[name] = (rel(x.to(gr[name].device), gr[name]), rel(gn[name], gr[name]))
    return out


def filter16_fwd_into(_lib, k_buf, saved_buf, args, shift, modulate, T):
    """hyena_filter16_fwd_ld on CALLER-owned buffers (test only: _lib.filter_fwd allocates its own): k_buf (D, P) fp32 -- the filter goes
    to k_buf[:, :L] -- and saved_buf (3, 32, P) int32 or None, P = hyena_filter_row_pitch(L).  What lies in the columns L .. P - 1 of
    either buffer is the caller's to inspect afterwards."""
    p = _lib._filter_params(*args, shift, modulate)
    P = int(_lib.lib().hyena_filter_row_pitch(p.L))
    assert k_buf.shape == (p.D, P) and k_buf.dtype == torch.float32 and k_buf.is_contiguous()
    assert saved_buf is None or (saved_buf.shape == (3, 32, P) and saved_buf.dtype == torch.int32 and saved_buf.is_contiguous())
    dev = args[0].device
    with _lib._backend.guard(dev):
        _lib.check(_lib.lib().hyena_filter16_fwd_ld(ctypes.byref(p), _lib.dtype_code(T), k_buf.data_ptr(), P,
                                                    None if saved_buf is None else saved_buf.data_ptr(), _lib._backend.stream(dev)))
    return k_buf[:, :p.L]


K_SENTINEL = -7.25e7                  # what the pad columns L .. P - 1 of k and of `saved` hold before the call -- and must hold after it
S_SENTINEL = 0x5EA15EA1


def check_local(_lib, args, shift, modulate, T, dk, need_dz=True, chunk=1 << 16, compact=False, label=""):
    """Every forward and backward condition of this module on one input, through the C ABI of whatever backend `_lib` is routed to
    (the CPU emulation or the gfx950 library): asserts them, prints the figures first, and returns them with the call's k and gradients.  `compact`: keep the decoded
    pre-activations in T instead of fp64 (the long lengths)."""
    z, w3 = args[0], args[8]
    L, D, dev = z.shape[0], w3.shape[0], z.device
    P = int(_lib.lib().hyena_filter_row_pitch(L))
    # ---- forward: pad columns, SAVE template, the production wrapper
    k_buf = torch.full((D, P), K_SENTINEL, dtype=torch.float32, device=dev)
    saved = torch.full((3, 32, P), S_SENTINEL, dtype=torch.int32, device=dev)
    k = filter16_fwd_into(_lib, k_buf, saved, args, shift, modulate, T)
    k_plain = filter16_fwd_into(_lib, torch.full_like(k_buf, K_SENTINEL), None, args, shift, modulate, T)
    k_prod, saved_prod = _lib.filter_fwd(*args, shift, modulate, save=True, compute_dtype=T)
    pads_ok = bool((k_buf[:, L:] == K_SENTINEL).all()) and bool((saved[:, :, L:] == S_SENTINEL).all())
    same_k = torch.equal(k, k_plain) and torch.equal(k, k_prod) and torch.equal(saved[:, :, :L], saved_prod[:, :, :L])
    finite = bool(torch.isfinite(k).all())
    acts = decode_saved(saved, L, T, dtype=T if compact else torch.float64)
    fwd = forward_stats(k, acts, args, shift, modulate, T, chunk=chunk)
    print(f"[filter16-local] {label} fwd pads_ok={pads_ok} same_k={same_k} " + " ".join(
        f"{n}={[float(f'{v:.3g}') for v in fwd[n]] if isinstance(fwd[n], list) else float(f'{fwd[n]:.3g}')}" for n in sorted(fwd)), flush=True)
    # ---- backward on the forward's own `saved`
    g1 = _lib.filter_bwd(dk, saved, *args, shift, modulate, need_dz, compute_dtype=T)
    g2 = _lib.filter_bwd(dk, saved, *args, shift, modulate, need_dz, compute_dtype=T)
    deterministic = all((a is None and b is None) or torch.equal(a, b) for a, b in zip(g1, g2))
    bwd = backward_stats(g1, dk, acts, args, shift, modulate, T, need_dz=need_dz, chunk=chunk)
    print(f"[filter16-local] {label} bwd deterministic={deterministic} " +
          " ".join(f"{n}:E={e:.3g},N={nn:.3g}" for n, (e, nn) in bwd.items()), flush=True)
    assert pads_ok, "columns L .. P - 1 of k / saved were written"
    assert same_k, "save=False, save=True and _lib.filter_fwd do not give the same bits"
    assert finite
    assert fwd["max_arg"] <= SINCOS_RANGE, fwd["max_arg"]                     # the range hy_sincos' error was measured over
    cap = 1e-2 if T == torch.bfloat16 else 2e-2
    assert all(s <= cap for s in fwd["ambiguous"]), fwd["ambiguous"]          # condition on the input
    assert fwd["viol_a"] == [0, 0, 0], (fwd["viol_a"], fwd["worst_a"])
    assert fwd["viol_k"] == 0, (fwd["viol_k"], fwd["worst_k"])
    assert all(s < 1e-2 for s in fwd["inexact"]), fwd["inexact"]              # condition on the input
    assert deterministic
    assert (g1[-1] is not None) == need_dz
    for n, (e, nn) in bwd.items():
        assert e < nn / 4, (n, e, nn)
    return {"fwd": fwd, "bwd": bwd, "k": k, "grads": g1}


def check_module_path(f, L, T, dk, res):
    """HyenaFilter.filter_dl under autocast of T -- with and without grad mode -- against the direct calls of check_local (`res`): same bits for
    the filter and for every gradient the module's parameters receive; a buffer z receives none"""
    dev = dk.device.type
    f.zero_grad(set_to_none=True)
    with torch.autocast(dev, dtype=T):
        with torch.no_grad():
            k0 = f.filter_dl(L)
        k = f.filter_dl(L)
    assert torch.equal(k0, res["k"]) and torch.equal(k.detach(), res["k"])
    k.backward(dk)
    lin = [f.implicit_filter[i] for i in (0, 2, 4, 6)]
    dw0, db0, dw1, db1, dw2, db2, dw3, dfreq, dz = res["grads"]
    for got, want in ((lin[0].weight.grad, dw0), (lin[0].bias.grad, db0), (lin[1].weight.grad, dw1), (lin[1].bias.grad, db1),
                      (lin[2].weight.grad, dw2), (lin[2].bias.grad, db2), (lin[3].weight.grad, dw3), (f.implicit_filter[1].freq.grad.reshape(-1), dfreq)):
        assert torch.equal(got, want)
    z = f.pos_emb.z
    if dz is None:
        assert not (isinstance(z, torch.nn.Parameter) and z.requires_grad)
    else:
        assert torch.equal(z.grad[0, :L], dz) and not bool(z.grad[0, L:].any())
