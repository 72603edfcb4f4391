"""What the kernels do with a non-finite value they are meant to read: NaN, inf and fp16 overflow.  Shared by the emulator tests
(tests/test_nonfinite_emu.py) and the GPU tests (tests/test_gpu_nonfinite.py).  Plain torch; not a test file.  Counts, run times, tables and the
seeded defects: profiles/nonfinite_local.md.  (The sampler's non-finite logits: tests/decode_sample_local.py, case_nonfinite.)

B. The 16-bit store conversion.  ``cm_post_fwd`` alone with w = (0, 0, 1), b = 0 and no in_proj bias stores z = cvt(y * x): one rounding of a
   product that is exact in fp32.  y runs over all 65536 bit patterns of the type, x over 16 multipliers; the expected value is
   ``(y.double() * x.double()).to(dtype)``, held bit for bit (any NaN where a NaN is expected; the multiplier -0 reaches the product as +0,
   see suite_cvt_exact).  Then one kernel per remaining store helper with operands scaled until fp16 overflows: inf beyond 65520, never a
   saturated 65504, a zero or a NaN (hold_threshold).
C. Propagation and containment through the 17 autograd Functions (tests/autograd_local.py's REGISTRY, Case and run): a clean run against runs
   that differ from it in ONE element -- NaN or +inf, in ``dout`` (backward plant) or in the activation input (forward plant), inside unit 0:
     C1  forward plant: every output outside unit 0 keeps the clean run's bits
     C2  forward plant: every output has a non-finite element inside unit 0
     C3  backward plant: the activation's gradient outside unit 0 keeps the clean run's bits
     C4  backward plant: every gradient returned has a non-finite element (the activation's inside unit 0), but for DISCONNECTED
   UNITS says what each Function treats independently and where that axis sits in its activation and in each output.
D. The loss scaler end to end: the 2-layer HyenaDNALM of autograd_local.lm_build under fp16 autocast, AdamW and torch.amp.GradScaler."""
import copy

import torch

from tests import autograd_local as AL

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
same_bits = AL.same_bits

# ---- C. units -------------------------------------------------------------------------------------------------------------------------------
# key of autograd_local.REGISTRY -> (what a unit is, the unit's axes in the activation (None: the entry has none), the unit's axes in each output).
# Unit 0 of a tensor: index 0 on every one of those axes.  "batch": Functions that hold a convolution along the sequence (the long one, or
# InProjPreCMFunc's three-tap one) or a pool over it; "row": one position of one sequence; None: no independent units, propagation checks only.
UNITS = {
    "FFTConvFunc": ("batch", (0,), [(0,)]),                                      # u (B, D, L) -> y (B, D, L)
    "HyenaFilterFunc": (None, (), [()]),                                         # z (L, E) -> k (D, L): every tap of every channel reads all of z's row ...
    "InProjCMFunc": ("row", (0, 1), [(1, 2)]),                                   # u (B, L, D) -> xT (G D, B, L)
    "InProjPreCMFunc": ("batch", (0,), [(1,), (0,)]),                            # u (B, L, D) -> xT (3 D, B, L), vg (B, D, L): the short filter runs along L
    "OutProjCMFunc": ("row", (1, 2), [(0, 1)]),                                  # zT (D, B, L) -> (B, L, D)
    "SplitKLinearFunc": ("row", (0,), [(0,)]),                                   # x (rows, D) -> (rows, N)
    "SmallVocabEmbeddingFunc": ("row", None, [(0, 1)]),                          # ids (1, n) -> (1, n, D)
    "HyenaMixerFunc": ("batch", (0,), [(0,)]),                                   # x (B, Lx, 3 D) -> (B, L, D)
    "HyenaMixerCMFunc": ("batch", (1,), [(1,)]),                                 # xT (3 D, B, Lx) -> zT (D, B, L)
    "HyenaMixerOutCMFunc": ("batch", (1,), [(0,)]),                              # xT (3 D, B, L) -> (B, L, D)
    "HyenaMixerOutCMFunc+addnorm": ("batch", (1,), [(0,), (0,)]),                # ... -> out, residual (B, L, D)
    "HyenaMixerCMOrderNFunc": ("batch", (1,), [(1,)]),
    "HyenaMixerCMOrderNFunc+order4": ("batch", (1,), [(1,)]),
    "AddLayerNormFunc": ("row", (0, 1), [(0, 1), (0, 1)]),                       # x0 (b, l, D) -> out, residual (b, l, D)
    "EmbedAddLayerNormFunc": ("row", None, [(0, 1), (0, 1)]),
    "SoftEmbedAddLayerNormFunc": ("row", None, [(0, 1), (0, 1)]),                # row (0, 0) is soft token 0
    "AddNormPoolFunc": ("batch", (0,), [(0,)]),                                  # x0 (B, L, D) -> pooled (B, D)
    "RowHeadFunc": ("row", (0,), [(0,)]),
    "FusedMlpFunc": ("row", (0,), [(0,)]),
}
# (key, input) -> why that gradient is not connected to the planted element of dout.  Expected to be empty.
DISCONNECTED = {}
PLANTS = (("nan", float("nan")), ("+inf", float("inf")))


def unit0(t, axes):
    """bool mask of t's shape: unit 0 (every element where there are no unit axes)"""
    m = torch.ones(t.shape, dtype=torch.bool)
    for ax in axes:
        shape = [1] * t.dim()
        shape[ax] = t.shape[ax]
        m = m & (torch.arange(t.shape[ax]) == 0).view(shape)
    return m


def site(t, axes, allowed=None):
    """the planted element: index 0 on the unit's axes, the middle of every other axis (``allowed``: the nearest such element that it admits)"""
    idx = tuple(0 if ax in axes else t.shape[ax] // 2 for ax in range(t.dim()))
    if allowed is None or bool(allowed[idx]):
        return idx
    cand = (allowed & unit0(t, axes)).nonzero()
    assert len(cand), "no admissible element in unit 0"
    return tuple(cand[len(cand) // 2].tolist())


def _planted(t, idx, value):
    t = t.detach().clone()
    t[idx] = value
    return t


def _nonfinite(t, mask=None):
    t = t.detach().cpu().float()
    bad = ~torch.isfinite(t)
    return bool((bad if mask is None else bad & mask).any())


def _patterns(e):
    pats = [("all", frozenset(e.inputs))]
    if e.dk and set(e.inputs) - set(e.dk):
        pats.append(("need_dk=False", frozenset(set(e.inputs) - set(e.dk))))
    return pats


def connected(case, req, douts, d_idx):
    """Which gradient elements the planted element of dout feeds, where the case has an fp64 oracle: the oracle's gradients for a dout that is 1
    there and 0 elsewhere, an element counting as fed when it exceeds 1e-6 of the tensor's largest (the oracle's FFT leaves 1e-16 of it on
    the elements that are not).  A NaN or an inf times any number, and any sum with it, is not finite: every fed element must be non-finite,
    not just one per tensor -- a kernel that drops the value on ONE of its paths still fills the others.  -> {input: bool mask}, {} without oracle"""
    if case.oracle is None:
        return {}
    onehot = [torch.zeros_like(d) for d in douts]
    onehot[0][d_idx] = 1.0
    out = {}
    for n, g in AL.oracle_grads(case, req, onehot).items():
        if g is not None and bool((g != 0).any()):
            out[n] = g.abs() > 1e-6 * g.abs().max()
    return out


def suite_propagation(_lib, dev, key, i, gpu=False):
    """C1 - C4 for case ``i`` of REGISTRY[key] -> the number of planted runs"""
    e = AL.REGISTRY[key]
    kind, act_axes, out_axes = UNITS[key]
    case = e.cases(gpu)[i](dev)
    n_runs = 0
    for pname, req in _patterns(e):
        clean = AL.run(_lib, case, req)
        douts = case.douts
        outs_axes = out_axes
        assert len(outs_axes) == len(clean.outs), (key, [tuple(o.shape) for o in clean.outs])
        for o in clean.outs:
            assert not _nonfinite(o), (case.label, "the clean run is not finite")
        # ---- backward plants: one element of the first output's gradient, in unit 0
        d_idx = site(douts[0], outs_axes[0])
        conn = connected(case, req, douts, d_idx)
        for vname, value in PLANTS:
            planted = [_planted(douts[0], d_idx, value)] + list(douts[1:])
            got = AL.run(_lib, case, req, douts=planted)
            n_runs += 1
            tag = (case.label, pname, "dout" + str(d_idx), vname)
            assert got.spies.kernels() == clean.spies.kernels(), tag
            for a, b in zip(got.outs, clean.outs):
                assert same_bits(a.cpu(), b.cpu()), tag + ("the forward changed",)
            for n, g in got.grads.items():
                assert g is not None, tag + (n,)
                if (key, n) in DISCONNECTED:
                    continue
                inside = unit0(g, act_axes) if n == e.act else None
                assert _nonfinite(g, inside), tag + (n, "C4: the gradient is finite" + (" inside unit 0" if n == e.act else ""))
                if conn.get(n) is not None:
                    fin = torch.isfinite(g.detach().cpu().float()) & conn[n]
                    assert not bool(fin.any()), tag + (n, "C4: elements the planted one feeds are finite", int(fin.sum()), fin.nonzero()[:4].tolist())
            if e.act in got.grads and kind is not None:
                others = ~unit0(got.grads[e.act], act_axes)               # (empty at B = 1: that case holds propagation alone)
                a, b = got.grads[e.act].cpu()[others], clean.grads[e.act].cpu()[others]
                assert same_bits(a, b), tag + ("C3: the activation's gradient outside unit 0 changed", int((a != b).sum()))
        # ---- forward plants: one element of the activation, in unit 0 (on a kept element under dropout: one whose clean gradient is not zero)
        if e.act is None or pname != "all":
            continue
        x = case.vals[e.act]
        allowed = (clean.grads[e.act].cpu() != 0) if case.seed is not None else None
        x_idx = site(x, act_axes, allowed)
        for vname, value in PLANTS:
            c2 = copy.copy(case)
            c2.vals = dict(case.vals, **{e.act: _planted(x, x_idx, value)})
            got = AL.run(_lib, c2, req, douts=douts)
            n_runs += 1
            tag = (case.label, e.act + str(x_idx), vname)
            assert got.spies.kernels() == clean.spies.kernels(), tag
            for a, b, axes in zip(got.outs, clean.outs, outs_axes):
                inside = unit0(a, axes)
                assert _nonfinite(a, inside), tag + ("C2: the output is finite inside unit 0",)
                if kind is not None:
                    p, q = a.cpu()[~inside], b.cpu()[~inside]
                    assert same_bits(p, q), tag + ("C1: an output outside unit 0 changed", int((p != q).sum()))
    print(f"[nonfinite-local] {case.label}: {n_runs} planted runs", flush=True)
    return n_runs


def suite_mlp_bwd_nan_preactivation(_lib, dev, T):
    """mlp_dh_dgelu_bwd alone (operands as tests/proj_local.py draws them) with NaN planted in the SAVED pre-activation a -- what the forward
    leaves there after an overflow: da = dh gelu'(NaN) is NaN exactly at those elements and db1 exactly at their columns; every other element
    keeps the bits of the clean call.  (No Function-level plant reaches gelu' with a non-finite argument: C plants dout, and a stays clean.)"""
    from tests import proj_local as PL
    from tests import shell_local as SL
    P, K, N = 77, 128, 256
    g = torch.Generator().manual_seed(53)
    dy, W2T = PL._op((P, K), g, T, dev), PL._op((N, K), g, T, dev, PL.W_SCALE)
    a = (SL._operand((P, N), g, torch.float64, "cpu").sign() * (1.0 + torch.rand((P, N), generator=g, dtype=torch.float64))).to(T).to(dev)
    planted = a.clone()
    sites = [(0, 0), (5, 17), (63, 255), (64, 128), (76, 31)]                   # both tiles, first and last unit
    for p, n in sites:
        planted[p, n] = float("nan")
    da0, db0 = _lib.mlp_dh_dgelu_bwd(dy, W2T, a)
    da1, db1 = _lib.mlp_dh_dgelu_bwd(dy, W2T, planted)
    assert bool(torch.isfinite(da0.float()).all()) and bool(torch.isfinite(db0).all())
    mask = torch.zeros(P, N, dtype=torch.bool)
    for p, n in sites:
        mask[p, n] = True
    cols = mask.any(0)
    da0, da1, db0, db1 = da0.cpu(), da1.cpu(), db0.cpu(), db1.cpu()
    assert bool(torch.isnan(da1[mask]).all()), "gelu'(NaN) came back as a number"
    assert same_bits(da1[~mask], da0[~mask]), "a NaN pre-activation changed another element of da"
    assert bool(torch.isnan(db1[cols]).all()) and same_bits(db1[~cols], db0[~cols]), "db1: the NaN columns, and only they"


# ---- D. the loss scaler ---------------------------------------------------------------------------------------------------------------------
SCALER_CFG = (128, F16, 2, 0.0)               # autograd_local.LM_GRID's smallest width at which the fused out_proj and the matrix-core MLP run
SCALE_HIGH, SCALE_LOW = 2.0 ** 40, 2.0 ** 7


def _snapshot(m, opt):
    params = {n: p.detach().clone() for n, p in m.named_parameters()}
    state = {(id(p), k): v.detach().clone() for p, s in opt.state.items() for k, v in s.items() if torch.is_tensor(v)}
    return params, state


def _same_snapshot(a, b):
    return (a[0].keys() == b[0].keys() and a[1].keys() == b[1].keys() and all(same_bits(a[0][n].cpu(), b[0][n].cpu()) for n in a[0])
            and all(same_bits(a[1][n].cpu(), b[1][n].cpu()) for n in a[1]))


def scaled_backward(m, ids, tgt, dev, scale):
    """one fresh forward + backward of the loss times ``scale`` under fp16 autocast -> the names of the parameters whose gradient is not finite"""
    from hyena_dna_amd import _castcache, _gradsum
    _castcache.reset()
    _gradsum.reset()
    m.zero_grad(set_to_none=True)
    torch.manual_seed(1)
    with torch.autocast(dev.type, dtype=F16):
        loss = m.loss(ids, tgt)
    assert bool(torch.isfinite(loss)), "the loss itself is finite: only the scaled backward overflows"
    (loss.float() * scale).backward()
    return [n for n, p in m.named_parameters() if p.grad is not None and not bool(torch.isfinite(p.grad).all())]


def _scaler_step(m, opt, ids, tgt, dev, init_scale):
    from hyena_dna_amd import _castcache, _gradsum
    _castcache.reset()
    _gradsum.reset()
    scaler = torch.amp.GradScaler(dev.type, init_scale=init_scale)
    opt.zero_grad(set_to_none=True)
    torch.manual_seed(1)
    with torch.autocast(dev.type, dtype=F16):
        loss = m.loss(ids, tgt)
    scaler.scale(loss).backward()
    scaler.unscale_(opt)
    bad = [n for n, p in m.named_parameters() if p.grad is not None and not bool(torch.isfinite(p.grad).all())]
    before = _snapshot(m, opt)
    scaler.step(opt)
    scaler.update()
    return bad, before, _snapshot(m, opt), scaler.get_scale()


def suite_scaler_steps(_lib, dev, gpu=False):
    """init_scale 2^40: every logit gradient is scale |p - y| / N with N = 142 <= 2^10 rows and 12 classes near uniform, above 2^26 for the
    target class -- beyond fp16 whatever the model holds.  The step must be skipped and the scale halved.  2^7 on the same model and batch:
    applied, scale kept.  And 2^40 once more, now that AdamW has state: parameters and state keep their bits."""
    with AL.Spies(_lib) as sp:
        m, ids, tgt = AL.lm_build(dev, SCALER_CFG)
        opt = torch.optim.AdamW(m.parameters(), lr=1e-3)
        bad, before, after, scale = _scaler_step(m, opt, ids, tgt, dev, SCALE_HIGH)
    # (the matrix-core in_proj and MLP read the device's autocast state: under the emulator's CPU autocast the library GEMMs stand in for them)
    for f in ("HyenaMixerOutCMFunc", "AddLayerNormFunc") + (("FusedMlpFunc", "InProjPreCMFunc") if gpu else ()):
        assert sp.ran.get(f), (f, "did not run: this is not the fused 16-bit model", sp.ran)
    assert bad, "2^40: every parameter gradient is finite after unscale_ -- the overflow was laundered on its way"
    assert _same_snapshot(before, after) and not after[1], "2^40: the step was applied"
    assert scale == SCALE_HIGH / 2, scale
    bad, before, after, scale = _scaler_step(m, opt, ids, tgt, dev, SCALE_LOW)
    assert not bad, ("2^7: not finite", bad)
    assert after[1] and any(not same_bits(before[0][n].cpu(), after[0][n].cpu()) for n in before[0]), "2^7: the step was not applied"
    assert scale == SCALE_LOW, scale
    bad, before, after, scale = _scaler_step(m, opt, ids, tgt, dev, SCALE_HIGH)
    assert bad and before[1] and _same_snapshot(before, after) and scale == SCALE_HIGH / 2, (len(bad), scale)
    print(f"[nonfinite-local] scaler: {len(bad)} parameters with a non-finite gradient at 2^40", flush=True)


def suite_scaler_sweep(_lib, dev):
    """2^40 down to 2^7 in halvings: overflowed at and above some s*, clean below it -> log2 s*"""
    m, ids, tgt = AL.lm_build(dev, SCALER_CFG)
    flags = [(e, bool(scaled_backward(m, ids, tgt, dev, 2.0 ** e))) for e in range(40, 6, -1)]
    assert flags[0][1] and not flags[-1][1], flags
    first_clean = [f for _, f in flags].index(False)
    assert all(f for _, f in flags[:first_clean]) and not any(f for _, f in flags[first_clean:]), ("not monotone", flags)
    s_star = flags[first_clean - 1][0]
    print(f"[nonfinite-local] scaler sweep on {_lib._backend.name}: s* = 2^{s_star}", flush=True)
    return s_star


# ---- B. the store conversion: exact carrier ---------------------------------------------------------------------------------------------------
CVT_DTYPES = (F32, BF16, F16)
CVT_D, CVT_L = 16, 65536
_ULP1 = {F16: 2.0 ** -10, BF16: 2.0 ** -7}


def cvt_multipliers(T):
    """16 finite multipliers, exact in T (fp32 I/O takes bf16's: every one of them, and every product with a bf16 pattern, is exact in fp32)"""
    t = BF16 if T == F32 else T
    fi = torch.finfo(t)
    m = [1.0, -1.0, 2.0, 0.5, 1.0 + _ULP1[t], 1.5, 3.0, 1040.0, fi.max, fi.smallest_normal, fi.smallest_normal * _ULP1[t], 0.0, -0.0, -3.0, 0.75,
         1.0 - _ULP1[t] / 2]
    v = torch.tensor(m, dtype=torch.float64)
    assert len(m) == CVT_D and torch.equal(v.to(t).double(), v) and bool(torch.isfinite(v).all())
    return v.to(T)


def all_patterns(T):
    """every bit pattern of the 16-bit type, +-0, subnormals, +-inf and every NaN among them (fp32 I/O: the bf16 patterns widened)"""
    bits = torch.arange(65536, dtype=torch.int32).to(torch.int16)               # (wraps: pattern p as the int16 of the same bits)
    return bits.view(BF16).float() if T == F32 else bits.view(T)


def suite_cvt_exact(_lib, dev, T):
    """z[d, 0, p] = cvt(pattern p * multiplier d) from cm_post_fwd on its own, against the one rounding of the exact product.  The kernel's
    c0 is fma(1, x + 0.0f, +0) by its own definition (an absent in_proj bias is +0.0f): that is x for every finite x but -0, which it
    turns into +0 -- the expected product takes the multiplier as x + 0.0 for that reason, signs of zero included everywhere."""
    lib, D, L = _lib.lib(), CVT_D, CVT_L
    code, stream = _lib.dtype_code(T), _lib._backend.stream(dev)
    mult = cvt_multipliers(T)
    y = all_patterns(T)[None, None, :].repeat(1, D, 1).contiguous()             # (B, D, L)
    x = torch.zeros(3 * D, 1, L, dtype=T)
    x[:D, 0, :] = mult[:, None]
    assert 63.0 in y[0, 7].double().tolist() and float(mult[7]) == 1040.0       # 1040 * 63 = 65520: the tie that rounds to fp16 inf
    w = torch.zeros(3 * D, 3)
    w[:, 2] = 1.0
    b = torch.zeros(3 * D)
    want = (y[0].double() * (x[:D, 0].double() + 0.0)).to(T)                    # (D, L); exact in fp32, so one rounding
    if T == F16:
        assert want[7].double()[y[0, 7].double() == 63.0].tolist() == [float("inf")]
    cs = _lib.row_pitch(L)
    yd, xd, wd, bd = y.to(dev), x.to(dev), w.to(dev), b.to(dev)
    z = torch.full((D * cs,), 1536.0, dtype=T).to(dev)
    with _lib._backend.guard(dev):
        _lib.check(lib.hyena_cm_post_fwd_ld(yd.data_ptr(), xd.data_ptr(), None, wd.data_ptr(), bd.data_ptr(), z.data_ptr(), 1, L, L, D, L, L, cs, L, L,
                                            code, stream))
    got = torch.as_strided(z, (D, L), (cs, 1)).cpu()
    it = torch.int32 if T == F32 else torch.int16
    nan = torch.isnan(want)
    ok = torch.where(nan, torch.isnan(got), got.contiguous().view(it) == want.view(it))
    bad = (~ok).nonzero()
    print(f"[nonfinite-local] cvt {AL.NAME[T]}: {int(nan.sum())} NaN expected, {int(torch.isinf(want).sum())} inf, {len(bad)} mismatches", flush=True)
    assert not len(bad), [(float(mult[d]), hex(p), float(want[d, p]), float(got[d, p])) for d, p in bad[:8].tolist()]


# ---- B. the store conversion: threshold carriers ----------------------------------------------------------------------------------------------
# One kernel per remaining store helper, alone, fp16, operands scaled (by powers of two, chosen from the reference alone) until part of the
# outputs leaves fp16's range.  ref, E: the module's own fp64 reference and fp32 error bound; `bound`: the module's existing element-wise bound.
#   |ref| - E >= 65520: the stored value is inf with ref's sign      (fp16 rounds to nearest even: 65520 is the tie that goes to inf)
#   |ref| + E <= 65504: finite and within `bound`
#   in between: either; never NaN.  At most 1 % of the outputs lie in between, at least 64 and at most half are certain to overflow.
F16_MAX, F16_TIE = 65504.0, 65520.0
_shares = {}


def hold_threshold(name, got, ref, E, bound):
    assert got.dtype == F16 and got.shape == ref.shape, (name, got.dtype, got.shape, ref.shape)
    got, a = got.cpu(), ref.abs()
    over, under = a - E >= F16_TIE, a + E <= F16_MAX
    share = float((~(over | under)).double().mean())
    _shares[name] = (int(over.sum()), ref.numel(), share)
    print(f"[nonfinite-local] threshold {name}: {int(over.sum())} of {ref.numel()} outputs overflow, {share:.3%} in between", flush=True)
    assert 64 <= int(over.sum()) <= ref.numel() // 2 and share <= 0.01, (name, int(over.sum()), ref.numel(), share)
    assert not bool(torch.isnan(got).any()), (name, "NaN stored")
    g = got.double()
    bad = over & ~(torch.isinf(g) & (torch.sign(g) == torch.sign(ref)))
    assert not bool(bad.any()), (name, "an overflow was not stored as inf of the reference's sign", int(bad.sum()), g[bad][:4].tolist(), ref[bad][:4].tolist())
    fin = under & torch.isfinite(g)
    assert bool((fin == under).all()), (name, "a value inside the range was stored as inf", int((under & ~fin).sum()))
    d = (g - ref).abs()
    assert bool((d[under] <= bound[under]).all()), (name, float((d[under] / bound[under].clamp_min(1e-300)).max()))


def thr_fftconv(_lib, dev, L):
    """fftconv_fwd, B = 1, D = 2: k and bias scaled so that a row's rms is about 45000"""
    from tests import fftconv_local as FL
    u, k, b, _ = FL.inputs(1, 2, L, F16, 11 * L)
    s = 45000.0 / float(FL._rms(FL.ref64(u, k, b, u)[0]).max())
    k, b = (k * s).float(), (b * s).float()
    ref = FL.ref64(u, k, b, u)[0]
    E = FL.c_bound(L)[0] * FL.U * FL._rms(ref).expand_as(ref)
    out = _lib.fftconv_fwd(u.to(dev), k.to(dev), b.to(dev))
    hold_threshold(f"fftconv_fwd L={L}", out, ref, E, E + FL.half_ulp_io(ref.abs(), F16))


def thr_mixer_post(_lib, dev, D):
    """mixer_post_fwd (narrow: D = 8; wide: D = 64): y scaled by 2^14"""
    from tests import shell_local as SL
    B, L, Lx = 2, 321, 322
    lib, code, stream = _lib.lib(), _lib.dtype_code(F16), _lib._backend.stream(dev)
    g = torch.Generator().manual_seed(D)
    w, b, _ = SL._params(3 * D, g, dev, False)
    x = SL._operand((B, Lx, 3 * D), g, F16, dev)
    y = (SL._operand((B, D, L), g, torch.float64, "cpu") * 2.0 ** 14).to(F16).to(dev)
    z = torch.full((B, L, D), SL.SENTINEL, dtype=F16, device=dev)
    with _lib._backend.guard(dev):
        _lib.check(lib.hyena_mixer_post_fwd(y.data_ptr(), x.data_ptr(), w.data_ptr(), b.data_ptr(), z.data_ptr(), B, L, Lx, D, code, stream))
    ref, E = SL.post_fwd64(x.cpu().permute(2, 0, 1).double(), None, w.cpu().double(), b.cpu().double(), y.cpu().double(), L)
    ref, E = ref.permute(1, 2, 0), E.permute(1, 2, 0)
    hold_threshold(f"mixer_post_fwd D={D}", z, ref, E, E + SL.half_ulp_io(ref.abs() + E, F16))


def thr_add_norm(_lib, dev):
    """add_norm_fwd's out (blk_store): the LayerNorm weight scaled by 2^15"""
    from tests import block_local as BL
    rows, D = 37, 128
    g = torch.Generator().manual_seed(5)
    w, b = BL.draw_params(D, g, dev)
    w = w * 2.0 ** 15
    x0, res = BL.draw_forward((rows,), D, F16, True, 0.0, g, dev)
    out = _lib.add_norm_fwd(x0, res, w, b, BL.EPS, F16)[0]
    R = BL.fwd64(x0.cpu().double(), res.cpu().double(), w.cpu().double(), b.cpu().double(), None, 1.0)
    hold_threshold("add_norm_fwd", out, R["out"], R["E_out"], R["E_out"] + BL.half_ulp_io(R["out"].abs() + R["E_out"], F16))


def thr_decode_post(_lib, dev):
    """decode_post, single form (Elem::st), position 0: partials and history as tests/decode_local.py draws them, x0 scaled"""
    from tests import decode_local as DL
    B, D, Lcap, t = 4, 256, 8200, 0
    lib, code, stream = _lib.lib(), _lib.dtype_code(F16), _lib._backend.stream(dev)
    g = torch.Generator().manual_seed(17)
    nch, ldr = -(-Lcap // DL.CHUNK), DL._ceil(Lcap, 8)
    part = torch.full((nch, B, 1, D), DL.NAN, device=dev)
    part[0] = DL.flat((B, 1, D), g, F32, dev, 1.0, 2.0)
    vt = DL.flat((B, 1, D), g, F16, dev, 1.0, 2.0)
    vgr = torch.full((B, D, ldr), DL.NAN, dtype=F16, device=dev)
    vgr[:, :, t] = vt[:, 0]
    x0 = DL.flat((B, 1, D), g, F32, dev) * 20000.0
    fb = DL.flat((D,), g, F32, dev, 1.0, 2.0)
    z = torch.full((B, 1, D), DL.SENTINEL, dtype=F16, device=dev)
    pos = torch.tensor([t], dtype=torch.int32, device=dev)
    with _lib._backend.guard(dev):
        _lib.check(lib.hyena_decode_post(part.data_ptr(), vgr.data_ptr(), fb.data_ptr(), x0.data_ptr(), z.data_ptr(), pos.data_ptr(), B, D, Lcap, ldr,
                                         code, stream))
    assert pos.tolist() == [t + 1]
    f = fb.cpu().double()[None, None, :] * vt.cpu().double()
    y64, A, x64 = part[0].cpu().double() + f, part[0].cpu().double().abs() + f.abs(), x0.cpu().double()
    nc = torch.ones(())
    Eyr = DL.gamma(nc + 1.0) * A
    Eyr = Eyr + DL.half_ulp_io(y64.abs() + Eyr, F16)
    e = x64.abs() * Eyr
    m = (y64 * x64).abs() + e
    E = e + DL.U * m                                                            # post_bound without the last rounding
    bound = DL.post_bound(y64, A, nc, x64, F16)
    assert torch.equal(bound, E + DL.half_ulp_io(m + DL.U * m, F16))
    hold_threshold("decode_post single", z, y64 * x64, E, bound)


def thr_mlp(_lib, dev):
    """mlp_fc1_gelu_fwd's a: x scaled by 2^14, the weights by 2"""
    from tests import proj_local as PL
    P, K, N = 77, 128, 256
    g = torch.Generator().manual_seed(31)
    x, W1 = PL._op((P, K), g, F16, dev, 2.0 ** 14), PL._op((N, K), g, F16, dev, PL.W_SCALE * 2)
    b1 = PL._op((N,), g, F16, dev, 0.25).float()
    assert _lib.mlp_supported(P, K, N, F16)
    a, _ = _lib.mlp_fc1_gelu_fwd(x, W1, b1)
    ref, E = PL.product64(W1.cpu().double(), x.cpu().double(), b1.cpu().double())
    ref, E = ref.t(), E.t()
    hold_threshold("mlp_fc1_gelu_fwd a", a, ref, E, E + PL.half_ulp_io(ref.abs() + E, F16))


def thr_outproj(_lib, dev):
    """outproj_gate_fwd's out against the STORED zT (finite: only the product leaves the range): out_proj's weight scaled by 2^13"""
    from tests import proj_local as PL
    from tests import shell_local as SL
    B, L, D = 2, 65, 128
    rp = _lib.row_pitch
    g = torch.Generator().manual_seed(41)
    w, b, bin_ = SL._params(3 * D, g, dev, True)
    w, b, bin_ = w.abs(), 1.0 + b.abs(), bin_.abs()
    x, xs, csx, bsx = PL._x0(B, L, L, D, g, F16, dev, "cm", rp)
    x.view[:D, :, :L] = x.view[:D, :, :L].abs()
    ys, lda = SL.rows_strides(B, D, L, True, rp)
    y = SL.Buf.input(PL._op((B, D, L), g, F16, dev), ys)
    W = PL._op((D, D), g, F16, dev, PL.W_SCALE * 2.0 ** 13)
    ob = PL._op((D,), g, F16, dev, 0.25).float()
    assert _lib.outproj_supported(B, L, L, D, F16)
    out, zT = _lib.outproj_gate_fwd(y.view, x.view, bin_, w, b, W, ob, want_z=True)
    z2 = zT.cpu().double().permute(1, 2, 0).reshape(B * L, D)
    assert bool(torch.isfinite(z2).all())
    ref, E = PL.product64(W.cpu().double(), z2, ob.cpu().double())
    ref, E = ref.t(), E.t()
    hold_threshold("outproj_gate_fwd out", out.reshape(B * L, D), ref, E, E + PL.half_ulp_io(ref.abs() + E, F16))


THRESHOLD = {
    "add_norm_fwd": thr_add_norm,
    "mixer_post_fwd-narrow": lambda lib, dev: thr_mixer_post(lib, dev, 8),
    "mixer_post_fwd-wide": lambda lib, dev: thr_mixer_post(lib, dev, 64),
    "decode_post-single": thr_decode_post,
    "outproj_gate_fwd": thr_outproj,
    "mlp_fc1_gelu_fwd": thr_mlp,
    "fftconv_fwd-L2048": lambda lib, dev: thr_fftconv(lib, dev, 2048),
    "fftconv_fwd-L32768": lambda lib, dev: thr_fftconv(lib, dev, 32768),
}


def suite_threshold(_lib, dev, name):
    THRESHOLD[name](_lib, dev)
