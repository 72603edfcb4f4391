"""The autograd layer above the kernels -- the 17 torch.autograd.Functions of hyena_dna_amd -- held to its gradients under freezing, recompute,
retained graphs and gradient layouts.  Shared by the emulator tests (tests/test_autograd_local_emu.py) and the GPU tests
(tests/test_gpu_autograd_local.py).  Plain torch; not a test file.  Tables, counts, run times and the seeded defects: profiles/autograd_local.md.

REGISTRY has one entry per Function: its differentiable inputs, its named input groups, and cases -- each a builder that reaches the Function
through the public wrapper that selects it (where that wrapper sits behind an ``is_cuda`` gate the emulator calls ``.apply`` and the device
goes through the wrapper).  A case runs under PATTERNS: the sets of inputs that require a gradient.  Per pattern (check_pattern):
    (a) the output is the all-required run's, bit for bit
    (b) every input that requires a gradient gets a finite tensor of its own shape and type, never None
    (c) every other input gets None
    (d) every gradient is the all-required run's bit for bit when the same kernels ran -- the kernels: tests.fftconv_local.route for every long
        convolution plus the names of the _lib entry points that ran; where the route legitimately differs (``need_dk=False``, ``need_du=False``,
        ``spectra=absent``: the pattern's id says so) the gradient is held to the fp64 oracle gradient (oracle.hyena_oracle's pieces in float64 under
        torch autograd) at the tolerance tests/test_gpu_contract.py holds that gradient to at that type (ORACLE_TOL, no constant of its own)
    (e) optional work is skipped when frozen: the flags the spies saw at _lib.fftconv_bwd / outproj_gate_fwd are the ones the pattern implies
and a spy on ``Func.apply`` shows that the Function ran: a case that falls through to a generic PyTorch path fails."""
import importlib
import itertools
import pkgutil

import torch
import torch.nn.functional as F

from oracle import hyena_oracle as O
from tests import fftconv_local as FL

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
NAME = {F32: "fp32", BF16: "bf16", F16: "fp16"}
same_bits = FL.same_bits

# Gradient tolerances (relative L2 against the fp64 oracle), each the one tests/test_gpu_contract.py holds the same gradient to at that type; the
# emulator file asserts that these literals still stand in that file at the statements named here.
CONTRACT_SOURCE = {
    "op_fp32": ("ty, tg = 2e-5, 2e-4", 2e-4),             # test_operator_at_contract_shapes_vs_oracle, fp32
    "op_16": ("ty, tg = 1.5e-2, 3e-2", 3e-2),             # ... 16-bit operands around the fp32 filter
    "op_16_filter16": ("ty, tg = 3e-2, 6e-2", 6e-2),      # ... bf16 autocast, the filter from the 16-bit kernels
    "order_n_fp32": ("ty, tg = 3e-5, 3e-4", 3e-4),        # test_operator_of_higher_order_vs_oracle, fp32
    "order_n_16": ("ty, tg = 2e-2, 4e-2", 4e-2),          # ... 16-bit
    "core_16": ("assert e < 1.2e-2, (n, e)", 1.2e-2),     # test_mixer_core_cm_at_contract_shapes_vs_oracle, bf16 tensors
}
ORACLE_TOL = {k: v[1] for k, v in CONTRACT_SOURCE.items()}

# the _lib entry points whose calls make up a run's kernel list (flags: what of a call's arguments selects another kernel or optional work)
KERNELS = ("fftconv_fwd", "fftconv_bwd", "mixer_pre_fwd", "mixer_post_fwd", "mixer_post_bwd", "mixer_pre_bwd", "cm_pre_fwd", "cm_post_fwd",
           "cm_post_bwd", "cm_pre_bwd", "inproj_pre_fwd", "outproj_gate_fwd", "outproj_gate_addnorm_fwd", "outproj_dgrad_gate_bwd", "colsum",
           "mlp_fc1_gelu_fwd", "mlp_dh_dgelu_bwd", "filter_fwd", "filter_bwd", "add_norm_fwd", "add_norm_bwd", "embed_add_norm_fwd",
           "embed_add_norm_bwd", "soft_embed_add_norm_fwd", "soft_embed_add_norm_bwd", "row_head_fwd", "row_head_bwd", "add_norm_pool_fwd",
           "add_norm_pool_bwd")


def function_classes():
    """every torch.autograd.Function subclass defined under hyena_dna_amd/, by a scan of the package: {class name: class}"""
    import hyena_dna_amd
    found = {}
    for m in pkgutil.iter_modules(hyena_dna_amd.__path__):
        if m.name == "build":
            continue
        mod = importlib.import_module("hyena_dna_amd." + m.name)
        for v in vars(mod).values():
            if isinstance(v, type) and issubclass(v, torch.autograd.Function) and v.__module__ == mod.__name__:
                found[v.__name__] = v
    return found


# ---- spies ------------------------------------------------------------------------------------------------------------------------------
class Spies:
    """While active: counts the calls of every registered Function's ``apply`` (``ran``) and records the calls of the _lib entry points in
    KERNELS with their route-selecting flags (``calls``; ``kernels()`` is the list (d) compares)."""

    def __init__(self, _lib):
        self._lib, self.ran, self.calls, self._undo = _lib, {}, [], []

    def __enter__(self):
        for name, cls in function_classes().items():
            had = cls.__dict__.get("apply")
            orig = cls.apply

            def apply(*a, _n=name, _o=orig):
                self.ran[_n] = self.ran.get(_n, 0) + 1
                return _o(*a)
            cls.apply = staticmethod(apply)
            self._undo.append((cls, "apply", had))
        for name in KERNELS:
            real = getattr(self._lib, name)

            def spy(*a, _n=name, _r=real, **k):
                self.calls.append((_n, self._flags(_n, a, k)))
                return _r(*a, **k)
            setattr(self._lib, name, spy)
            self._undo.append((self._lib, name, real))
        return self

    def __exit__(self, *exc):
        for obj, name, old in reversed(self._undo):
            if old is None:
                delattr(obj, name)
            else:
                setattr(obj, name, old)
        self._undo = []

    def _flags(self, n, a, k):
        if n == "fftconv_fwd":
            return {"save": bool(k.get("save", a[4] if len(a) > 4 else False)), "shape": tuple(a[0].shape)}
        if n == "fftconv_bwd":
            B, D, L = a[0].shape
            need_du = bool(k.get("need_du", a[4] if len(a) > 4 else True))
            need_dk = bool(k.get("need_dk", a[5] if len(a) > 5 else True))
            saved = k.get("saved", a[7] if len(a) > 7 else None) is not None
            return {"need_du": need_du, "need_dk": need_dk, "saved": saved, "route": FL.route(self._lib, B, D, L, need_du, need_dk, saved)}
        if n in ("outproj_gate_fwd", "outproj_gate_addnorm_fwd"):
            return {"want_z": bool(k.get("want_z", a[7] if len(a) > 7 else False))}
        if n == "filter_fwd":
            return {"save": bool(k.get("save", a[13] if len(a) > 13 else False))}
        if n == "filter_bwd":
            return {"need_dz": bool(k.get("need_dz"))}
        return {}

    def of(self, name):
        return [f for n, f in self.calls if n == name]

    def kernels(self):
        """the kernels that ran: the entry points' names in call order, a long convolution's backward as its route"""
        return [n + (":" + f["route"] if n == "fftconv_bwd" else "") for n, f in self.calls]


# ---- cases ------------------------------------------------------------------------------------------------------------------------------
class Case:
    """One way into one Function: ``vals`` the differentiable inputs by name (on the device, detached), ``call(t)`` the public wrapper on live
    tensors ``t`` -> output or tuple of outputs, ``oracle(t64)`` the same function in plain torch on float64 tensors (only where a route can
    differ), ``tol`` the ORACLE_TOL key, ``flags(req)`` the spy flags the pattern ``req`` implies ({} where there are none)."""

    def __init__(self, func, label, dtype, vals, call, oracle=None, tol=None, flags=None, seed=None):
        self.func, self.label, self.dtype, self.vals, self.call, self.oracle, self.tol = func, label, dtype, vals, call, oracle, tol
        self.flags = flags or (lambda req: {})
        self.seed = seed
        self.douts = None

    def live(self, req):
        return {n: v.detach().clone().requires_grad_(n in req) for n, v in self.vals.items()}

    def grad_outputs(self, outs):
        if self.douts is None:
            g = torch.Generator().manual_seed(4242)
            self.douts = [torch.randn(o.shape, generator=g).to(dtype=o.dtype, device=o.device) for o in outs]
        return self.douts


def _tup(x):
    return tuple(x) if isinstance(x, (tuple, list)) else (x,)


class Run:
    def __init__(self, outs, grads, spies):
        self.outs, self.grads, self.spies = outs, grads, spies


def run(_lib, case, req, douts=None, backwards=1, no_grad=False):
    """forward of ``case`` with the inputs in ``req`` requiring a gradient, and ``backwards`` backward passes over the one graph (retained between
    them) -> Run, or a list of Runs (one per backward, each with its own spies on the backward alone; the first carries the forward's)"""
    from hyena_dna_amd import _castcache, _gradsum
    _castcache.reset()
    _gradsum.reset()
    if case.seed is not None:
        torch.manual_seed(case.seed)
    t = case.live(req)                       # (under no_grad too: the inputs still require a gradient, as a trained model's parameters do when it is served)
    with Spies(_lib) as fwd:
        if no_grad:
            with torch.no_grad():
                outs = _tup(case.call(t))
        else:
            outs = _tup(case.call(t))
    assert fwd.ran.get(case.func, 0) >= 1, (case.func, "did not run: the call fell through to another path", fwd.ran)
    if no_grad:
        return Run([o.detach() for o in outs], {}, fwd)
    names = [n for n in case.vals if n in req]
    diff = [(o, g) for o, g in zip(outs, case.grad_outputs(outs) if douts is None else douts) if o.requires_grad]
    assert diff, "no output is connected to the inputs that require a gradient"
    runs = []
    for i in range(backwards):
        with Spies(_lib) as bwd:
            gs = torch.autograd.grad([o for o, _ in diff], [t[n] for n in names], [g for _, g in diff], retain_graph=i + 1 < backwards,
                                     allow_unused=True)
        sp = bwd
        if i == 0:
            sp.calls = fwd.calls + bwd.calls
            sp.ran = fwd.ran
        runs.append(Run([o.detach() for o in outs], dict(zip(names, gs)), sp))
        for n in case.vals:                                        # (c): autograd.grad fills no .grad; nothing else may have
            assert t[n].grad is None, n
    return runs[0] if backwards == 1 else runs


def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()


def oracle_grads(case, req, douts):
    """the fp64 oracle gradients of the inputs in ``req``: case.oracle on float64 copies of the inputs as the kernels see them, torch autograd"""
    t = {n: v.detach().cpu().double().requires_grad_(n in req) for n, v in case.vals.items()}
    outs = _tup(case.oracle(t))
    names = [n for n in case.vals if n in req]
    gs = torch.autograd.grad(outs, [t[n] for n in names], [g.detach().cpu().double() for g in douts], allow_unused=True)
    return dict(zip(names, gs))


def check_pattern(case, base, got, req, named=()):
    """(a) - (e) of the module docstring for one pattern ``req`` against the all-required run ``base``; ``named``: the route differences the
    pattern's id names -- the only ones a differing kernel list may come from.  -> "same kernels" or the difference"""
    for a, b in zip(got.outs, base.outs):
        assert same_bits(a.cpu(), b.cpu()), (case.label, sorted(req), "(a) the output changes with the pattern")
    for n, v in case.vals.items():
        if n in req:
            g = got.grads.get(n)
            assert g is not None, (case.label, sorted(req), n, "(b) requires a gradient and got None")
            assert g.shape == v.shape and g.dtype == v.dtype, (case.label, n, g.shape, g.dtype)
            assert bool(torch.isfinite(g).all()), (case.label, n, "not finite")
        else:
            assert n not in got.grads
    want = case.flags(req)
    for key, v in want.items():                                    # (e)
        entry, flag = key.split(".")
        seen = [f[flag] for f in got.spies.of(entry)]
        if v is None:
            assert not seen, (case.label, sorted(req), key, "ran, and nothing asks for it", seen)
        else:
            assert seen and all(s == v for s in seen), (case.label, sorted(req), key, "expected", v, "saw", seen)
    kb, kg = base.spies.kernels(), got.spies.kernels()
    conv = lambda ks: [k for k in ks if k.startswith("fftconv_bwd:")]      # noqa: E731
    left = list(kb)
    for k in kg:                                                   # frozen inputs only ever take work away
        if not k.startswith("fftconv_bwd:"):
            assert k in left, (case.label, sorted(req), k, "ran here and not in the all-required run")
            left.remove(k)
    differs = bool(conv(kg)) and conv(kg) != conv(kb)
    if differs:
        assert named, (case.label, sorted(req), "the long convolution's backward takes another route and the id names none", conv(kg), conv(kb))
        assert case.oracle is not None, (case.label, "a route differs and the case has no oracle")
        ref = oracle_grads(case, req, case.douts)
        for n, r in ref.items():
            e = _rel(got.grads[n].cpu(), r)
            assert e < ORACLE_TOL[case.tol], (case.label, sorted(req), n, "(d) against the fp64 oracle", e, ORACLE_TOL[case.tol], conv(kg))
        bits = all(same_bits(got.grads[n].cpu(), base.grads[n].cpu()) for n in got.grads)
        return " | ".join(conv(kg)) + "  (all-required: " + " | ".join(conv(kb)) + f"; bits of the all-required run: {bits})"
    for n in got.grads:
        assert same_bits(got.grads[n].cpu(), base.grads[n].cpu()), (case.label, sorted(req), n, "(d) same kernels, other bits")
    return "same kernels"


# ---- patterns ---------------------------------------------------------------------------------------------------------------------------
def patterns(inputs, groups, act):
    """the sets of inputs that require a gradient.  At most five inputs: every non-empty subset.  More: each input alone, all but each one, all,
    and the named groups -- each once with the activation input and once without.  -> [(id, frozenset)] without duplicates"""
    inputs = tuple(inputs)
    out, seen = [], set()

    def add(name, s):
        s = frozenset(s)
        if s and s not in seen:
            seen.add(s)
            out.append((name, s))
    if len(inputs) <= 5:
        for r in range(1, len(inputs) + 1):
            for c in itertools.combinations(inputs, r):
                add("+".join(c), c)
        return out
    named = [("only_" + n, {n}) for n in inputs] + [("all_but_" + n, set(inputs) - {n}) for n in inputs] + [("all", set(inputs))]
    named += [(g, set(m)) for g, m in groups.items()]
    for name, s in named:
        if act is None:
            add(name, s)
            continue
        add(name + "-act", set(s) | {act})
        add(name + "-noact", set(s) - {act})
    return out


def pattern_id(entry, name, req):
    """the pattern's id, with the route differences it can legitimately cause"""
    d = entry.diffs(req)
    return name + ("".join("[" + x + "]" for x in d))


class Entry:
    def __init__(self, func, inputs, act, groups, cases_emu, cases_gpu=None, dk=(), du=None, route=""):
        self.func, self.inputs, self.act, self.groups, self.route = func, tuple(inputs), act, groups, route
        self.cases_emu, self.cases_gpu = cases_emu, cases_gpu if cases_gpu is not None else cases_emu
        self.dk, self.du = tuple(dk), du

    def patterns(self):
        return patterns(self.inputs, self.groups, self.act)

    def diffs(self, req):
        """the flags of the long convolution's backward that this pattern changes against the all-required run"""
        d = []
        if self.dk and not any(n in req for n in self.dk):
            d.append("need_dk=False")
        if self.du is not None and self.du not in req:
            d.append("need_du=False")
        return tuple(d)

    def cases(self, gpu):
        return self.cases_gpu if gpu else self.cases_emu


# ---- builders -----------------------------------------------------------------------------------------------------------------------------
def _g(seed):
    return torch.Generator().manual_seed(seed)


def _rn(g, *shape, scale=1.0):
    return torch.randn(*shape, generator=g) * scale


def _filter_like(g, D, L):
    return _rn(g, D, L) * torch.exp(-4 * torch.linspace(0, 1, L)) * 0.2


def _conv_flags(dk, du=None, z=None, early=None):
    """flags(req) of a case whose Function runs one or more long convolutions: need_dk from the inputs in ``dk``, need_du from ``du`` (None:
    always), want_z from ``z``; ``early``: the inputs of which one must require a gradient for the convolution's backward to run at all"""
    def flags(req):
        f = {}
        if early is not None and not any(n in req for n in early):
            f["fftconv_bwd.need_dk"] = None
        else:
            f["fftconv_bwd.need_dk"] = any(n in req for n in dk)
            if du is not None:
                f["fftconv_bwd.need_du"] = du in req
        if z is not None:
            f["outproj_gate_fwd.want_z" if z[1] == "plain" else "outproj_gate_addnorm_fwd.want_z"] = z[0] in req
        return f
    return flags


def case_fftconv(dev, T, B, D, L):
    from hyena_dna_amd.fftconv import fftconv_func
    u, k, b, _ = FL.inputs(B, D, L, T, 11 * L + D)
    vals = {"u": u.to(dev), "k": k.to(dev), "D": b.to(dev)}
    return Case("FFTConvFunc", f"fftconv-{NAME[T]}-B{B}-D{D}-L{L}", T, vals, lambda t: fftconv_func(t["u"], t["k"], t["D"], gelu=False),
                oracle=lambda t: O.fftconv_ref(t["u"], t["k"], t["D"]), tol="op_fp32" if T == F32 else "core_16",
                flags=_conv_flags(("k", "D"), du="u"))


def _filter_oracle(t, tt, deltas, shift):
    h = t["z"]
    for w, b in (("w0", "b0"), ("w1", "b1"), ("w2", "b2")):
        h = torch.sin(t["freq"] * (h @ t[w].t() + t[b]))
    k = (h @ t["w3"].t()) * (torch.exp(-tt.double()[:, None] * deltas.double().abs()[None]) + shift)
    return k.t()


def case_filter(dev, L, D, E=5, order=64):
    from hyena_dna_amd.filter import hyena_filter_dl
    g = _g(L + D)
    z, tt = O.positional_embedding(E, L)
    z, tt = z[0, :L].contiguous(), tt.reshape(-1)[:L].contiguous()
    deltas = torch.linspace(0.5, 3.0, D)
    vals = {"z": z, "w0": _rn(g, order, E, scale=0.4), "b0": _rn(g, order, scale=0.1), "w1": _rn(g, order, order, scale=0.1),
            "b1": _rn(g, order, scale=0.1), "w2": _rn(g, order, order, scale=0.1), "b2": _rn(g, order, scale=0.1),
            "w3": _rn(g, D, order, scale=0.1), "freq": torch.full((order,), 1.5) + _rn(g, order, scale=0.1)}
    vals = {n: v.to(dev) for n, v in vals.items()}
    td, dd = tt.to(dev), deltas.to(dev)

    def call(t):
        return hyena_filter_dl(t["z"], td, t["w0"], t["b0"], t["w1"], t["b1"], t["w2"], t["b2"], t["w3"], t["freq"], dd, 0.05, True, compute_dtype=None)

    def flags(req):
        return {"filter_fwd.save": True, "filter_bwd.need_dz": "z" in req}
    return Case("HyenaFilterFunc", f"filter-fp32-L{L}-D{D}", F32, vals, call, oracle=lambda t: _filter_oracle(t, tt, deltas, 0.05), tol="op_fp32",
                flags=flags)


def case_in_proj(dev, T, B, L, D, G=3):
    from hyena_dna_amd.projection import in_proj_cm
    g = _g(B + L + D)
    vals = {"u": _rn(g, B, L, D).to(T).to(dev), "weight": _rn(g, G * D, D, scale=D ** -0.5).to(T).to(dev)}
    return Case("InProjCMFunc", f"in_proj_cm-{NAME[T]}-B{B}-L{L}-D{D}", T, vals, lambda t: in_proj_cm(t["u"], t["weight"]))


def _shell(g, D, G=3):
    return _rn(g, G * D, scale=0.1), _rn(g, G * D, 1, 3, scale=0.5), _rn(g, G * D, scale=0.1)


def case_in_proj_pre(dev, T, B, L, D):
    from hyena_dna_amd import _lib
    from hyena_dna_amd.projection import in_proj_pre_cm
    g = _g(2 * B + L + D)
    vals = {"u": _rn(g, B, L, D).to(T).to(dev), "weight": _rn(g, 3 * D, D, scale=D ** -0.5).to(T).to(dev)}
    b_in, w, b = (x.to(dev) for x in _shell(g, D))
    assert _lib.proj_supported(B, L, D, T)
    return Case("InProjPreCMFunc", f"in_proj_pre_cm-{NAME[T]}-B{B}-L{L}-D{D}", T, vals, lambda t: in_proj_pre_cm(t["u"], t["weight"], b_in, w, b, L))


def case_out_proj(dev, T, B, L, D):
    from hyena_dna_amd.projection import out_proj_cm
    g = _g(3 * B + L + D)
    vals = {"zT": _rn(g, D, B, L).to(T).to(dev), "weight": _rn(g, D, D, scale=D ** -0.5).to(T).to(dev), "bias": _rn(g, D, scale=0.1).to(T).to(dev)}
    return Case("OutProjCMFunc", f"out_proj_cm-{NAME[T]}-B{B}-L{L}-D{D}", T, vals, lambda t: out_proj_cm(t["zT"], t["weight"], t["bias"]))


def case_split_k(dev, T, rows, D, N, gpu):
    from hyena_dna_amd.projection import SplitKLinearFunc, hyena_linear
    g = _g(rows + D)
    vals = {"x": _rn(g, rows, D).to(T).to(dev), "weight": _rn(g, N, D, scale=D ** -0.5).to(T).to(dev), "bias": _rn(g, N, scale=0.1).to(T).to(dev)}
    if gpu:                                           # through the gate of hyena_linear (rows >= projection.MIN_ROWS on the device)
        call = lambda t: hyena_linear(t["x"], t["weight"], t["bias"])      # noqa: E731
    else:
        call = lambda t: SplitKLinearFunc.apply(t["x"], t["weight"], t["bias"])      # noqa: E731
    return Case("SplitKLinearFunc", f"split_k-{NAME[T]}-rows{rows}-D{D}-N{N}", T, vals, call)


def case_small_vocab(dev, n_ids, V, D, gpu):
    from types import SimpleNamespace
    from hyena_dna_amd.lm import SmallVocabEmbeddingFunc, small_vocab_embedding
    g = _g(n_ids + V)
    ids = torch.randint(0, V, (1, n_ids), generator=g).to(dev)
    vals = {"weight": _rn(g, V, D).to(dev)}
    if gpu:                                           # through the gate of small_vocab_embedding (>= 32768 ids on the device), which reads these attributes
        call = lambda t: small_vocab_embedding(ids, SimpleNamespace(weight=t["weight"], padding_idx=None, max_norm=None, sparse=False,      # noqa: E731
                                                                    num_embeddings=V))
    else:
        call = lambda t: SmallVocabEmbeddingFunc.apply(ids, t["weight"])      # noqa: E731
    return Case("SmallVocabEmbeddingFunc", f"small_vocab-ids{n_ids}-V{V}-D{D}", F32, vals, call)


def _ref_core_pm(t, L):
    D = t["x"].shape[-1] // 3
    xc = O.short_conv_taps(t["x"].transpose(1, 2), t["sf_weight"], t["sf_bias"], L)
    x0, x1, v = xc.split(D, dim=1)
    return (O.fftconv_ref(v * x1, t["k"], t["bias"]) * x0).transpose(1, 2)


def case_mixer_pm(dev, T, B, Lx, L, D):
    from hyena_dna_amd.mixer import hyena_mixer_core
    g = _g(B * 1000 + L + D)
    _, w, b = _shell(g, D)
    vals = {"x": _rn(g, B, Lx, 3 * D).to(T), "sf_weight": w, "sf_bias": b, "k": _filter_like(g, D, L), "bias": _rn(g, D)}
    vals = {n: v.to(dev) for n, v in vals.items()}
    return Case("HyenaMixerFunc", f"mixer_pm-{NAME[T]}-B{B}-Lx{Lx}-L{L}-D{D}", T, vals,
                lambda t: hyena_mixer_core(t["x"], t["sf_weight"], t["sf_bias"], t["k"], t["bias"], L),
                oracle=lambda t: _ref_core_pm(t, L), tol="op_fp32" if T == F32 else "core_16", flags=_conv_flags(("k", "bias")))


def _ref_core_cm(t, L, order=2, ks=None):
    """oracle pieces, channel-major: (x_0 ... x_n, v) = short_conv(xT + b_in).split(D); v <- conv(v x_n, k_0); v <- conv(v x_{n-o}, k_o); z = v x_0"""
    n = order - 1
    D = t["xT"].shape[0] // (order + 1)
    x = (t["xT"] + t["b_in"][:, None, None]).permute(1, 0, 2)
    xc = O.short_conv_taps(x, t["sf_weight"], t["sf_bias"], L)
    *xs, v = xc.split(D, dim=1)
    ks = [t["k"]] if ks is None else ks
    bias = t["bias"].reshape(D, n)
    for o in range(n):
        v = O.fftconv_ref(v * xs[n - o], ks[o], bias[:, o])
    return (v * xs[0]).permute(1, 0, 2)


def _cm_vals(g, T, B, Lx, L, D, order=2):
    b_in, w, b = _shell(g, D, order + 1)
    vals = {"xT": _rn(g, (order + 1) * D, B, Lx).to(T), "b_in": b_in, "sf_weight": w, "sf_bias": b}
    if order == 2:
        vals["k"] = _filter_like(g, D, L)
    vals["bias"] = _rn(g, D * (order - 1))
    for o in range(order - 1 if order > 2 else 0):
        vals[f"k{o}"] = _filter_like(g, D, L)
    return vals


def case_mixer_cm(dev, T, B, Lx, L, D):
    from hyena_dna_amd.mixer import hyena_mixer_core_cm
    vals = {n: v.to(dev) for n, v in _cm_vals(_g(7 * B + L + D), T, B, Lx, L, D).items()}
    return Case("HyenaMixerCMFunc", f"mixer_cm-{NAME[T]}-B{B}-Lx{Lx}-L{L}-D{D}", T, vals,
                lambda t: hyena_mixer_core_cm(t["xT"], t["b_in"], t["sf_weight"], t["sf_bias"], t["k"], t["bias"], L),
                oracle=lambda t: _ref_core_cm(t, L), tol="op_fp32" if T == F32 else "core_16", flags=_conv_flags(("k", "bias")))


def case_mixer_order_n(dev, T, B, L, D, order):
    from hyena_dna_amd.mixer import hyena_mixer_core_cm_order_n
    vals = {n: v.to(dev) for n, v in _cm_vals(_g(5 * B + L + D + order), T, B, L, L, D, order).items()}
    kn = [f"k{o}" for o in range(order - 1)]
    return Case("HyenaMixerCMOrderNFunc", f"mixer_order{order}-{NAME[T]}-B{B}-L{L}-D{D}", T, vals,
                lambda t: hyena_mixer_core_cm_order_n(t["xT"], t["b_in"], t["sf_weight"], t["sf_bias"], [t[n] for n in kn], t["bias"], L, order),
                oracle=lambda t: _ref_core_cm(t, L, order, [t[n] for n in kn]), tol="order_n_fp32" if T == F32 else "order_n_16",
                flags=_conv_flags(["bias"] + kn))


def case_mixer_out(dev, T, B, L, D, norm):
    from hyena_dna_amd import _lib
    from hyena_dna_amd.mixer import hyena_mixer_out_cm, mixer_out_supported
    g = _g(9 * B + L + D + int(norm))
    vals = _cm_vals(g, T, B, L, L, D)
    vals.update({"w_out": _rn(g, D, D, scale=D ** -0.5).to(T), "b_out": _rn(g, D, scale=0.1).to(T)})
    if norm:
        vals.update({"residual": _rn(g, B, L, D, scale=2.0), "ln_w": 1.0 + _rn(g, D, scale=0.1), "ln_b": _rn(g, D, scale=0.1)})
    vals = {n: v.to(dev) for n, v in vals.items()}
    eps = 1e-5

    def call(t):
        assert mixer_out_supported(_lib.as_cm(t["xT"]), L, t["w_out"]), "the fused out_proj does not serve this case"
        return hyena_mixer_out_cm(t["xT"], t["b_in"], t["sf_weight"], t["sf_bias"], t["k"], t["bias"], L, None, t["w_out"], t["b_out"],
                                  add_norm=(t["residual"], t["ln_w"], t["ln_b"], eps) if norm else None)

    def oracle(t):
        zT = _ref_core_cm(t, L)
        out = zT.permute(1, 2, 0) @ t["w_out"].t() + t["b_out"]
        if not norm:
            return out
        res = out + t["residual"]
        return F.layer_norm(res, (D,), t["ln_w"], t["ln_b"], eps), res
    core = ("xT", "b_in", "sf_weight", "sf_bias", "k", "bias")
    return Case("HyenaMixerOutCMFunc", f"mixer_out{'_addnorm' if norm else ''}-{NAME[T]}-B{B}-L{L}-D{D}", T, vals, call, oracle=oracle, tol="core_16",
                flags=_conv_flags(("k", "bias"), z=("w_out", "norm" if norm else "plain"), early=core))


def _rows_case(g, T, shape, D, with_res=True):
    vals = {"x0": _rn(g, *shape, D).to(T)}
    if with_res:
        vals["residual"] = _rn(g, *shape, D, scale=2.0)
    vals.update({"weight": 1.0 + _rn(g, D, scale=0.1), "bias": _rn(g, D, scale=0.1)})
    return vals


def case_add_norm(dev, T, shape, D, p=0.0):
    from hyena_dna_amd.block import dropout_add_layer_norm
    vals = {n: v.to(dev) for n, v in _rows_case(_g(D + shape[-1]), T, shape, D).items()}
    return Case("AddLayerNormFunc", f"add_norm-{NAME[T]}-{'x'.join(map(str, shape))}x{D}-p{p}", T, vals,
                lambda t: dropout_add_layer_norm(t["x0"], t["residual"], t["weight"], t["bias"], p, 1e-5, prenorm=True, residual_in_fp32=True),
                seed=77 if p else None)


def case_embed_add_norm(dev, shape, V, D, p=0.0):
    from hyena_dna_amd.block import embedding_dropout_add_layer_norm
    g = _g(V + D)
    ids = torch.randint(0, V, shape, generator=g).to(dev)
    vals = {"table": _rn(g, V, D).to(dev), "weight": (1.0 + _rn(g, D, scale=0.1)).to(dev), "bias": _rn(g, D, scale=0.1).to(dev)}
    return Case("EmbedAddLayerNormFunc", f"embed_add_norm-{'x'.join(map(str, shape))}-V{V}-D{D}-p{p}", F32, vals,
                lambda t: embedding_dropout_add_layer_norm(ids, t["table"], t["weight"], t["bias"], p, 1e-5), seed=78 if p else None)


def case_soft_embed(dev, shape, n, V, D, p=0.0, sp=0.0):
    from hyena_dna_amd.block import soft_embedding_dropout_add_layer_norm
    g = _g(V + D + n)
    ids = torch.randint(0, V, shape, generator=g).to(dev)
    table, w, b = _rn(g, V, D).to(dev), (1.0 + _rn(g, D, scale=0.1)).to(dev), _rn(g, D, scale=0.1).to(dev)
    vals = {"soft": _rn(g, n, D, scale=0.5).to(dev)}
    return Case("SoftEmbedAddLayerNormFunc", f"soft_embed-{'x'.join(map(str, shape))}-n{n}-V{V}-D{D}-p{p}-sp{sp}", F32, vals,
                lambda t: soft_embedding_dropout_add_layer_norm(ids, table, t["soft"], w, b, p, sp, 1e-5), seed=79 if (p or sp) else None)


def case_pool(dev, T, B, L, D, mode="mean"):
    from hyena_dna_amd.block import dropout_add_layer_norm_pool
    vals = {n: v.to(dev) for n, v in _rows_case(_g(D + L + B), T, (B, L), D).items()}
    lengths = torch.tensor([L] + [max(L - 5 * (i + 1), 1) for i in range(B - 1)]).to(dev)
    return Case("AddNormPoolFunc", f"pool-{NAME[T]}-{mode}-B{B}-L{L}-D{D}", T, vals,
                lambda t: dropout_add_layer_norm_pool(t["x0"], t["residual"], t["weight"], t["bias"], 0.0, 1e-5, lengths=lengths, mode=mode))


def case_row_head(dev, T, rows, V, D):
    from hyena_dna_amd.soft_prompt import row_head
    g = _g(rows + V + D)
    weight = _rn(g, V, D, scale=D ** -0.5).to(T).to(dev)
    vals = {"x": _rn(g, rows, D).to(T).to(dev)}
    return Case("RowHeadFunc", f"row_head-{NAME[T]}-rows{rows}-V{V}-D{D}", T, vals, lambda t: row_head(t["x"], weight))


def case_mlp(dev, T, rows, D, H):
    from hyena_dna_amd.lm import fused_mlp
    g = _g(rows + D + H)
    vals = {"x": _rn(g, rows, D).to(T), "w1": _rn(g, H, D, scale=D ** -0.5).to(T), "b1": _rn(g, H, scale=0.1).to(T),
            "w2": _rn(g, D, H, scale=H ** -0.5).to(T), "b2": _rn(g, D, scale=0.1).to(T)}
    vals = {n: v.to(dev) for n, v in vals.items()}
    return Case("FusedMlpFunc", f"fused_mlp-{NAME[T]}-rows{rows}-D{D}-H{H}", T, vals, lambda t: fused_mlp(t["x"], t["w1"], t["b1"], t["w2"], t["b2"]))


# ---- the registry: one entry per Function ---------------------------------------------------------------------------------------------------
# Emulator shapes: the smallest that still take each route.  (B, L, D) = (2, 70, 8) fp32; the fused out_proj at bf16 (2, 127, 128) and fp16
# (1, 200, 256), with and without the add + LayerNorm epilogue; order 3 at fp32 (2, 77, 8) and bf16 (2, 100, 64), order 4 at fp32 (1, 70, 8); the
# position-major core with Lx > L; block / pool / soft-embed / row-head at D = 64 (the smallest their *_supported predicates admit) on 69 rows.
# L = 2053 (fp32, D = 8): the shortest length class whose convolution backward is separate kernels per gradient (fftconv_local.route: corr<4> /
# dk<4,1>), so that need_dk=False / need_du=False really change the kernel list there; below it one kernel (small_bwd) serves every pattern.
_CM_IN = ("xT", "b_in", "sf_weight", "sf_bias", "k", "bias")
_CM_GROUPS = {"filter": ("k", "bias"), "no_filter": ("xT", "b_in", "sf_weight", "sf_bias"), "biases": ("b_in", "sf_bias", "bias"),
              "weights": ("sf_weight",), "act": ("xT",)}
_OUT_GROUPS = {"filter": ("k", "bias"), "no_filter": ("xT", "b_in", "sf_weight", "sf_bias", "w_out", "b_out"),
               "biases": ("b_in", "sf_bias", "bias", "b_out"), "weights": ("sf_weight", "w_out"), "act": ("xT",)}
_OUTN_GROUPS = dict(_OUT_GROUPS, no_filter=_OUT_GROUPS["no_filter"] + ("residual", "ln_w", "ln_b"), biases=_OUT_GROUPS["biases"] + ("ln_b",),
                    weights=_OUT_GROUPS["weights"] + ("ln_w",))


def _order_entry(order, cases):
    ks = tuple(f"k{o}" for o in range(order - 1))
    ins = ("xT", "b_in", "sf_weight", "sf_bias", "bias") + ks
    groups = {"filter": ks + ("bias",), "no_filter": ins[:4], "biases": ("b_in", "sf_bias", "bias"), "weights": ("sf_weight",), "act": ("xT",)}
    return Entry("HyenaMixerCMOrderNFunc", ins, "xT", groups, cases, dk=ks + ("bias",), route="mixer.hyena_mixer_core_cm_order_n")


_FILTER_IN = ("z", "w0", "b0", "w1", "b1", "w2", "b2", "w3", "freq")
REGISTRY = {
    "FFTConvFunc": Entry("FFTConvFunc", ("u", "k", "D"), "u", {}, [lambda d: case_fftconv(d, F32, 2, 8, 70), lambda d: case_fftconv(d, BF16, 2, 64, 100),
                                                                     lambda d: case_fftconv(d, F32, 2, 8, 2053)],
                         dk=("k", "D"), du="u", route="fftconv.fftconv_func"),
    "HyenaFilterFunc": Entry("HyenaFilterFunc", _FILTER_IN, "z", {"filter": _FILTER_IN[1:], "biases": ("b0", "b1", "b2"), "weights": ("w0", "w1", "w2", "w3"),
                                                                   "act": ("z",)},
                             [lambda d: case_filter(d, 70, 64)], route="filter.hyena_filter_dl"),
    "InProjCMFunc": Entry("InProjCMFunc", ("u", "weight"), "u", {}, [lambda d: case_in_proj(d, F32, 2, 70, 8), lambda d: case_in_proj(d, BF16, 2, 100, 64, 4)],
                          route="projection.in_proj_cm"),
    "InProjPreCMFunc": Entry("InProjPreCMFunc", ("u", "weight"), "u", {}, [lambda d: case_in_proj_pre(d, BF16, 2, 127, 128),
                                                                          lambda d: case_in_proj_pre(d, F16, 1, 200, 256)],
                             route="projection.in_proj_pre_cm"),
    "OutProjCMFunc": Entry("OutProjCMFunc", ("zT", "weight", "bias"), "zT", {}, [lambda d: case_out_proj(d, F32, 2, 70, 8),
                                                                                 lambda d: case_out_proj(d, BF16, 2, 100, 64)],
                           route="projection.out_proj_cm"),
    "SplitKLinearFunc": Entry("SplitKLinearFunc", ("x", "weight", "bias"), "x", {},
                              [lambda d: case_split_k(d, F32, 77, 8, 24, False), lambda d: case_split_k(d, BF16, 77, 64, 192, False)],
                              [lambda d: case_split_k(d, BF16, 32769, 64, 192, True), lambda d: case_split_k(d, F32, 32769, 64, 64, True)],
                              route="projection.hyena_linear (rows >= 32768 on the device; emulator: .apply)"),
    "SmallVocabEmbeddingFunc": Entry("SmallVocabEmbeddingFunc", ("weight",), None, {}, [lambda d: case_small_vocab(d, 77, 12, 8, False)],
                                     [lambda d: case_small_vocab(d, 32769, 12, 64, True)],
                                     route="lm.small_vocab_embedding (>= 32768 ids on the device; emulator: .apply)"),
    "HyenaMixerFunc": Entry("HyenaMixerFunc", ("x", "sf_weight", "sf_bias", "k", "bias"), "x", {},
                            [lambda d: case_mixer_pm(d, F32, 2, 75, 70, 8), lambda d: case_mixer_pm(d, BF16, 2, 110, 100, 64)],
                            dk=("k", "bias"), route="mixer.hyena_mixer_core (HYENA_MIXER_LAYOUT=position)"),
    "HyenaMixerCMFunc": Entry("HyenaMixerCMFunc", _CM_IN, "xT", _CM_GROUPS,
                              [lambda d: case_mixer_cm(d, F32, 2, 70, 70, 8), lambda d: case_mixer_cm(d, BF16, 2, 110, 100, 64),
                               lambda d: case_mixer_cm(d, F32, 2, 2053, 2053, 8)],
                              dk=("k", "bias"), route="mixer.hyena_mixer_core_cm"),
    "HyenaMixerOutCMFunc": Entry("HyenaMixerOutCMFunc", _CM_IN + ("w_out", "b_out"), "xT", _OUT_GROUPS,
                                 [lambda d: case_mixer_out(d, BF16, 2, 127, 128, False), lambda d: case_mixer_out(d, F16, 1, 200, 256, False)],
                                 # the device also at (2, 127, 256): mixer._dgrad_fused takes out_proj's fused input gradient there under the auto policy
                                 [lambda d: case_mixer_out(d, BF16, 2, 127, 128, False), lambda d: case_mixer_out(d, F16, 1, 200, 256, False),
                                  lambda d: case_mixer_out(d, BF16, 2, 127, 256, False)],
                                 dk=("k", "bias"), route="mixer.hyena_mixer_out_cm"),
    "HyenaMixerOutCMFunc+addnorm": Entry("HyenaMixerOutCMFunc", _CM_IN + ("w_out", "b_out", "residual", "ln_w", "ln_b"), "xT", _OUTN_GROUPS,
                                         [lambda d: case_mixer_out(d, BF16, 2, 127, 128, True), lambda d: case_mixer_out(d, F16, 1, 200, 256, True)],
                                         dk=("k", "bias"), route="mixer.hyena_mixer_out_cm(add_norm=...)"),
    "HyenaMixerCMOrderNFunc": _order_entry(3, [lambda d: case_mixer_order_n(d, F32, 2, 77, 8, 3), lambda d: case_mixer_order_n(d, BF16, 2, 100, 64, 3)]),
    "HyenaMixerCMOrderNFunc+order4": _order_entry(4, [lambda d: case_mixer_order_n(d, F32, 1, 70, 8, 4)]),
    "AddLayerNormFunc": Entry("AddLayerNormFunc", ("x0", "residual", "weight", "bias"), "x0", {},
                              [lambda d: case_add_norm(d, F32, (3, 23), 64), lambda d: case_add_norm(d, BF16, (3, 23), 64, p=0.1)],
                              route="block.dropout_add_layer_norm"),
    "EmbedAddLayerNormFunc": Entry("EmbedAddLayerNormFunc", ("table", "weight", "bias"), None, {},
                                   [lambda d: case_embed_add_norm(d, (3, 23), 12, 64), lambda d: case_embed_add_norm(d, (3, 23), 12, 64, p=0.1)],
                                   route="block.embedding_dropout_add_layer_norm"),
    "SoftEmbedAddLayerNormFunc": Entry("SoftEmbedAddLayerNormFunc", ("soft",), None, {},
                                       [lambda d: case_soft_embed(d, (3, 20), 3, 12, 64), lambda d: case_soft_embed(d, (3, 20), 3, 12, 64, p=0.1, sp=0.2)],
                                       route="block.soft_embedding_dropout_add_layer_norm"),
    "AddNormPoolFunc": Entry("AddNormPoolFunc", ("x0", "residual", "weight", "bias"), "x0", {},
                             [lambda d: case_pool(d, F32, 3, 23, 64), lambda d: case_pool(d, BF16, 3, 23, 64, mode="sum")],
                             route="block.dropout_add_layer_norm_pool"),
    "RowHeadFunc": Entry("RowHeadFunc", ("x",), "x", {}, [lambda d: case_row_head(d, F32, 69, 12, 64), lambda d: case_row_head(d, BF16, 69, 12, 64)],
                         route="soft_prompt.row_head (frozen head)"),
    "FusedMlpFunc": Entry("FusedMlpFunc", ("x", "w1", "b1", "w2", "b2"), "x", {},
                          [lambda d: case_mlp(d, BF16, 77, 128, 256), lambda d: case_mlp(d, F16, 77, 128, 256)], route="lm.fused_mlp (lm.Mlp)"),
}
MIXERS = ("FFTConvFunc", "HyenaMixerFunc", "HyenaMixerCMFunc", "HyenaMixerOutCMFunc", "HyenaMixerOutCMFunc+addnorm", "HyenaMixerCMOrderNFunc",
          "HyenaMixerCMOrderNFunc+order4")


def sweep_params(gpu):
    """[(entry key, case index, pattern name, pattern id)] of the freeze-pattern sweep"""
    out = []
    for key, e in REGISTRY.items():
        for i in range(len(e.cases(gpu))):
            for name, req in e.patterns():
                out.append((key, i, name, f"{key}-c{i}-{pattern_id(e, name, req)}"))
    return out


_cache = {}


def case_and_base(_lib, dev, key, i, gpu):
    """the case and its all-required run, built once per (entry, case, device) and shared by the patterns"""
    ck = (key, i, str(dev), gpu, _lib._backend.name)
    if ck not in _cache:
        e = REGISTRY[key]
        case = e.cases(gpu)[i](dev)
        assert tuple(case.vals) == e.inputs, (key, tuple(case.vals), e.inputs)
        _cache[ck] = (case, run(_lib, case, frozenset(e.inputs)))
    return _cache[ck]


def suite_pattern(_lib, dev, key, i, name, gpu=False):
    e = REGISTRY[key]
    req = dict(e.patterns())[name]
    case, base = case_and_base(_lib, dev, key, i, gpu)
    got = run(_lib, case, req)
    how = check_pattern(case, base, got, req, named=e.diffs(req))
    print(f"[autograd-local] {case.label} {name}: {how}", flush=True)
    return how


def suite_no_grad(_lib, dev, key, i, gpu=False):
    """the forward under torch.no_grad(): the all-required run's output bits; no spectra kept, no zT written, nothing saved by the filter"""
    case, base = case_and_base(_lib, dev, key, i, gpu)
    got = run(_lib, case, frozenset(REGISTRY[key].inputs), no_grad=True)
    for a, b in zip(got.outs, base.outs):
        assert same_bits(a.cpu(), b.cpu()), (case.label, "no_grad changes the output")
    for name, flag in (("fftconv_fwd", "save"), ("outproj_gate_fwd", "want_z"), ("outproj_gate_addnorm_fwd", "want_z"), ("filter_fwd", "save")):
        assert not any(f[flag] for f in got.spies.of(name)), (case.label, name, flag, "under no_grad")
    assert all(not o.requires_grad for o in got.outs)


def _permuted(g):
    """the same values behind a permuted, non-contiguous view"""
    if g.dim() < 2:
        return g
    perm = list(range(g.dim()))[::-1]
    return g.permute(perm).contiguous().permute(perm)


def _sliced(g):
    """the same values as a slice of a larger buffer (rows further apart, first element off the buffer's start)"""
    big = torch.full(g.shape[:-1] + (g.shape[-1] + 3,), float("nan"), dtype=g.dtype, device=g.device)
    big[..., 1:1 + g.shape[-1]] = g
    return big[..., 1:1 + g.shape[-1]]


def suite_layouts(_lib, dev, key, i, gpu=False):
    """the output gradient as a permuted view and as a slice of a larger buffer gives the bits of the contiguous gradient; expanded ones (what
    ``.sum().backward()`` hands the Function) the bits of contiguous ones"""
    e = REGISTRY[key]
    req = frozenset(e.inputs)
    case, base = case_and_base(_lib, dev, key, i, gpu)
    douts = case.douts
    for form, fn in (("permuted", _permuted), ("sliced", _sliced)):
        views = [fn(g) for g in douts]
        assert any(not v.is_contiguous() for v in views) or all(g.dim() < 2 for g in douts), form
        got = run(_lib, case, req, douts=views)
        for n in e.inputs:
            assert same_bits(got.grads[n].cpu(), base.grads[n].cpu()), (case.label, form, n)
    ones = [torch.ones_like(g) for g in douts]
    want = run(_lib, case, req, douts=ones)
    expanded = [torch.ones((), dtype=g.dtype, device=g.device).expand(g.shape) for g in douts]
    got = run(_lib, case, req, douts=expanded)
    for n in e.inputs:
        assert same_bits(got.grads[n].cpu(), want.grads[n].cpu()), (case.label, "expanded", n)
    # and literally .sum().backward()
    t = case.live(req)
    if case.seed is not None:
        torch.manual_seed(case.seed)
    outs = [o for o in _tup(case.call(t)) if o.requires_grad]
    sum(o.sum() for o in outs).backward()
    for n in e.inputs:
        assert same_bits(t[n].grad.cpu(), want.grads[n].cpu()), (case.label, ".sum().backward()", n)


def suite_retained(_lib, dev, key, i, gpu=False, env=None, mp=None, want_saved=None, builder=None):
    """three backward passes over one retained graph.  Without kept spectra all three give the same bits; with them the first backward drops
    them, the second recomputes (``spectra=absent``: another kernel list, held to the fp64 oracle gradient) and the third gives the second's bits"""
    e = REGISTRY[key]
    req = frozenset(e.inputs)
    for name, v in (env or {}).items():
        mp.setenv(name, v)
    try:
        case = (builder or e.cases(gpu)[i])(dev)
        r1, r2, r3 = run(_lib, case, req, backwards=3)
        saved = [[f["saved"] for f in r.spies.of("fftconv_bwd")] for r in (r1, r2, r3)]
        assert saved[0] and len(saved[0]) == len(saved[1]) == len(saved[2])
        assert not any(saved[1]) and not any(saved[2]), "the spectra outlive the first backward"
        if want_saved is not None:
            assert all(saved[0]) == want_saved and any(saved[0]) == want_saved, (case.label, "spectra kept by the first backward", saved[0], want_saved)
        for n in e.inputs:
            assert same_bits(r3.grads[n].cpu(), r2.grads[n].cpu()), (case.label, n, "the third backward is not the second")
        k1 = [k for k in r1.spies.kernels() if k.startswith("fftconv_bwd:")]
        k2 = [k for k in r2.spies.kernels() if k.startswith("fftconv_bwd:")]
        if any(saved[0]):
            assert k1 != k2
            ref = oracle_grads(case, req, case.douts)
            for r in (r1, r2):
                for n, g in ref.items():
                    err = _rel(r.grads[n].cpu(), g)
                    assert err < ORACLE_TOL[case.tol], (case.label, n, "spectra=absent against the fp64 oracle", err, ORACLE_TOL[case.tol])
            bits = all(same_bits(r2.grads[n].cpu(), r1.grads[n].cpu()) for n in e.inputs)
            how = "spectra=absent: " + " | ".join(k2) + "  (first: " + " | ".join(k1) + f"; bits of the first backward: {bits})"
        else:
            assert k1 == k2
            for n in e.inputs:
                assert same_bits(r2.grads[n].cpu(), r1.grads[n].cpu()), (case.label, n, "same kernels, other bits on the second backward")
            how = "same kernels"
        print(f"[autograd-local] retained {case.label}: {how}", flush=True)
        return how
    finally:
        for name in (env or {}):
            mp.delenv(name, raising=False)


# ---- the two-level plan with and without kept spectra (retained graphs): L = 3069 under HYENA_FFTCONV_ONCHIP=0, the knob of tests/fftconv_local.py ----
TWO_LEVEL_L = 3069
TWO_LEVEL_ENV = {"HYENA_FFTCONV_ONCHIP": "0"}
TWO_LEVEL = {
    "FFTConvFunc": lambda d: case_fftconv(d, F32, 2, 8, TWO_LEVEL_L),
    "HyenaMixerFunc": lambda d: case_mixer_pm(d, F32, 2, TWO_LEVEL_L + 4, TWO_LEVEL_L, 8),
    "HyenaMixerCMFunc": lambda d: case_mixer_cm(d, BF16, 2, TWO_LEVEL_L, TWO_LEVEL_L, 8),
    "HyenaMixerCMOrderNFunc": lambda d: case_mixer_order_n(d, F32, 2, TWO_LEVEL_L, 8, 3),
    "HyenaMixerOutCMFunc": lambda d: case_mixer_out(d, BF16, 2, TWO_LEVEL_L, 128, False),
}


def suite_retained_two_level(_lib, dev, mp, key, saved):
    env = dict(TWO_LEVEL_ENV, HYENA_FFTCONV_SAVE_SPECTRA="1" if saved else "0")
    return suite_retained(_lib, dev, key, None, env=env, mp=mp, want_saved=saved, builder=TWO_LEVEL[key])


# ---- the language model: activation checkpointing, freezing and the _gradsum side table ------------------------------------------------------
LM_LEN = 71                                                    # odd, and at least one 64-position tile (the fused out_proj at d_model 128)
LM_GRID = [(D, ac, order, p) for D in (64, 128) for ac in (None, BF16) for order in (2, 3) for p in (0.0, 0.1)]
CKPT = [(True, False), (False, True), (True, True)]
LM_FREEZE = {"all_trainable": lambda n: True, "biases_only": lambda n: n.endswith("bias"), "filter_only": lambda n: ".filter_fn." in n,
             "out_proj_bias_only": lambda n: n.endswith("out_proj.bias"), "fc2_bias_only": lambda n: n.endswith("fc2.bias")}
LM_CROSS = [(64, None, 2, 0.1), (128, BF16, 3, 0.1)]           # the configurations the freeze patterns are crossed with the four flag combinations at
_lm_cache = {}


def lm_id(D, ac, order, p):
    return f"D{D}-{'fp32' if ac is None else NAME[ac] + '_autocast'}-order{order}-p{p}"


def _plain_name(n):
    return n.replace(".layer.", ".")


def lm_build(dev, cfg, ck=(False, False), freeze="all_trainable", B=2):
    """the 2-layer HyenaDNALM of lm_run (torch seed 0, biases given values, ``freeze`` applied) in train mode, its ids and targets"""
    import hyena_dna_amd.lm as LM
    D, ac, order, p = cfg
    L = LM_LEN
    torch.manual_seed(0)
    layer = dict(l_max=L + 2, order=order, filter_order=64, emb_dim=5, short_filter_order=3, modulate=True, w=10)
    m = LM.HyenaDNALM(d_model=D, n_layer=2, d_inner=4 * D, vocab_size=12, layer=layer, resid_dropout=p, embed_dropout=p, pad_vocab_size_multiple=8,
                      fused_dropout_add_ln=True, residual_in_fp32=True, checkpoint_mixer=ck[0], checkpoint_mlp=ck[1]).to(dev).train()
    with torch.no_grad():                                      # (the LM initialises its biases to zero: give them values)
        g = torch.Generator().manual_seed(5)
        for n, q in m.named_parameters():
            if n.endswith("bias") and not n.endswith("filter_fn.bias"):
                q.copy_((0.1 * torch.randn(q.shape, generator=g)).to(dev))
    want = LM_FREEZE[freeze]
    for n, q in m.named_parameters():
        q.requires_grad_(bool(want(_plain_name(n))))
    ids = torch.randint(7, 11, (B, L), generator=torch.Generator().manual_seed(3)).to(dev)
    return m, ids, torch.roll(ids, -1, 1)


def lm_run(_lib, dev, cfg, ck=(False, False), freeze="all_trainable", gradsum=True, B=2):
    """one training step's loss and parameter gradients (by name, ``.layer.`` removed) of a 2-layer HyenaDNALM built from torch seed 0 and run
    from torch seed 1, with the Functions that ran and every hit of the _gradsum side table (the tensor asked about, the sums handed over)"""
    import hyena_dna_amd.lm as LM
    from hyena_dna_amd import _castcache, _gradsum
    key = (cfg, ck, freeze, gradsum, str(dev), _lib._backend.name)
    if key in _lm_cache:
        return _lm_cache[key]
    D, ac, order, p = cfg
    m, ids, tgt = lm_build(dev, cfg, ck, freeze, B)
    takes, real_take, was = [], _gradsum.take, _gradsum.ENABLED

    def take(x2):
        got = real_take(x2)
        if got is not None:
            takes.append((x2.detach().clone(), got.detach().clone()))
        return got
    _castcache.reset()
    _gradsum.reset()
    _gradsum.take, _gradsum.ENABLED = take, gradsum
    try:
        torch.manual_seed(1)
        with Spies(_lib) as sp:
            with torch.autocast(dev.type, dtype=ac or BF16, enabled=ac is not None):
                loss = m.loss(ids, tgt)
            loss.backward()
    finally:
        _gradsum.take, _gradsum.ENABLED = real_take, was
    out = {"loss": loss.detach(), "grads": {_plain_name(n): q.grad for n, q in m.named_parameters()},
           "trainable": {_plain_name(n) for n, q in m.named_parameters() if q.requires_grad}, "ran": dict(sp.ran), "takes": takes,
           "colsums": [(f) for f in sp.of("colsum")]}
    _lm_cache[key] = out
    return out


def hold_gradsum(takes):
    """every hit of the side table: the sums handed over against the float64 column sums of the very tensor, within the bound tests/block_local.py
    holds the np = 3 column sums of add_norm_bwd to (sum_bound over blk_depth(rows) additions).  -> the largest |error| / bound"""
    from tests import block_local as BL
    worst = 0.0
    for x2, sums in takes:
        x64 = x2.double().cpu()
        assert sums.dtype == F32 and sums.shape == (x2.shape[1],) and bool(torch.isfinite(sums).all())
        S = x64.abs().sum(0)
        bound = BL.sum_bound(S, torch.zeros_like(S), BL.blk_depth(x2.shape[0]), 0)
        err = (sums.double().cpu() - x64.sum(0)).abs()
        assert bool((err <= bound).all()), ("side-table sums", tuple(x2.shape), float((err / bound.clamp_min(1e-300)).max()))
        worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
    return worst


def suite_lm_checkpoint(_lib, dev, cfg, ck, freeze="all_trainable"):
    """loss and every parameter gradient of the checkpointed model are the plain model's bits, under the same freeze pattern"""
    ref = lm_run(_lib, dev, cfg, (False, False), freeze)
    got = lm_run(_lib, dev, cfg, ck, freeze)
    assert same_bits(got["loss"].cpu(), ref["loss"].cpu()), (cfg, ck, freeze, "loss", got["loss"].item(), ref["loss"].item())
    assert set(got["grads"]) == set(ref["grads"]) and got["trainable"] == ref["trainable"] and ref["trainable"]
    for n, r in ref["grads"].items():
        g = got["grads"][n]
        if n in ref["trainable"]:
            assert r is not None and g is not None, (cfg, ck, freeze, n, "a trainable parameter without a gradient")
            assert bool(torch.isfinite(g).all()) and g.shape == r.shape and g.dtype == r.dtype
            assert same_bits(g.cpu(), r.cpu()), (cfg, ck, freeze, n, "checkpointing changes the gradient")
        else:
            assert r is None and g is None, (cfg, ck, freeze, n, "a frozen parameter with a gradient")
    # the recompute really ran: the wrapped module's Functions twice
    mixer = [f for f in ("HyenaMixerCMFunc", "HyenaMixerOutCMFunc", "HyenaMixerCMOrderNFunc") if ref["ran"].get(f)]
    assert mixer
    for f in mixer:
        assert got["ran"][f] == ref["ran"][f] * (2 if ck[0] else 1), (f, got["ran"], ref["ran"])
    if ref["ran"].get("FusedMlpFunc"):
        assert got["ran"]["FusedMlpFunc"] == ref["ran"]["FusedMlpFunc"] * (2 if ck[1] else 1)
    hold_gradsum(got["takes"])
    hold_gradsum(ref["takes"])


def suite_lm_gradsum(_lib, dev, cfg, ck, freeze):
    """``out_proj.bias`` only / ``fc2.bias`` only, the side table on and off: the bias gets its gradient either way, the sums taken from the table are
    within the bound, and the two gradients agree to that bound's size (both are column sums of the same tensor)"""
    on = lm_run(_lib, dev, cfg, ck, freeze, gradsum=True)
    off = lm_run(_lib, dev, cfg, ck, freeze, gradsum=False)
    assert not off["takes"]
    hold_gradsum(on["takes"])
    assert same_bits(on["loss"].cpu(), off["loss"].cpu())
    assert on["trainable"] and on["trainable"] == off["trainable"]
    for n in on["trainable"]:
        for r in (on, off):
            g = r["grads"][n]
            assert g is not None and bool(torch.isfinite(g).all()) and bool((g != 0).any()), (cfg, ck, freeze, n)
    for n, g in on["grads"].items():
        assert (g is None) == (n not in on["trainable"]) and (off["grads"][n] is None) == (g is None), n
    return len(on["takes"])


def pattern_counts():
    return {key: (len(e.inputs), len(e.patterns()), len(e.cases(False)), len(e.cases(True))) for key, e in REGISTRY.items()}


if __name__ == "__main__":
    for key, (n_in, n_pat, ce, cg) in pattern_counts().items():
        print(f"{key}: {n_in} inputs, {n_pat} patterns, {ce} emulator cases, {cg} device cases -> {n_pat * ce} / {n_pat * cg}")
