"""Sequence classification (hyena_dna_amd.classifier, block.dropout_add_layer_norm_pool, include/hyena_block.h hyena_add_norm_pool_*) on the
CPU-emulated kernels: the fused add + LayerNorm + pooled readout against the unfused graph (dropout_add_layer_norm -> fp32 masked mean / sum),
SequenceDecoder against the reference's class, load_backbone, refusals, padding, and the runner's ``dna_embedding`` model."""
import ctypes
import os
import sys

import pytest
import torch

REF = os.environ.get("HYENA_REFERENCE", "/root/reference")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()


def _lengths(kind, B, L):
    if kind == "none":
        return None
    if kind == "full":
        return torch.full((B,), L, dtype=torch.int64)
    return torch.tensor(([0, 1, L - 1, L] * B)[:B], dtype=torch.int64)           # ragged: n_b in {0, 1, L - 1, L}


# (B, L, D): L = 37 / 70 / 9 are not multiples of the chunk (a multiple of 4 rows); 2100 x 1 and 530 x 5 spread a sequence over several
# chunks (the finish kernel's fixed-order sum over chunks, chunks past n_b that leave at once)
SHAPES = [(4, 37, 64), (4, 70, 128), (5, 9, 256), (1, 2100, 64), (5, 530, 128)]


def _pool_cases():
    import itertools
    out = []
    for shape, dtype, kind, mode, p in itertools.product(SHAPES, [torch.float32, torch.bfloat16, torch.float16], ["none", "full", "ragged"],
                                                         ["mean", "sum"], [0.0, 0.1]):
        if shape[1] > 500 and (dtype == torch.float16 or (p > 0 and mode == "sum")):
            continue                                   # the long shapes run once per remaining axis value (emulation time)
        out.append((shape, dtype, kind, mode, p))
    return out


@pytest.mark.parametrize("shape,dtype,kind,mode,p", _pool_cases())
def test_fused_pool_matches_the_unfused_graph(emu_backend, shape, dtype, kind, mode, p):
    """forward and every gradient (x0, residual, weight, bias).  The unfused graph is dropout_add_layer_norm (the add_norm kernels) followed by
    an fp32 masked mean / sum over the same inputs; with p > 0 both sides get the SAME seed, so the unfused side applies the kernel's own mask
    (the keep / drop decision is a function of (seed, linear index), test_block_emu.py checks that rule against the published generator).

    Tolerances, from the number formats (never from the fused kernel's results):
      * gradients and fp32 values: both sides compute in fp32 and differ in summation order only -> 2e-5 relative (L2), the bound
        test_block_emu.py uses for these kernels;
      * 16-bit values: the unfused route rounds every normalised element to the I/O type before the sum (relative error <= 2^-8 bf16 /
        2^-11 fp16 each: half an ulp of an 8 / 11-bit significand), the fused one does not: |difference| <= that times scale_b * sum_t |out[b, t, c]|;
      * 16-bit dx0: compared with the graph on fp32 copies of the same inputs (no 16-bit dout in between); both the stored value and the exact one
        are within half an ulp of each other -> 2^-8 / 2^-11 of the largest magnitude."""
    from hyena_dna_amd.block import AddLayerNormFunc, AddNormPoolFunc, dropout_add_layer_norm_pool, masked_pool
    B, L, D = shape
    g = torch.Generator().manual_seed(B * 1000 + L + D)
    x0 = torch.randn(shape, generator=g).to(dtype)
    residual = torch.randn(shape, generator=g) * 2
    weight = 1 + 0.2 * torch.randn(D, generator=g)
    bias = 0.1 * torch.randn(D, generator=g)
    gp = torch.randn(B, D, generator=g)
    n = _lengths(kind, B, L)
    seed = torch.tensor([0x0123_4567_89AB_CDEF], dtype=torch.int64)
    extra = (p, seed) if p > 0 else ()

    def leaves(x):
        return x.clone().requires_grad_(True), residual.clone().requires_grad_(True), weight.clone().requires_grad_(True), bias.clone().requires_grad_(True)

    xs, rs, ws, bs = leaves(x0)
    n32 = None if n is None else n.to(torch.int32)
    got = AddNormPoolFunc.apply(xs, rs, ws, bs, 1e-5, n32, mode, *extra)
    assert got.dtype == torch.float32 and got.shape == (B, D) and torch.isfinite(got).all()
    ggrads = torch.autograd.grad(got, [xs, rs, ws, bs], gp)

    def unfused(x):
        a, r, w, b = leaves(x)
        out = AddLayerNormFunc.apply(a, r, w, b, 1e-5, False, *extra)
        y = masked_pool(out, n, mode)
        return out.detach(), y, torch.autograd.grad(y, [a, r, w, b], gp)

    out_u, want, _ = unfused(x0)
    out32, want32, wgrads = unfused(x0.float())
    if dtype == torch.float32:
        assert _rel(got, want) < 2e-5, _rel(got, want)
    else:
        half_ulp = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}[dtype]
        bound = masked_pool(out32.abs(), n, mode) * half_ulp + 1e-6 + 2e-5 * want32.abs()
        assert ((got - want).abs() <= bound).all(), ((got - want).abs() - bound).max().item()
        assert _rel(got, want32) < 2e-5                                     # and against the fp32 graph: summation order only
    for name, a, r in zip(("dx0", "dresidual", "dweight", "dbias"), ggrads, wgrads):
        assert a.shape == r.shape, name
        if name == "dx0" and dtype != torch.float32:
            assert a.dtype == dtype
            tol = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}[dtype]
            assert (a.float() - r).abs().max() <= tol * r.abs().max() + 1e-7, name
        else:
            assert a.dtype == torch.float32 and _rel(a, r) < 2e-5, (name, _rel(a, r))
    if n is not None:
        for b_ in range(B):                                                      # pad rows: exactly zero gradients, n_b = 0: exactly zero output
            assert not ggrads[0][b_, int(n[b_]):].any() and not ggrads[1][b_, int(n[b_]):].any()
            if int(n[b_]) == 0:
                assert not got[b_].any()
    # the public function: same values, lengths in any integer type
    if p == 0:
        pub = dropout_add_layer_norm_pool(x0, residual, weight, bias, 0.0, 1e-5, lengths=n, mode=mode)
        assert torch.equal(pub, got.detach())
    # two runs: the same bits
    again = AddNormPoolFunc.apply(xs, rs, ws, bs, 1e-5, n32, mode, *extra)
    assert torch.equal(again, got)


def test_pool_lengths_are_clamped_and_colsum_is_offered(emu_backend):
    from hyena_dna_amd import _gradsum, _lib
    from hyena_dna_amd.block import dropout_add_layer_norm_pool
    B, L, D = 3, 21, 128
    g = torch.Generator().manual_seed(1)
    x0 = torch.randn(B, L, D, generator=g).to(torch.bfloat16).requires_grad_(True)
    res = torch.randn(B, L, D, generator=g)
    w, b = torch.ones(D), torch.zeros(D)
    wild = dropout_add_layer_norm_pool(x0, res, w, b, 0.0, 1e-5, lengths=torch.tensor([-5, 7, 10 ** 6]))
    tame = dropout_add_layer_norm_pool(x0, res, w, b, 0.0, 1e-5, lengths=torch.tensor([0, 7, L]))
    assert torch.equal(wild, tame) and not wild[0].any()
    _gradsum.reset()
    dx, = torch.autograd.grad(tame.sum(), [x0])
    sums = _gradsum.take(dx.reshape(-1, D))                 # the np == 3 path: the column sums of dx0 as stored, for the layer in front
    if _gradsum.ENABLED:
        assert sums is not None and torch.allclose(sums, dx.float().reshape(-1, D).sum(0), rtol=1e-5, atol=1e-6)
    assert _lib.add_norm_pool_supported(256, torch.bfloat16) and not _lib.add_norm_pool_supported(96, torch.bfloat16)
    assert not _lib.add_norm_pool_supported(2048, torch.float32) and not _lib.add_norm_pool_supported(256, torch.float64)


def test_pool_fallback_and_refusals(emu_backend, monkeypatch):
    from hyena_dna_amd import _lib
    from hyena_dna_amd.block import dropout_add_layer_norm_pool, masked_pool
    import torch.nn.functional as F
    x0, res = torch.randn(2, 11, 48), torch.randn(2, 11, 48)
    w, b = torch.rand(48) + 0.5, torch.randn(48)
    n = torch.tensor([4, 0])
    calls = []
    monkeypatch.setattr(_lib, "add_norm_pool_fwd", lambda *a, **k: calls.append(1))
    y = dropout_add_layer_norm_pool(x0, res, w, b, 0.0, 1e-5, lengths=n, mode="sum")        # D = 48: the same graph in torch ops
    want = masked_pool(F.layer_norm(x0 + res, (48,), w, b, 1e-5), n, "sum")
    assert not calls and torch.allclose(y, want, atol=1e-6) and not y[1].any()
    with pytest.raises(ValueError):
        dropout_add_layer_norm_pool(x0, res, w, b, 0.0, 1e-5, mode="max")
    with pytest.raises(ValueError):
        dropout_add_layer_norm_pool(x0, res, w, b, 1.0, 1e-5)
    with pytest.raises(ValueError):
        dropout_add_layer_norm_pool(x0, res, w, b, 0.0, 1e-5, lengths=torch.tensor([1.0, 2.0]))
    with pytest.raises(ValueError):
        dropout_add_layer_norm_pool(x0[0], res[0], w, b, 0.0, 1e-5)


def test_host_tensors_are_refused_by_the_product_backend():
    from hyena_dna_amd import _lib
    from hyena_dna_amd.block import dropout_add_layer_norm_pool
    assert _lib._backend.name == "hip"
    x0, res = torch.randn(2, 8, 64), torch.randn(2, 8, 64)
    with pytest.raises(_lib.HyenaLibraryError):
        dropout_add_layer_norm_pool(x0, res, torch.ones(64), torch.zeros(64), 0.0, 1e-5)
    with pytest.raises(_lib.HyenaLibraryError):
        dropout_add_layer_norm_pool(torch.randn(2, 8, 48), None, torch.ones(48), torch.zeros(48), 0.0, 1e-5)     # the torch route refuses them too


def test_pool_c_abi_refuses_bad_arguments_without_a_device():
    """the new entry points of include/hyena_block.h in the product library: host-only answers, HYENA_ERR_BAD_ARG before any launch"""
    from hyena_dna_amd import build
    L = ctypes.CDLL(build.build(verbose=False))
    L.hyena_add_norm_pool_partial_floats.restype = ctypes.c_size_t
    L.hyena_add_norm_pool_partial_floats.argtypes = [ctypes.c_int, ctypes.c_long, ctypes.c_int]
    F32, BF16 = 0, 1
    assert L.hyena_add_norm_pool_supported(256, BF16) == 1 and L.hyena_add_norm_pool_supported(1024, F32) == 1
    assert L.hyena_add_norm_pool_supported(1088, BF16) == 0 and L.hyena_add_norm_pool_supported(100, BF16) == 0 and L.hyena_add_norm_pool_supported(256, 7) == 0
    # the grid is a function of (B, L): at most 2048 workgroups over the batch, 3 D floats of backward partials each
    assert L.hyena_add_norm_pool_partial_floats(1, 1 << 20, 256) == 2048 * 3 * 256
    assert L.hyena_add_norm_pool_partial_floats(8, 32768, 256) == 8 * 256 * 3 * 256
    assert L.hyena_add_norm_pool_partial_floats(2, 159999, 256) == 2 * 1000 * 3 * 256        # 160 rows per chunk
    assert L.hyena_add_norm_pool_partial_floats(0, 8, 256) == 0
    f = ctypes.c_float
    v = ctypes.c_void_p
    one = ctypes.c_void_p(16)              # never dereferenced: the checks come first
    L.hyena_add_norm_pool_fwd.argtypes = [v, ctypes.c_int, v, v, v, f, f, v, v, ctypes.c_int, v, v, v, v, ctypes.c_int, ctypes.c_long, ctypes.c_int, v]
    L.hyena_add_norm_pool_bwd.argtypes = [v, v, ctypes.c_int, v, v, v, v, f, v, v, ctypes.c_int, v, v, v, v, v, v, ctypes.c_int, ctypes.c_long, ctypes.c_int, v]
    assert L.hyena_add_norm_pool_fwd(None, BF16, None, one, one, 1e-5, 0.0, None, None, 0, one, one, one, one, 2, 64, 256, None) == 1
    assert L.hyena_add_norm_pool_fwd(one, BF16, None, one, one, 1e-5, 0.0, None, None, 2, one, one, one, one, 2, 64, 256, None) == 1      # mode
    assert L.hyena_add_norm_pool_fwd(one, BF16, None, one, one, 1e-5, 0.1, None, None, 0, one, one, one, one, 2, 64, 256, None) == 1      # p without a seed
    assert L.hyena_add_norm_pool_fwd(one, BF16, None, one, one, 1e-5, 0.0, None, None, 0, one, one, one, one, 2, 64, 96, None) == 1       # D
    assert L.hyena_add_norm_pool_fwd(one, BF16, None, one, one, 1e-5, 0.0, None, None, 0, one, one, one, one, 0, 64, 256, None) == 1      # B
    assert L.hyena_add_norm_pool_bwd(None, one, BF16, None, one, one, one, 0.0, None, None, 0, one, None, one, one, None, one, 2, 64, 256, None) == 1
    assert L.hyena_add_norm_pool_bwd(one, one, BF16, None, one, one, one, 0.0, None, None, 0, one, None, one, one, None, None, 2, 64, 256, None) == 1


# ---- SequenceDecoder against the reference's class ----------------------------------------------------------------------------------
needs_ref = pytest.mark.skipif(not os.path.isfile(os.path.join(REF, "src", "tasks", "decoders.py")), reason="reference checkout not present")


@needs_ref
def test_sequence_decoder_matches_the_reference_class(tmp_path):
    """every supported mode / l_output / lengths / mask combination against the reference's own src.tasks.decoders.SequenceDecoder, fp32 on CPU
    tensors (tests/_decoder_worker.py: a process of its own, because the reference's imports need inert stand-ins for packages that are not
    installed -- the way tests/test_overlay_reference.py runs the reference)"""
    import subprocess
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_decoder_worker.py")], cwd=str(tmp_path), capture_output=True, text=True,
                         timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "DECODER_OK cases=44" in out.stdout, out.stdout


def test_sequence_decoder_refusals():
    from hyena_dna_amd.classifier import SequenceDecoder
    x = torch.randn(2, 6, 8)
    with pytest.raises(NotImplementedError):
        SequenceDecoder(8, mode="ragged")
    with pytest.raises(NotImplementedError):
        SequenceDecoder(8, mode="median")
    for mode in ("pool", "sum"):
        with pytest.raises(NotImplementedError):
            SequenceDecoder(8, l_output=2, mode=mode)(x)
        with pytest.raises(NotImplementedError):
            SequenceDecoder(8, mode=mode)(x)                                   # every position's running mean / sum
    with pytest.raises(ValueError):
        SequenceDecoder(8, l_output=0, use_lengths=True, mode="last")(x)


# ---- the model surface ---------------------------------------------------------------------------------------------------------------
def _layer(L):
    return dict(l_max=L + 2, order=2, filter_order=64, emb_dim=5, short_filter_order=3, modulate=True, w=10)


def _classifier(L, D=64, mode="pool", n_layer=2, d_output=2, **kw):
    from hyena_dna_amd.classifier import DNAEmbeddingModel, HyenaDNAClassifier, SequenceDecoder
    bb = DNAEmbeddingModel(d_model=D, n_layer=n_layer, d_inner=2 * D, vocab_size=12, layer=_layer(L), resid_dropout=0.0, embed_dropout=0.0,
                           pad_vocab_size_multiple=8, fused_dropout_add_ln=True, residual_in_fp32=True)
    return HyenaDNAClassifier(bb, SequenceDecoder(bb.d_output, d_output=d_output, l_output=0, mode=mode), **kw)


def test_lm_hidden_is_trunk_plus_final_norm_and_embedding_model_returns_it(emu_backend):
    from hyena_dna_amd.classifier import DNAEmbeddingModel
    from hyena_dna_amd.lm import HyenaDNALM
    L, D = 64, 64
    kw = dict(d_model=D, n_layer=2, d_inner=2 * D, vocab_size=12, layer=_layer(L), resid_dropout=0.0, embed_dropout=0.0, pad_vocab_size_multiple=8)
    torch.manual_seed(0)
    lm = HyenaDNALM(**kw).eval()
    torch.manual_seed(0)
    em = DNAEmbeddingModel(return_hidden_state=True, **kw).eval()
    assert list(lm.state_dict()) == list(em.state_dict()) and em.d_output == D
    assert em.lm_head.weight is em.backbone.embeddings.word_embeddings.weight
    ids = torch.randint(7, 11, (2, L))
    h, r = lm.trunk(ids)
    assert r.dtype == torch.float32 and h.shape == r.shape == (2, L, D)
    assert torch.equal(lm.hidden(ids), lm._final_norm(h, r))
    hid, none = em(ids)
    assert none is None and torch.equal(hid, lm.hidden(ids))
    with pytest.raises(NotImplementedError):
        DNAEmbeddingModel(fused_mlp=True, **kw)


def test_load_backbone_round_trip(emu_backend):
    from hyena_dna_amd.classifier import load_backbone
    from hyena_dna_amd.lm import HyenaDNALM
    L, D = 64, 64
    torch.manual_seed(1)
    lm = HyenaDNALM(d_model=D, n_layer=2, d_inner=2 * D, vocab_size=12, layer=_layer(L), resid_dropout=0.0, embed_dropout=0.0, pad_vocab_size_multiple=8)
    ckpt = {"model." + k: v.clone() for k, v in lm.state_dict().items()}
    torch.manual_seed(2)
    clf = _classifier(L, D)
    fresh_head = {k: v.clone() for k, v in clf.decoder.state_dict().items()}
    used = load_backbone(clf, ckpt)
    assert set(used) == set(lm.state_dict())
    for k, v in lm.state_dict().items():
        assert torch.equal(clf.backbone.state_dict()[k], v), k
    assert clf.backbone.lm_head.weight is clf.backbone.backbone.embeddings.word_embeddings.weight
    for k, v in clf.decoder.state_dict().items():
        assert torch.equal(v, fresh_head[k])
    ids = torch.randint(7, 11, (2, L))
    assert torch.equal(clf.backbone.eval()(ids)[0], lm.eval().hidden(ids))
    assert all(p.requires_grad for p in clf.parameters())
    # a key the checkpoint lacks raises; head keys may be absent (ignore_head) and are required without it
    short = {k: v for k, v in ckpt.items() if "ln_f.bias" not in k}
    with pytest.raises(KeyError):
        load_backbone(clf, short)
    no_head = {k: v for k, v in ckpt.items() if "head" not in k}
    load_backbone(clf, no_head)
    with pytest.raises(KeyError):
        load_backbone(clf, no_head, ignore_head=False)
    load_backbone(clf, ckpt, freeze_backbone=True)
    assert not any(p.requires_grad for p in clf.backbone.parameters()) and all(p.requires_grad for p in clf.decoder.parameters())


@pytest.mark.parametrize("mode", ["pool", "sum", "last", "first"])
def test_classifier_routes_agree_and_no_normalised_tensor_exists(emu_backend, monkeypatch, mode):
    """the fused readout == the unfused route (final norm over all positions, then the decoder), values and gradients; on the fused route
    _lib.add_norm_fwd is never called for ln_f -- the normalised (B, L, D) tensor does not exist"""
    from hyena_dna_amd import _lib
    L, D, B = 64, 64, 3
    torch.manual_seed(4)
    clf = _classifier(L, D, mode=mode).eval()
    ids = torch.randint(7, 11, (B, L))
    lengths = torch.tensor([L, 17, 1])
    ln_calls = []
    real = _lib.add_norm_fwd

    def spy(x0, residual, weight, bias, *a, **k):
        if torch.equal(weight, clf.backbone.backbone.ln_f.weight.detach().float()) and torch.equal(bias, clf.backbone.backbone.ln_f.bias.detach().float()):
            ln_calls.append(tuple(x0.shape))
        return real(x0, residual, weight, bias, *a, **k)

    with torch.no_grad():                                                         # ln_f has to be told apart from the blocks' norms
        clf.backbone.backbone.ln_f.weight.add_(0.25)
        clf.backbone.backbone.ln_f.bias.add_(0.5)
    monkeypatch.setattr(_lib, "add_norm_fwd", spy)
    params = [p for p in clf.parameters() if p.requires_grad]
    for n in (None, lengths):
        ln_calls.clear()
        y = clf(ids, lengths=n)
        assert y.shape == (B, 2) and y.dtype == torch.float32
        if mode in ("pool", "sum"):
            assert ln_calls == []
        else:
            assert ln_calls == [(B, D)]                                           # one row per sequence, sliced in front of the norm
        gy = torch.autograd.grad(y.square().sum(), params, allow_unused=True)
        hidden = clf.backbone(ids)[0]
        assert ln_calls[-1] == (B * L, D)
        want = clf.decoder.output_transform(clf.decoder.readout(hidden, lengths=n, use_lengths=n is not None).float())
        gw = torch.autograd.grad(want.square().sum(), params, allow_unused=True)
        assert torch.allclose(y, want, rtol=1e-4, atol=1e-5), (y - want).abs().max()
        for p_, a, b in zip(params, gy, gw):
            assert (a is None) == (b is None)
            if a is not None:
                assert _rel(a, b) < 1e-4 or (a - b).abs().max() < 1e-6
    if mode in ("pool", "sum"):
        clf.fused_readout = False
        ln_calls.clear()
        assert torch.allclose(clf(ids, lengths=lengths), y, rtol=1e-4, atol=1e-5) and ln_calls == [(B * L, D)]


def test_padded_and_unpadded_classifier_runs_agree_at_4_x_1023(emu_backend, monkeypatch):
    """the backbone's end-padding to a multiple of 64 positions never changes what is pooled: the pad positions are excluded through lengths"""
    import hyena_dna_amd.lm as LM
    B, L, D = 4, 1023, 64
    torch.manual_seed(5)
    clf = _classifier(L + 1, D, n_layer=1).eval()
    ids = torch.randint(7, 11, (B, L))
    lengths = torch.tensor([L, 1000, 64, 1])
    seen = []
    real = clf.backbone.trunk
    monkeypatch.setattr(clf.backbone, "trunk", lambda i, *a, **k: (seen.append(i.shape[1]), real(i, *a, **k))[1])
    outs = {}
    for pad in (True, False):
        monkeypatch.setattr(LM, "PAD_SEQUENCES", pad)
        outs[pad] = (clf(ids).detach(), clf(ids, lengths=lengths).detach())
    assert seen == [1024, 1024, 1023, 1023]
    for a, b in zip(outs[True], outs[False]):
        assert torch.allclose(a, b, rtol=1e-4, atol=1e-5), (a - b).abs().max()
    # a bidirectional stack runs unpadded
    monkeypatch.setattr(LM, "PAD_SEQUENCES", True)
    for m in clf.backbone._mixers():
        monkeypatch.setattr(m.filter_fn, "bidirectional", True, raising=False)
    assert clf.backbone._aligned_length(ids) == L


def test_classifier_loss_counts_lengths_from_pad_tokens(emu_backend):
    from hyena_dna_amd.runner import make_synthetic_classification
    L, D = 64, 64
    ids, lengths, labels = make_synthetic_classification(6, max_length=L, seed=3)
    assert ids.shape == (6, L) and ((ids != 4).sum(1) == lengths).all() and set(labels.tolist()) <= {0, 1}
    assert ((ids == 4) | ((ids >= 7) & (ids <= 10))).all() and (lengths >= L // 2).all() and (lengths < L).any()
    ids2, lengths2, labels2 = make_synthetic_classification(6, max_length=L, seed=3)
    assert torch.equal(ids, ids2) and torch.equal(labels, labels2)
    motif = torch.tensor(["ACGT".index(c) for c in "TATAAGGC"]) + 7
    has = torch.tensor([bool((row.unfold(0, 8, 1) == motif).all(1).any()) for row in ids])
    assert torch.equal(has, labels.bool())
    torch.manual_seed(6)
    clf = _classifier(L, D, pad_token_id=4).eval()
    assert torch.equal(clf(ids), clf(ids, lengths=lengths))
    loss = clf.loss(ids, labels)
    want = torch.nn.functional.cross_entropy(clf(ids, lengths=lengths), labels)
    assert loss.dim() == 0 and torch.allclose(loss, want, rtol=1e-5)
    loss.backward()
    assert clf.decoder.output_transform.weight.grad is not None


needs_cfg = pytest.mark.skipif(not os.path.isfile(os.path.join(REF, "configs", "experiment", "hg38", "genomic_benchmark.yaml")),
                               reason="reference checkout not present")


@needs_cfg
def test_runner_builds_the_genomic_benchmark_classifier():
    from hyena_dna_amd import runner
    from hyena_dna_amd.classifier import DNAEmbeddingModel, HyenaDNAClassifier, SequenceDecoder
    cfg = runner.compose(os.path.join(REF, "configs"), experiment="hg38/genomic_benchmark")
    assert cfg["model"]["_name_"] == "dna_embedding" and cfg["decoder"] == {"_name_": "sequence", "mode": "pool"} and cfg["dataset"]["d_output"] == 2
    model = runner.build_model(cfg)
    assert isinstance(model, HyenaDNAClassifier) and isinstance(model.backbone, DNAEmbeddingModel) and isinstance(model.decoder, SequenceDecoder)
    bb = model.backbone
    assert bb.d_model == 128 and len(bb.backbone.layers) == 2 and bb.backbone.embeddings.word_embeddings.weight.shape == (16, 128)
    assert model.decoder.mode == "pool" and model.decoder.squeeze and model.decoder.output_transform.out_features == 2
    lm_cfg = {"model": dict(cfg["model"], _name_="lm")}
    assert type(runner.build_model(lm_cfg)).__name__ == "HyenaDNALM"
    with pytest.raises(NotImplementedError):
        runner.build_model({"model": dict(cfg["model"], _name_="s4")})
    with pytest.raises(NotImplementedError):
        runner.build_model(dict(cfg, decoder={"_name_": "token"}))
